"""RMSD after best-fit superposition on the device: abopt_superposed_rmsd (every query row against every reference row) and
abopt_cluster_shapes_grouped (greedy clusters by shape), their wrappers and the two sampler functions, against the float64 statement of
tests/superpose_statement.py, which also builds the inputs and asserts the conditions they satisfy.

The bound on every RMSD is DockQ's contract of DESIGN.md section 6.7: the kernel works in double, so what remains is the rounding of the result to fp32 --
|rmsd - rmsd64| <= 2^-23 rmsd64 + 1e-6 A."""
import ctypes

import numpy as np
import pytest
import torch

import scorer_harness as harness
import screen_workers
import superpose_statement as st
from ab_opt_amd import hip, sampler, screen
from scorer_harness import DEV
from test_pose_clusters import greedy_f64

REL, ABS = 2.0 ** -23, 1e-6


def _close(got, want):
    """the bound above, elementwise; -1 (not scored) has to match exactly"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.where(want < 0, got == want, np.abs(got - want) <= REL * np.abs(want) + ABS)


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _call(c, q=None, **kw):
    return hip.superposed_rmsd(_t(c['q'] if q is None else q), _t(c['r']), qfit=_t(c['qfit']), rfit=_t(c['rfit']), qscore=_t(c['qscore']), rscore=_t(c['rscore']), **kw)


# ------------------------------------------------------------------------------------------ CPU
def test_svd_statement_equals_the_eigenvector_statement():
    """Kabsch by SVD with the determinant correction and Horn's quaternion by numpy's eigh give the same RMSD, counts, rotation and translation on every case
    (condition (b) holds on all of them, so the rotation is determined): two float64 statements of one definition."""
    for tag in st.TAGS:
        c = st.case(tag)
        a = c['want']
        b = st.rows(c['q'], c['qfit'], c['qscore'], c['r'], c['rfit'], c['rscore'], fit=st.horn)
        assert np.array_equal(a['n_fit'], b['n_fit']) and np.array_equal(a['n_score'], b['n_score']), tag
        far = 1e3 if tag.startswith('far') else 1.0                 # t = cy - R cx carries the rotation's error times |cx|
        assert np.allclose(a['rmsd'], b['rmsd'], rtol=1e-9, atol=1e-9) and np.allclose(a['rot'], b['rot'], atol=1e-9) and \
            np.allclose(a['trans'], b['trans'], atol=1e-8 * far), tag


def test_cases_hold_what_they_claim():
    """The conditions of every case hold (they are asserted where a case is built), and few seeds were passed over to find them."""
    for tag in st.TAGS:
        c = st.case(tag)
        assert st.conditions(c) == [] and c['seeds_tried'] < 50, (tag, c['seeds_tried'])
    for S, n in st.CLUSTER_SHAPES:
        c = st.cluster_case(S, n)
        assert c['margin'] > st.MARGIN and c['seeds_tried'] < 50, (S, n, c['margin'], c['seeds_tried'])
        if S > 1:
            for g in range(st.CLUSTER_G):
                label = st.greedy_shapes(c['rm'][g], c['tight'])[0]
                assert st.same_partition(label, c['family'][g]), (S, n, g)


def test_a_mirror_image_has_a_nonzero_rmsd():
    """Proper rotations only: a chiral set of four points against its mirror image cannot be superposed (the best improper fit would give 0)."""
    x = np.array([[0.0, 0, 0], [2.0, 0, 0], [0, 3.0, 0], [0, 0, 1.5]])
    y = x * np.array([1.0, 1.0, -1.0])
    for fit in (st.kabsch, st.horn):
        p = st.pair(x, None, None, y, None, None, fit=fit)
        assert p['rmsd'] > 0.5 and abs(np.linalg.det(p['rot']) - 1.0) < 1e-12, (fit.__name__, p['rmsd'])
    assert st.pair(x, None, None, x @ st._rotation(np.array([1.0, 2, 3]), 1.1).T + 5.0, None, None)['rmsd'] < 1e-12


def test_a_hand_worked_three_point_case():
    """x = (-1, 0, 0), (1, 0, 0), (0, 1, 0) onto y = (-1, 0, 0), (1, 0, 0), (0, 4, 0).  Centroids (0, 1/3, 0) and (0, 4/3, 0); the covariance of the centred
    points is diag(2, 8/3, 0), so the best rotation is the identity and t = (0, 1, 0); the residuals are (0, 1), (0, 1), (0, -2): ss = 6, rmsd = sqrt 2.
    Scored on the third point alone the deviation is 2.  Two fit points, or counts that differ, are not scored."""
    x = np.array([[-1.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]])
    y = np.array([[-1.0, 0, 0], [1.0, 0, 0], [0, 4.0, 0]])
    for fit in (st.kabsch, st.horn):
        p = st.pair(x, None, None, y, None, None, fit=fit)
        assert abs(p['rmsd'] - np.sqrt(2.0)) < 1e-12 and np.allclose(p['rot'], np.eye(3), atol=1e-12) and np.allclose(p['trans'], [0, 1, 0], atol=1e-12)
        assert (p['n_fit'], p['n_score']) == (3, 3)
        last = np.array([False, False, True])
        p = st.pair(x, None, last, y, None, last, fit=fit)
        assert abs(p['rmsd'] - 2.0) < 1e-12 and (p['n_fit'], p['n_score']) == (3, 1)
    two = np.array([True, True, False])
    for p in (st.pair(x, two, None, y, two, None), st.pair(x, None, None, y, two, None), st.pair(x, None, two, y, None, None),
              st.pair(x, None, ~(two | ~two), y, None, ~(two | ~two))):
        assert p['rmsd'] == -1.0 and p['n_fit'] == 0 and p['n_score'] == 0 and np.array_equal(p['rot'], np.eye(3)) and not p['trans'].any()


def test_the_greedy_walk_is_that_of_the_pose_clusters():
    """greedy_walk over the unsuperposed relation is greedy_f64 of tests/test_pose_clusters.py, capped and uncapped: the statement of the shape clusters
    differs from that of the pose clusters in the relation alone."""
    rng = np.random.default_rng(3)
    x = (rng.normal(size=(40, 5, 3)) * 2.0).astype(np.float32)
    for cutoff in (1.5, 2.5, 3.5):
        for cap in (0, 3):
            want = greedy_f64(x, cutoff, cap)
            got = st.greedy_walk(st.plain_rmsd(x, x) <= cutoff, cap)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (cutoff, cap)


def test_bad_arguments_are_refused_before_any_launch():
    """Every ValueError of the two wrappers and the two sampler functions on CPU tensors (nothing has touched a device), the refusal of a CPU tensor once
    everything else is valid, and the return codes of the C entries on dummy pointers that are never dereferenced."""
    q, r = torch.zeros(3, 9, 3), torch.zeros(2, 9, 3, dtype=torch.float64)
    sr = hip.superposed_rmsd
    for bad in (q[0], q[:, :, :2], q.long()):
        with pytest.raises(ValueError, match=r'q .* must be floating point \(rows, n, 3\)'):
            sr(bad, r)
    with pytest.raises(ValueError, match=r'r .* must be floating point'):
        sr(q, r.long())
    with pytest.raises(ValueError, match='r has 257 elements per row, expected 1 .. 256'):
        sr(q, torch.zeros(2, 257, 3))
    with pytest.raises(ValueError, match='q has 0 elements per row'):
        sr(q[:, :0], r)
    with pytest.raises(ValueError, match=r'mask of q .* must be \(rows, n\)'):
        sr(q, r, qfit=torch.ones(3, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match=r'mask of r .* must be \(rows, n\)'):
        sr(q, r, rfit=torch.ones(3, 9, dtype=torch.bool))
    with pytest.raises(ValueError, match=r'qscore .* must be \(rows, n\)'):
        sr(q, r, qscore=torch.ones(3, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match=r'rscore .* must be \(rows, n\)'):
        sr(q, r, rscore=torch.ones(3, 9, dtype=torch.bool))
    with pytest.raises(ValueError, match='HIP device only'):        # everything valid: the CPU tensor is refused before anything is allocated
        sr(q, r, qfit=torch.ones(3, 9, dtype=torch.bool), want_transform=True)
    ca = torch.zeros(4, 3, 3)
    cs = hip.cluster_shapes_grouped
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='cluster_shapes_grouped: cutoff must be finite and >= 0'):
            cs(ca, 4, bad)
        with pytest.raises(ValueError, match='cluster_shapes: cutoff must be finite and >= 0'):
            sampler.cluster_shapes(ca, bad)
    with pytest.raises(ValueError, match='whole groups'):
        cs(ca, 3, 2.0)
    with pytest.raises(ValueError, match='whole groups'):
        cs(torch.zeros(4, 3), 4, 2.0)
    with pytest.raises(ValueError, match='have 2 points, expected 3 .. 256'):
        cs(torch.zeros(4, 2, 3), 4, 2.0)
    with pytest.raises(ValueError, match='have 257 points, expected 3 .. 256'):
        cs(torch.zeros(4, 257, 3), 4, 2.0)
    with pytest.raises(ValueError, match='max_clusters must be >= 0'):
        cs(ca, 4, 2.0, max_clusters=-1)
    with pytest.raises(RuntimeError, match='HIP device only'):      # valid arguments reach the binding, which has no CPU path
        cs(ca, 4, 2.0, max_clusters=2)
    for bad in (0, -3):
        with pytest.raises(ValueError, match='cluster_shapes: max_clusters must be >= 1 or None'):
            sampler.cluster_shapes(ca, 2.0, max_clusters=bad)
    for bad in (torch.zeros(4, 3), torch.zeros(4, 2, 3), torch.zeros(4, 257, 3), torch.zeros(0, 5, 3)):
        with pytest.raises(ValueError, match=r'cluster_shapes: expected \(P, n, 3\) structures with P >= 1 and 3 <= n <= 256'):
            sampler.cluster_shapes(bad, 2.0)
    batch = dict(aa=torch.zeros(1, 9, dtype=torch.long), generate_flag=torch.zeros(1, 9, dtype=torch.bool), fragment_type=torch.ones(1, 9, dtype=torch.long),
                 pos_heavyatom=torch.zeros(1, 9, 4, 3), mask_heavyatom=torch.ones(1, 9, 4, dtype=torch.bool))
    pos, mask = torch.zeros(1, 9, 4, 3), torch.ones(1, 9, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match="fit must be 'generated', 'context', 'antibody' or a"):
        sampler.superposed_rmsd(batch, pos, mask, fit='designed')
    with pytest.raises(ValueError, match="score must be 'generated', 'context', 'antibody' or a"):
        sampler.superposed_rmsd(batch, pos, mask, score='loop')
    with pytest.raises(ValueError, match=r'expected pos \(G\*S, L, A >= 2, 3\)'):
        sampler.superposed_rmsd(batch, pos[:, :, :1], mask[:, :, :1])
    with pytest.raises(ValueError, match=r'expected pos \(G\*S, L, A >= 2, 3\)'):
        sampler.superposed_rmsd(batch, pos, mask, fit=torch.ones(1, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match='ref_fit / ref_score select residues of ref_ca'):
        sampler.superposed_rmsd(batch, pos, mask, ref_fit=torch.ones(1, 9, dtype=torch.bool))
    with pytest.raises(ValueError, match='HIP device only'):
        sampler.superposed_rmsd(batch, pos, mask, fit='antibody')

    L_ = hip.lib()
    dummy = (ctypes.c_char * 16)()
    a = ctypes.c_void_p(ctypes.addressof(dummy))

    def rmsd(Q=3, R=2, na=9, nb=12, q=a, n_score=a):
        return L_.abopt_superposed_rmsd(q, None, None, a, None, None, Q, R, na, nb, a, a, n_score, None, None, None)
    for kw, rc, word in ((dict(na=257), 3, '256'), (dict(nb=257), 3, '256'), (dict(na=0), 1, 'bad dims'), (dict(Q=-1), 1, 'bad dims'),
                         (dict(Q=65536, R=65536), 1, 'bad dims'), (dict(Q=0, na=257), 3, '256'), (dict(q=None), 1, 'NULL'), (dict(n_score=None), 1, 'NULL')):
        assert rmsd(**kw) == rc and word in L_.abopt_last_error().decode(), (kw, L_.abopt_last_error().decode())
    assert rmsd(Q=0, q=None) == 0 and rmsd(R=0) == 0                 # no-ops, between the value checks and the pointer checks

    def shapes(G=2, S=5, n=7, cutoff=2.0, cap=0, ws_bytes=1 << 20, structs=a):
        return L_.abopt_cluster_shapes_grouped(structs, G, S, n, cutoff, cap, a, ws_bytes, a, a, a, a, None, None)
    for kw, rc, word in ((dict(G=1, S=16385), 3, '16385'), (dict(n=257), 3, '256'), (dict(n=2), 1, 'n >= 3'), (dict(n=0), 1, 'bad dims'), (dict(S=0), 1, 'bad dims'),
                         (dict(cap=-1), 1, 'bad dims'), (dict(cutoff=-1.0), 1, 'cutoff'), (dict(cutoff=float('nan')), 1, 'cutoff'),
                         (dict(cutoff=float('inf')), 1, 'cutoff'), (dict(G=65536, S=1), 1, '65535'), (dict(structs=None), 1, 'NULL'),
                         (dict(ws_bytes=7), 4, 'workspace too small')):
        assert shapes(**kw) == rc and word in L_.abopt_last_error().decode(), (kw, L_.abopt_last_error().decode())
    assert shapes(G=0, structs=None) == 0


def test_binding_and_header_agree_on_the_new_entries():
    """The export list still equals the header (tests/test_abi.py checks every signature; this names the two new ones), and the ABI is still 59."""
    from test_abi import parse_header, signature_mismatches
    protos = parse_header()[0]
    assert {'abopt_superposed_rmsd', 'abopt_cluster_shapes_grouped'} <= set(protos) and set(hip.EXPORTS) == set(protos)
    assert signature_mismatches(hip._SIGNATURES, protos) == {}
    assert hip.ABI_VERSION == 59 and hip.lib().abopt_abi_version() == 59
    assert len(protos['abopt_superposed_rmsd'][1]) == 16 and len(protos['abopt_cluster_shapes_grouped'][1]) == 14
    assert protos['abopt_cluster_shapes_grouped'][1] == protos['abopt_cluster_poses_grouped'][1]


# ------------------------------------------------------------------------------------------ GPU: every query against every reference
@pytest.mark.gpu
@pytest.mark.parametrize('tag', st.TAGS)
def test_device_equals_the_statement(tag):
    """n_fit, n_score and the not-scored pairs exactly, rmsd within the bound, on every length class, NULL masks, masks that are no prefixes, score sets other
    than the fit sets, pairs with mismatched counts, fewer than three fit points and empty rows, and coordinates far from the origin."""
    c = st.case(tag)
    got = {k: v.cpu().numpy() for k, v in _call(c, want_transform=True).items()}
    w = c['want']
    assert got['rmsd'].dtype == np.float32 and got['n_fit'].dtype == np.int32 and got['n_score'].dtype == np.int32
    assert np.array_equal(got['n_fit'], w['n_fit']) and np.array_equal(got['n_score'], w['n_score']), tag
    off = w['n_fit'] == 0
    assert (got['rmsd'][off] == -1).all() and (got['rot'][off] == np.eye(3, dtype=np.float32)).all() and (got['trans'][off] == 0).all(), tag
    err = np.abs(got['rmsd'].astype(np.float64) - w['rmsd'])
    print(tag, 'max |rmsd - rmsd64| =', err.max(), 'at rmsd64 up to', w['rmsd'].max())
    assert _close(got['rmsd'], w['rmsd']).all(), (tag, err.max())
    plain = _call(c)
    assert set(plain) == {'rmsd', 'n_fit', 'n_score'} and all(np.array_equal(plain[k].cpu().numpy(), got[k]) for k in plain), tag


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ('null_16', 'null_65', 'score_63_255', 'far_64'))
def test_rigid_invariance(tag):
    """Every query moved by a random rotation and translation (float64, rounded to fp32): the RMSD equals the statement on the moved values within the same
    bound, and stays where it was up to the rounding of the moved coordinates, while the unsuperposed RMSD of hip.gapped_rmsd moves by more than 1 A."""
    c = st.case(tag)
    q2, want = st.moved(c)
    before, after = _call(c)['rmsd'].cpu().numpy(), _call(c, q=q2)['rmsd'].cpu().numpy()
    assert _close(after, want['rmsd']).all(), (tag, np.abs(after - want['rmsd']).max())
    if c['kind'] == 'null':
        # score == fit: the RMSD is a minimum over the transforms.  The moved coordinates are rounded to fp32, each point moves by at most sqrt(3) half-ulps
        # of the largest coordinate, under every transform the RMSD (a norm of the residuals) moves by no more, and so does its minimum.
        drift = np.sqrt(3.0) * 2.0 ** -24 * max(np.abs(q2).max(), np.abs(c['q']).max())
        assert (np.abs(after.astype(np.float64) - before) <= drift + REL * np.abs(before) + ABS).all(), tag
        r = _t(c['r'])
        g0, g1 = hip.gapped_rmsd(_t(c['q']), r)['rmsd'].cpu().numpy(), hip.gapped_rmsd(_t(q2), r)['rmsd'].cpu().numpy()
        assert (np.abs(g1 - g0) > 1.0).all(), (tag, np.abs(g1 - g0).min())


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ('null_3', 'null_64', 'score_16_15', 'far_score_17_65'))
def test_transform(tag):
    """rot is orthonormal with determinant +1, and applying (rot, trans) to the query's score points in float64 reproduces rmsd.  h = 2^-25 bounds the rounding
    of an entry of rot (|entry| <= 1: half an ulp below 1) and 2^-24 |t_j| that of an entry of trans; the double arithmetic behind them errs at the 1e-15 level.
      orthonormality  rot = R + E with R orthonormal, |E_ij| <= h:  rot^T rot - 1 = R^T E + E^T R + E^T E, and |(R^T E)_ij| <= h sum_k |R_ki| <= sqrt(3) h,
                      so every entry is within 2 sqrt(3) h + 3 h^2;  det(rot) = det(1 + R^T E) = 1 + tr(R^T E) + O(h^2), within 3 sqrt(3) h (1 + 0.01)
      rmsd            the residual of a score point x moves by E x + tau: |(E x)_j| <= h (|x_0| + |x_1| + |x_2|) <= sqrt(3) h |x| and |tau_j| <= 2^-24 max|t|, so
                      every residual moves by at most D = 3 h X + sqrt(3) 2^-24 T, X = the largest |x| of the query (uncentred: rot acts on x as it
                      is), T = max |t_j|; the RMSD is a norm of the residuals, so it moves by at most D; the returned rmsd is itself rounded once (2^-24)."""
    c = st.case(tag)
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in _call(c, want_transform=True).items()}
    h = 2.0 ** -25
    on = np.argwhere(got['n_fit'] > 0)
    assert len(on)
    for i, j in on:
        rot, t = got['rot'][i, j], got['trans'][i, j]
        assert np.abs(rot.T @ rot - np.eye(3)).max() <= 2 * np.sqrt(3) * h + 3 * h * h + 1e-14, (tag, i, j)
        assert abs(np.linalg.det(rot) - 1.0) <= 3 * np.sqrt(3) * h * 1.01 + 1e-14, (tag, i, j)
        xs = c['q'][i][(c['qfit'] if c['qscore'] is None else c['qscore'])[i]] if c['qfit'] is not None else c['q'][i]
        ys = c['r'][j][(c['rfit'] if c['rscore'] is None else c['rscore'])[j]] if c['rfit'] is not None else c['r'][j]
        D = 3 * h * np.linalg.norm(xs.astype(np.float64), axis=1).max() + np.sqrt(3) * 2.0 ** -24 * np.abs(t).max()
        again = st.rmsd_under(rot, t, xs, ys)
        assert abs(again - got['rmsd'][i, j]) <= D + 2.0 ** -24 * 1.001 * got['rmsd'][i, j] + 1e-12, (tag, i, j, again, got['rmsd'][i, j], D)
        # and it is the statement's rotation: condition (b) leaves both float64 solves some 1e-13 of freedom (1e-16 over the eigen-gap), the rest is h
        assert np.abs(rot - c['want']['rot'][i, j]).max() <= h + 1e-10, (tag, i, j)


@pytest.mark.gpu
def test_a_call_equals_its_single_pair_calls():
    c = st.case('score_16_15')
    t = dict(q=_t(c['q']), r=_t(c['r']), qfit=_t(c['qfit']), rfit=_t(c['rfit']), qscore=_t(c['qscore']), rscore=_t(c['rscore']))
    whole = hip.superposed_rmsd(**t, want_transform=True)
    assert int((whole['n_fit'] > 0).sum()) >= 4
    for x in range(0, t['q'].shape[0], 3):
        for y in range(t['r'].shape[0]):
            one = hip.superposed_rmsd(**{k: v[x:x + 1] if k.startswith('q') else v[y:y + 1] for k, v in t.items()}, want_transform=True)
            harness.assert_same_results(one, {k: v[x:x + 1, y:y + 1] for k, v in whole.items()}, (x, y))


@pytest.mark.gpu
def test_cluster_rmsd_matrix_is_symmetric_and_equals_the_pair_entry():
    """The optional rmsd of the cluster entry equals its transpose bit for bit, is 0 on the diagonal, equals abopt_superposed_rmsd on rows (min, max) of the same
    structures with NULL masks bit for bit, and lies within the bound of float64.  Asking for it does not change the clusters."""
    for S, n in ((65, 3), (65, 16), (129, 40)):
        c = st.cluster_case(S, n)
        xd = _t(c['x'])
        out = hip.cluster_shapes_grouped(xd, S, c['mixed'], want_rmsd=True)
        rm = out['rmsd']
        assert rm.shape == (st.CLUSTER_G, S, S) and rm.dtype == torch.float32
        assert torch.equal(rm, rm.transpose(1, 2).contiguous()), (S, n)
        assert (torch.diagonal(rm, dim1=1, dim2=2) == 0).all(), (S, n)
        for g in range(st.CLUSTER_G):
            pairs = hip.superposed_rmsd(xd[g * S:(g + 1) * S], xd[g * S:(g + 1) * S])['rmsd']
            upper = torch.triu(pairs, 1)                             # entry (a, b) with a < b: query a = row min, reference b = row max
            assert torch.equal(rm[g], upper + upper.t()), (S, n, g)
        assert _close(rm.cpu().numpy(), c['rm']).all(), (S, n, np.abs(rm.cpu().numpy() - c['rm']).max())
        plain = hip.cluster_shapes_grouped(xd, S, c['mixed'])
        for k in ('label', 'centre', 'size', 'count'):
            assert torch.equal(out[k], plain[k]), (S, n, k)


@pytest.mark.gpu
def test_folded_grid():
    """R just past the 2^22 workgroups of one grid row (16 reference rows each, Q = 2 in one tile row): the pairs of the second grid row equal a small call bit
    for bit, like all the others, and that small call the statement.  The rows are drawn from eight distinct ones per side, n = 3."""
    rng = np.random.default_rng(13)
    Q, R, n = 2, 16 * (1 << 22) + 1, 3
    base = dict(q=(rng.normal(size=(8, n, 3)) * 3).astype(np.float32), r=(rng.normal(size=(8, n, 3)) * 3).astype(np.float32), qfit=rng.random((8, n)) < 0.9,
                rfit=rng.random((8, n)) < 0.9)
    assert base['qfit'].all(1).any() and base['rfit'].all(1).any() and not base['rfit'].all()
    want = st.rows(base['q'], base['qfit'], None, base['r'], base['rfit'], None)
    small = hip.superposed_rmsd(_t(base['q']), _t(base['r']), qfit=_t(base['qfit']), rfit=_t(base['rfit']))
    assert np.array_equal(small['n_fit'].cpu().numpy(), want['n_fit']) and _close(small['rmsd'].cpu().numpy(), want['rmsd']).all() and (want['n_fit'] > 0).any()
    iq, ir = torch.from_numpy(rng.integers(0, 8, Q)).to(DEV), torch.from_numpy(rng.integers(0, 8, R)).to(DEV)
    d = {k: _t(v)[iq if k.startswith('q') else ir].contiguous() for k, v in base.items()}
    got = hip.superposed_rmsd(d['q'], d['r'], qfit=d['qfit'], rfit=d['rfit'])
    for name in ('rmsd', 'n_fit', 'n_score'):
        assert torch.equal(got[name], small[name][iq][:, ir]), name


@pytest.mark.gpu
def test_calls_are_capturable():
    """Both calls recorded with torch.cuda.graph and replayed on OTHER inputs copied into the static tensors give what the eager calls give on them."""
    a, b = st.case('score_16_15'), st.build('score_16_15', 99)
    names = ('q', 'r', 'qfit', 'rfit', 'qscore', 'rscore')
    call = lambda **t: hip.superposed_rmsd(**t, want_transform=True)
    t, other = {k: _t(a[k]) for k in names}, {k: _t(b[k]) for k in names}
    eager = {k: v.clone() for k, v in call(**t).items()}
    first, held = harness.capture_replays_on_other_inputs(call, t, other)
    harness.assert_same_results(first, eager, 'the first replay against the eager call')
    assert not torch.equal(held['rmsd'], first['rmsd'])
    c = st.cluster_case(65, 16)
    call = lambda structs: hip.cluster_shapes_grouped(structs, 65, c['mixed'], want_rmsd=True)
    x1, x2 = _t(c['x']), _t(c['x'][::-1].copy())
    eager = {k: v.clone() for k, v in call(structs=x1).items()}
    first, held = harness.capture_replays_on_other_inputs(call, dict(structs=x1), dict(structs=x2))
    harness.assert_same_results(first, eager, 'the first replay against the eager call')
    assert not torch.equal(held['rmsd'], first['rmsd'])


@pytest.mark.gpu
def test_empty_calls_and_unsupported_width():
    z = lambda *s: torch.zeros(*s, device=DEV)
    out = hip.superposed_rmsd(z(0, 9, 3), z(4, 5, 3), want_transform=True)
    assert tuple(out['rmsd'].shape) == (0, 4) and tuple(out['rot'].shape) == (0, 4, 3, 3) and tuple(out['trans'].shape) == (0, 4, 3)
    assert tuple(hip.superposed_rmsd(z(4, 5, 3), z(0, 9, 3))['n_fit'].shape) == (4, 0)
    wide = z(2, 257, 3)
    f = torch.full((2, 2, 9), 7.0, device=DEV)
    i = torch.full((2, 2), 7, dtype=torch.int32, device=DEV)
    rc = hip.lib().abopt_superposed_rmsd(hip.ptr(wide), None, None, hip.ptr(wide), None, None, 2, 2, 257, 257, hip.ptr(f), hip.ptr(i), hip.ptr(i), hip.ptr(f),
                                         hip.ptr(f), hip.stream())
    torch.cuda.synchronize()
    assert rc == 3 and bool((f == 7).all()) and bool((i == 7).all())    # ABOPT_EUNSUPPORTED, and nothing was launched
    empty = hip.cluster_shapes_grouped(z(0, 7, 3), 5, 1.0)
    assert empty['label'].shape == (0,) and empty['count'].shape == (0,)


# ------------------------------------------------------------------------------------------ GPU: clusters by shape
def _assert_equals_statement(out, c, S, cutoff, cap, tag):
    label, centre, size, count = (out[k].cpu().numpy() for k in ('label', 'centre', 'size', 'count'))
    G = st.CLUSTER_G
    assert label.shape == (G * S,) and centre.shape == (G, S) and size.shape == (G, S) and count.shape == (G,), tag
    for g in range(G):
        wl, wc, ws = st.greedy_shapes(c['rm'][g], cutoff, cap)
        C = len(wc)
        assert count[g] == C, (tag, g, count[g], C)
        assert np.array_equal(label[g * S:(g + 1) * S], wl), (tag, g)
        assert np.array_equal(centre[g, :C], wc) and (centre[g, C:] == -1).all(), (tag, g)
        assert np.array_equal(size[g, :C], ws) and (size[g, C:] == 0).all(), (tag, g)
        if cap:
            assert C <= cap and (wl == -1).sum() == S - ws.sum(), (tag, g)


@pytest.mark.gpu
def test_shape_clusters_recover_the_families_and_equal_the_greedy_statement():
    """G = 3, S in {1, 63, 64, 65, 129}, n in {3, 16, 40}: members of four shape families, each rigidly displaced at random plus 0.05 A noise.  At the cutoff
    between the within-family and the between-family RMSDs the shape clusters ARE the families, where cluster_poses_grouped on the same input finds only
    singletons; at a cutoff among the between-family RMSDs (clusters that merge families) and with max_clusters 1 and 3, label, centre, size and count are
    those of the float64 greedy statement."""
    for S, n in st.CLUSTER_SHAPES:
        c = st.cluster_case(S, n)
        xd = _t(c['x'])
        out = hip.cluster_shapes_grouped(xd, S, c['tight'])
        _assert_equals_statement(out, c, S, c['tight'], 0, (S, n, 'tight'))
        if S > 1:
            poses = hip.cluster_poses_grouped(xd, S, c['tight'])
            for g in range(st.CLUSTER_G):
                assert st.same_partition(out['label'][g * S:(g + 1) * S].cpu().numpy(), c['family'][g]), (S, n, g)
                assert not st.same_partition(poses['label'][g * S:(g + 1) * S].cpu().numpy(), c['family'][g]) and poses['count'][g].item() == S, (S, n, g)
        for cap in (0, 1, 3):
            out = hip.cluster_shapes_grouped(xd, S, c['mixed'], max_clusters=cap)
            _assert_equals_statement(out, c, S, c['mixed'], cap, (S, n, 'mixed', cap))
    c = st.cluster_case(129, 16)
    assert not st.same_partition(st.greedy_shapes(c['rm'][0], c['mixed'])[0], c['family'][0])      # the mixed cutoff merges families: another walk than the tight one
    got = sampler.cluster_shapes(_t(c['x'][:129]), c['mixed'], max_clusters=3)
    wl, wc, ws = st.greedy_shapes(c['rm'][0], c['mixed'], 3)
    assert all(got[k].dtype == torch.int64 and got[k].is_cuda for k in ('label', 'centre', 'size'))
    assert got['label'].tolist() == wl.tolist() and got['centre'].tolist() == wc.tolist() and got['size'].tolist() == ws.tolist()


@pytest.mark.gpu
def test_degenerate_cutoffs_and_nan():
    """c = 0: S singletons with centres 0 .. S - 1 (no two structures of the inputs fit exactly); a huge c: one cluster of S centred at 0; a structure with a
    NaN coordinate, at index 3 and at index 64 (the second word of the bit rows), is a singleton and the call returns."""
    for S, n in ((1, 16), (65, 3), (129, 40)):
        c = st.cluster_case(S, n)
        xd = _t(c['x'][:S])
        out = hip.cluster_shapes_grouped(xd, S, 0.0)
        assert out['count'].item() == S and out['label'].tolist() == list(range(S)) and out['centre'][0].tolist() == list(range(S))
        assert out['size'][0].tolist() == [1] * S
        for huge in (1e6, 3e38):
            out = hip.cluster_shapes_grouped(xd, S, huge)
            assert out['count'].item() == 1 and out['label'].tolist() == [0] * S
            assert out['centre'][0].tolist() == [0] + [-1] * (S - 1) and out['size'][0].tolist() == [S] + [0] * (S - 1)
    c = st.cluster_case(65, 16)
    bad = c['x'][:65].copy()
    bad[3, 5, 1] = np.nan
    bad[64, 0, 0] = np.nan
    rm = st.shape_rmsd(bad)
    assert np.isnan(rm[3, :3]).all() and np.isnan(rm[:64, 64]).all()
    for cut in (c['mixed'], 1e6):
        out = hip.cluster_shapes_grouped(_t(bad), 65, cut, want_rmsd=True)
        wl, wc, ws = st.greedy_shapes(rm, cut)
        assert out['count'].item() == len(wc) and out['label'].tolist() == wl.tolist() and out['centre'][0, :len(wc)].tolist() == wc.tolist()
        lab, size = out['label'].cpu().numpy(), out['size'][0].cpu().numpy()
        assert size[lab[3]] == 1 and size[lab[64]] == 1 and int(out['size'].sum()) == 65
        off = torch.ones(65, dtype=torch.bool, device=DEV)
        off[3] = False
        assert torch.isnan(out['rmsd'][0, 3][off]).all() and torch.isnan(out['rmsd'][0, :64, 64]).all() and out['rmsd'][0, 3, 3].item() == 0


@pytest.mark.gpu
def test_grouped_call_equals_per_group_calls():
    for S, n in ((63, 3), (64, 16), (65, 40), (129, 16)):
        c = st.cluster_case(S, n)
        for cap in (0, 2):
            call = lambda structs: hip.cluster_shapes_grouped(structs, S, c['mixed'], max_clusters=cap, want_rmsd=True)
            harness.grouped_equals_per_group(call, [((S, n, cap), st.CLUSTER_G, S, dict(structs=_t(c['x'])))], ('centre', 'size', 'count', 'rmsd'))


@pytest.mark.gpu
def test_cluster_refusals_arrive_before_any_launch():
    """S = 16385 and n = 257 (ABOPT_EUNSUPPORTED), n = 2, a negative, a NaN and an infinite cutoff (ABOPT_EINVAL) and a short workspace (ABOPT_EWORKSPACE)
    through the C entry point: the return codes, and label / centre / size / count / rmsd keep the pattern they were filled with.  The wrapper raises."""
    L_ = hip.lib()
    G, S, n = 2, 65, 16
    xd = _t(st.cluster_case(65, 16)['x'])
    fill = lambda *shape: torch.full(shape, 77, dtype=torch.int32, device=DEV)
    label, centre, size, count = fill(G * S), fill(G * S), fill(G * S), fill(G)
    rmsd = torch.full((G, S, S), 77.0, device=DEV)
    need = L_.abopt_cluster_ws_bytes(G, S)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def call(G=G, S=S, n=n, cutoff=2.0, cap=0, ws_bytes=need):
        return L_.abopt_cluster_shapes_grouped(hip.ptr(xd), G, S, n, cutoff, cap, hip.ptr(ws), ws_bytes, hip.ptr(label), hip.ptr(centre), hip.ptr(size),
                                               hip.ptr(count), hip.ptr(rmsd), hip.stream())
    assert call(G=1, S=16385) == 3 and '16385' in L_.abopt_last_error().decode()
    assert call(n=257) == 3 and '256' in L_.abopt_last_error().decode()
    assert call(n=2) == 1 and 'n >= 3' in L_.abopt_last_error().decode()
    assert call(cutoff=-1.0) == 1 and call(cutoff=float('nan')) == 1 and call(cutoff=float('inf')) == 1 and 'cutoff' in L_.abopt_last_error().decode()
    assert call(S=0) == 1 and call(cap=-1) == 1 and call(G=-1) == 1
    assert call(ws_bytes=need - 1) == 4 and 'workspace too small' in L_.abopt_last_error().decode()
    assert call(G=0) == 0                                            # a no-op
    torch.cuda.synchronize()
    for t in (label, centre, size, count):
        assert (t == 77).all()
    assert (rmsd == 77.0).all()
    assert call() == 0                                               # ... and the same buffers are filled by a good call
    torch.cuda.synchronize()
    assert (label != 77).all() and (count != 77).all() and (rmsd != 77.0).all()
    with pytest.raises(RuntimeError, match='abopt error 3'):
        hip.cluster_shapes_grouped(torch.zeros(16385, 3, 3, device=DEV), 16385, 1.0)


# ------------------------------------------------------------------------------------------ GPU: the sampler functions on the screen's complex
@pytest.mark.gpu
def test_sampler_functions_on_the_screen_complex():
    """The native against itself gives 0; the native with its generated loop rigidly displaced gives ~0 fitted on the loop itself and the displacement's RMS
    deviation fitted on the context and scored on the loop; reference loops of the loop's length give (G*S, R); cluster_shapes over the loops of two poses'
    designs equals hip.cluster_shapes_grouped."""
    one = screen_workers.complex_(DEV)
    pos, mask = one['pos_heavyatom'], one['mask_heavyatom']
    gen = one['generate_flag'][0].bool()
    n = int(gen.sum())
    ctx = (screen.chain_groups(one['fragment_type'])[0] == 1) & ~gen
    assert n >= 8 and int(ctx.sum()) >= 8
    res = sampler.superposed_rmsd(one, pos, mask)
    assert set(res) == {'rmsd', 'n_fit', 'n_score'} and tuple(res['rmsd'].shape) == (1,)
    assert 0 <= res['rmsd'].item() <= ABS and res['n_fit'].tolist() == [n] == res['n_score'].tolist()
    rng = np.random.default_rng(5)
    R, t = st.random_motion(rng, 3.0)
    native = pos[0].cpu().numpy().astype(np.float64)
    loop = gen.cpu().numpy()
    moved64 = native.copy()
    moved64[loop] = native[loop] @ R.T + t
    moved = torch.from_numpy(moved64.astype(np.float32)).to(DEV)[None]
    # fitted on the loop itself: what the rounding of the moved coordinates leaves (each moves by at most sqrt(3) half-ulps of the largest coordinate)
    own = sampler.superposed_rmsd(one, moved, mask, fit='generated')
    assert 0 <= own['rmsd'].item() <= np.sqrt(3.0) * 2.0 ** -24 * np.abs(moved64).max() + ABS and own['n_fit'].tolist() == [n]
    # fitted on the context, which did not move (the fit is the identity), scored on the loop: the RMS displacement of the loop's CA, by the statement
    ca_ok = (mask[0, :, 1].bool() & gen).cpu().numpy()
    want = st.pair(moved64.astype(np.float32)[:, 1], (ctx & mask[0, :, 1].bool()).cpu().numpy(), ca_ok, native[:, 1], (ctx & mask[0, :, 1].bool()).cpu().numpy(), ca_ok)
    fw = sampler.superposed_rmsd(one, moved, mask, fit='context', score='generated', want_transform=True)
    assert want['rmsd'] > 1.0 and _close(fw['rmsd'].cpu().numpy(), [want['rmsd']]).all() and fw['n_fit'].tolist() == [want['n_fit']] and fw['n_score'].tolist() == [n]
    assert tuple(fw['rot'].shape) == (1, 3, 3) and tuple(fw['trans'].shape) == (1, 3) and np.abs(fw['rot'][0].cpu().numpy() - np.eye(3)).max() < 1e-5
    # a panel of reference loops: the native loop, and the moved one
    refs = torch.stack([pos[0, gen, 1], moved[0, gen, 1]])
    S = 4
    both = torch.cat([pos, moved]).repeat(2, 1, 1, 1)
    panel = sampler.superposed_rmsd(one, both, mask.expand(S, -1, -1), ref_ca=refs)
    assert tuple(panel['rmsd'].shape) == (S, 2) and bool((panel['rmsd'] >= 0).all()) and bool((panel['rmsd'] <= 1e-5).all()) and bool((panel['n_fit'] == n).all())
    assert bool((sampler.superposed_rmsd(one, both, mask.expand(S, -1, -1), fit='antibody')['rmsd'][[1, 3]] > 0.1).all())
    # the loops of the designs of two poses: a few noisy variants of the native loop and of a bent one, each pose in its own frame
    loop_ca = native[loop][:, 1]
    bent = loop_ca.copy()
    bent[n // 2:] = (bent[n // 2:] - bent[n // 2]) @ st._rotation(np.array([0.3, 1.0, 0.2]), 0.9).T + bent[n // 2]
    cas = []
    for pose in range(2):
        Rp, tp = st.random_motion(rng, 20.0)
        for k in range(6):
            cas.append((bent if k % 2 else loop_ca) @ Rp.T + tp + rng.normal(size=(n, 3)) * 0.05)
    ca = torch.from_numpy(np.stack(cas).astype(np.float32)).to(DEV)
    got = sampler.cluster_shapes(ca, 0.6)
    raw = hip.cluster_shapes_grouped(ca, 12, 0.6)
    C = raw['count'].item()
    assert C == 2 and got['label'].tolist() == raw['label'].tolist() and got['centre'].tolist() == raw['centre'][0, :C].tolist()
    assert got['size'].tolist() == raw['size'][0, :C].tolist() == [6, 6] and got['label'].tolist() == [0, 1] * 6
    assert sampler.cluster_poses(ca, 0.6)['centre'].numel() == 4     # without superposition: the two shapes of either pose, four clusters
