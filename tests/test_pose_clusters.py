"""Pose clustering: abopt_cluster_poses_grouped / hip.cluster_poses_grouped / sampler.cluster_poses and the clustered screen
(screen.optimize_antibody(cluster_cutoff=..., max_clusters=..., redock_cutoff=...)).

The definition is restated below in numpy / float64 (`greedy_f64`).  fp32 and float64 may disagree on a pair whose RMSD sits on the cutoff, so no test
input has one: `case` builds clustered inputs and `cutoff_with_margin` moves a nominal cutoff c into the widest gap between the float64 pairwise
RMSDs inside [0.9 c, 1.1 c]; every use asserts that no pair lies within 1e-3 c of the cutoff actually used.  (fp32's error bound on ssd is
(3 n + 2) 2^-24 relative -- two roundings for (a - b)^2 and one per fma of the chain --, 9e-6 at n = 50; on the RMSD it is half of that.)"""
import functools

import numpy as np
import pytest
import torch

import pose_cluster_workers
import scorer_harness as harness
import screen_workers
from ab_opt_amd import screen
from ab_opt_amd.model import generate_mask_from_str
from scorer_harness import screen_models                           # noqa: F401 (the fixture)

DEV = torch.device('cuda:0')
SHAPES = [(G, S, n) for G in (1, 3) for S in (1, 2, 63, 64, 65, 130) for n in (1, 7, 50)]          # S: word boundaries of the bit rows
NOMINAL = (1.5, 2.0, 4.0)


# ------------------------------------------------------------------------------------------ the float64 statement and the inputs
def pair_rmsd_f64(x):
    """(S, n, 3) -> (S, S) float64 RMSD without superposition."""
    x = np.asarray(x, dtype=np.float64)
    d = x[:, None] - x[None]
    return np.sqrt((d * d).sum((2, 3)) / x.shape[1])


def greedy_f64(x, cutoff, max_clusters=0):
    """The definition (include/abopt.h: abopt_cluster_poses_grouped) for ONE group x (S, n, 3), in float64 -> (label [S], centre [C], size [C])."""
    x = np.asarray(x, dtype=np.float64)
    S, n = x.shape[:2]
    d = x[:, None] - x[None]
    with np.errstate(invalid='ignore'):
        adj = (d * d).sum((2, 3)) <= float(cutoff) ** 2 * n          # NaN compares False
    adj[np.arange(S), np.arange(S)] = True                          # the diagonal is always set
    alive = np.ones(S, dtype=bool)
    label, centre, size = -np.ones(S, dtype=np.int64), [], []
    while alive.any() and not (max_clusters and len(centre) >= max_clusters):
        cnt = (adj & alive[None]).sum(1)
        cnt[~alive] = -1
        c = int(np.argmax(cnt))                                     # the first maximum: ties go to the lowest index
        members = adj[c] & alive
        label[members] = len(centre)
        centre.append(c)
        size.append(int(members.sum()))
        alive &= ~members
    return label, np.array(centre, dtype=np.int64), np.array(size, dtype=np.int64)


def _raw_structures(G, S, n, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(5, n, 3)) * 8.0
    which = rng.integers(0, 5, size=G * S)
    sigma = rng.choice([0.3, 1.0, 2.5], size=G * S)
    return (centres[which] + rng.normal(size=(G * S, n, 3)) * sigma[:, None, None]).astype(np.float32)


def cutoff_with_margin(rmsds, c):
    """The midpoint of the widest gap between consecutive sorted values of `rmsds` inside [0.9 c, 1.1 c] (the window's ends close the first and the
    last gap) -> (cutoff, distance of the nearest value to it)."""
    r = np.sort(np.asarray(rmsds, dtype=np.float64).reshape(-1))
    r = r[np.isfinite(r)]
    pts = np.concatenate([[0.9 * c], r[(r > 0.9 * c) & (r < 1.1 * c)], [1.1 * c]])
    i = int(np.argmax(np.diff(pts)))
    cut = 0.5 * (pts[i] + pts[i + 1])
    return cut, (np.abs(r - cut).min() if r.size else np.inf)


@functools.lru_cache(maxsize=None)
def case(G, S, n):
    """Inputs with a margin, built once per shape and shared by the tests: 5 centres (normal x 8 A), a random centre per structure, jitter with sigma from
    {0.3, 1.0, 2.5} A, rounded to fp32 -> (x [G*S, n, 3] fp32 numpy, {nominal cutoff: cutoff}, float64 RMSDs [G, S, S]).  The seed is the first one whose
    structures leave, for every nominal cutoff, a gap of more than 2e-3 c in the window (a dense shape such as (3, 130, 50) has ~600 pairs inside it)."""
    for seed in range(200):
        x = _raw_structures(G, S, n, 1000 * seed + 7 * S + n + G)
        rm = np.stack([pair_rmsd_f64(x[g * S:(g + 1) * S]) for g in range(G)])
        iu = np.triu_indices(S, 1)
        pairs = np.concatenate([rm[g][iu] for g in range(G)])
        cuts = {c: cutoff_with_margin(pairs, c) for c in NOMINAL}
        if all(m > 1e-3 * c for c, (_, m) in cuts.items()):
            break
    for c, (cut, margin) in cuts.items():
        assert margin > 1e-3 * c and 0.9 * c <= cut <= 1.1 * c, (G, S, n, c, cut, margin)       # a condition on the inputs, not on the code
    return x, {c: cut for c, (cut, _) in cuts.items()}, rm


def _assert_equals_statement(out, x, G, S, cutoff, max_clusters, tag):
    label, centre, size, count = (out[k].cpu().numpy() for k in ('label', 'centre', 'size', 'count'))
    assert label.shape == (G * S,) and centre.shape == (G, S) and size.shape == (G, S) and count.shape == (G,), tag
    for g in range(G):
        wl, wc, ws = greedy_f64(x[g * S:(g + 1) * S], cutoff, max_clusters)
        C = len(wc)
        assert count[g] == C, (tag, g, count[g], C)
        assert np.array_equal(label[g * S:(g + 1) * S], wl), (tag, g)
        assert np.array_equal(centre[g, :C], wc) and (centre[g, C:] == -1).all(), (tag, g)
        assert np.array_equal(size[g, :C], ws) and (size[g, C:] == 0).all(), (tag, g)
        if max_clusters:
            assert C <= max_clusters and (wl == -1).sum() == S - ws.sum(), (tag, g)


# ------------------------------------------------------------------------------------------ CPU
def test_greedy_statement_on_a_hand_worked_example_with_a_tie():
    """Six points on a line (n = 1, so the RMSD is the distance), cutoff 1.5: neighbour counts 2, 3, 2, 2, 2, 1.  Structure 1 is picked first (3) and takes
    {0, 1, 2}; structures 3 and 4 then tie at 2 and the lower index wins; 5 is a singleton.  With a cap of 2, structure 5 keeps label -1.  A second line
    where EVERY count ties at 2 gives the centres 0, 2, 4."""
    line = lambda *v: np.array(v, dtype=np.float64).reshape(-1, 1, 1) * np.array([1.0, 0.0, 0.0])
    label, centre, size = greedy_f64(line(0, 1, 2, 10, 11, 20), 1.5)
    assert label.tolist() == [0, 0, 0, 1, 1, 2] and centre.tolist() == [1, 3, 5] and size.tolist() == [3, 2, 1]
    label, centre, size = greedy_f64(line(0, 1, 2, 10, 11, 20), 1.5, max_clusters=2)
    assert label.tolist() == [0, 0, 0, 1, 1, -1] and centre.tolist() == [1, 3] and size.tolist() == [3, 2]
    label, centre, size = greedy_f64(line(0, 1, 10, 11, 20, 21), 1.5)
    assert label.tolist() == [0, 0, 1, 1, 2, 2] and centre.tolist() == [0, 2, 4] and size.tolist() == [2, 2, 2]
    # clusters are numbered in order of discovery, not by position: the chain 0-1-2-3-4 loses {0, 1, 2} to the first pick, then 31 (count 3) goes before 3 (2 left)
    label, centre, size = greedy_f64(line(0, 1, 2, 3, 4, 30, 31, 32), 1.5)
    assert centre.tolist() == [1, 6, 3] and size.tolist() == [3, 3, 2] and label.tolist() == [0, 0, 0, 2, 2, 1, 1, 1]
    # a NaN structure is its own singleton, and the loop terminates
    x = line(0, 1, 2, 3)
    x[2, 0, 1] = np.nan
    label, centre, size = greedy_f64(x, 1.5)
    assert label.tolist() == [0, 0, 1, 2] and centre.tolist() == [0, 2, 3] and size.tolist() == [2, 1, 1]


def test_cutoff_arguments_are_validated_without_a_device():
    """sampler.cluster_poses and optimize_antibody refuse negative / non-finite cutoffs and max_clusters < 1 with ValueError before anything touches a
    device: the tensors here live on the CPU and the models are None."""
    from ab_opt_amd import hip, sampler
    from ab_opt_amd.utils import synth
    ca = torch.zeros(4, 3, 3)
    for bad in (-1.0, float('nan'), float('inf'), -0.5):
        with pytest.raises(ValueError, match='finite and >= 0'):
            sampler.cluster_poses(ca, bad)
        with pytest.raises(ValueError, match='finite and >= 0'):
            hip.cluster_poses_grouped(ca, 4, bad)
    for bad in (0, -3):
        with pytest.raises(ValueError, match='max_clusters'):
            sampler.cluster_poses(ca, 2.0, max_clusters=bad)
    with pytest.raises(ValueError, match='max_clusters'):
        hip.cluster_poses_grouped(ca, 4, 2.0, max_clusters=-1)
    with pytest.raises(ValueError, match='whole groups'):
        hip.cluster_poses_grouped(ca, 3, 2.0)
    with pytest.raises(ValueError, match=r'\(P, n, 3\)'):
        sampler.cluster_poses(torch.zeros(4, 3), 2.0)
    with pytest.raises(RuntimeError, match='HIP device only'):          # valid arguments reach the binding, which has no CPU path
        sampler.cluster_poses(ca, 2.0, max_clusters=2)
    one = synth.make_batch(1, synth.LAYOUT_128, seed=21)
    call = lambda **kw: screen.optimize_antibody(None, None, one, 4, 2, 2, **kw)
    for name in ('cluster_cutoff', 'redock_cutoff'):
        for bad in (-1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError, match=name):
                call(**{name: bad})
    for bad in (0, -1):
        with pytest.raises(ValueError, match='max_clusters'):
            call(cluster_cutoff=2.0, max_clusters=bad)
    with pytest.raises(ValueError, match='needs cluster_cutoff'):
        call(max_clusters=3)


# ------------------------------------------------------------------------------------------ GPU: the kernels
@pytest.mark.gpu
def test_clusters_equal_the_float64_greedy_statement():
    """label, centre, size and count of the device call are exactly those of the numpy / float64 statement, over S in {1, 2, 63, 64, 65, 130} x n in {1, 7, 50}
    x G in {1, 3} at nominal cutoffs 1.5, 2.0 and 4.0 A (moved into a gap of the inputs, see the module docstring), uncapped and with max_clusters 1 and 3
    (poses left over at the cap: label -1).  The inputs produce multi-member clusters, singletons and ties."""
    from ab_opt_amd import hip
    for G, S, n in SHAPES:
        x, cuts, _ = case(G, S, n)
        xd = torch.from_numpy(x).to(DEV)
        for c in NOMINAL:
            for cap in (0, 1, 3):
                out = hip.cluster_poses_grouped(xd, S, cuts[c], max_clusters=cap)
                _assert_equals_statement(out, x, G, S, cuts[c], cap, (G, S, n, c, cap))
    x, cuts, _ = case(1, 130, 7)
    _, _, size = greedy_f64(x, cuts[2.0])
    assert (size > 1).sum() >= 2 and (size == 1).sum() >= 1, size      # the inputs exercise both kinds of cluster
    # sampler.cluster_poses: the same clusters as int64, sliced to the C found
    from ab_opt_amd import sampler
    got = sampler.cluster_poses(torch.from_numpy(x).to(DEV), cuts[2.0], max_clusters=3)
    wl, wc, ws = greedy_f64(x, cuts[2.0], 3)
    assert all(got[k].dtype == torch.int64 and got[k].is_cuda for k in ('label', 'centre', 'size'))
    assert got['label'].tolist() == wl.tolist() and got['centre'].tolist() == wc.tolist() and got['size'].tolist() == ws.tolist()


@pytest.mark.gpu
def test_rmsd_matrix_is_symmetric_and_matches_float64():
    """The optional rmsd output: equal to its transpose bit for bit (one fma chain in index order for (a, b) and (b, a)), zero on the diagonal, and within
    the fp32 bound of float64: ssd carries (3 n + 2) u relative (u = 2^-24: two roundings in (a - b)^2, one per fma), the correctly rounded division and
    square root add u / 2 + u after the root halves what came before, so |rmsd - rmsd64| <= ((3 n + 2) / 2 + 3 / 2) u rmsd64 (x 1.001 for the second-order
    terms).  Asking for the matrix does not change the clusters."""
    from ab_opt_amd import hip
    u = 2.0 ** -24
    for G, S, n in SHAPES:
        x, cuts, rm64 = case(G, S, n)
        xd = torch.from_numpy(x).to(DEV)
        out = hip.cluster_poses_grouped(xd, S, cuts[2.0], want_rmsd=True)
        rm = out['rmsd']
        assert rm.shape == (G, S, S) and rm.dtype == torch.float32
        assert torch.equal(rm, rm.transpose(1, 2).contiguous()), (G, S, n)
        assert (torch.diagonal(rm, dim1=1, dim2=2) == 0).all(), (G, S, n)
        bound = ((3 * n + 2) / 2 + 1.5) * u * 1.001
        err = np.abs(rm.cpu().numpy().astype(np.float64) - rm64)
        assert (err <= bound * rm64).all(), (G, S, n, (err / np.maximum(rm64, 1e-300)).max(), bound)
        plain = hip.cluster_poses_grouped(xd, S, cuts[2.0])
        for k in ('label', 'centre', 'size', 'count'):
            assert torch.equal(out[k], plain[k]), (G, S, n, k)


@pytest.mark.gpu
def test_degenerate_cutoffs():
    """c = 0: S singletons with centres 0 .. S - 1; a huge c: one cluster of S centred at 0 (every count ties); duplicated structures merge at c = 0 (the
    triplet is found first); a structure with a NaN coordinate is a singleton and the call returns."""
    from ab_opt_amd import hip
    for S, n in ((1, 7), (65, 7), (130, 50)):
        x, cuts, _ = case(1, S, n)
        xd = torch.from_numpy(x).to(DEV)
        out = hip.cluster_poses_grouped(xd, S, 0.0)
        assert out['count'].item() == S and out['label'].tolist() == list(range(S)) and out['centre'][0].tolist() == list(range(S))
        assert out['size'][0].tolist() == [1] * S
        for huge in (1e6, 3e38):                                    # 3e38^2 n overflows fp32: the threshold is +inf
            out = hip.cluster_poses_grouped(xd, S, huge)
            assert out['count'].item() == 1 and out['label'].tolist() == [0] * S
            assert out['centre'][0].tolist() == [0] + [-1] * (S - 1) and out['size'][0].tolist() == [S] + [0] * (S - 1)
    x, cuts, _ = case(1, 65, 7)
    dup = x.copy()
    dup[9] = dup[64] = dup[2]
    dup[30] = dup[11]
    out = hip.cluster_poses_grouped(torch.from_numpy(dup).to(DEV), 65, 0.0)
    _assert_equals_statement(out, dup, 1, 65, 0.0, 0, 'duplicates')
    assert out['count'].item() == 62 and out['centre'][0, :2].tolist() == [2, 11] and out['size'][0, :3].tolist() == [3, 2, 1]
    assert out['label'][[2, 9, 64]].tolist() == [0, 0, 0] and out['label'][[11, 30]].tolist() == [1, 1]
    bad = x.copy()
    bad[3, 5, 1] = np.nan
    bad[64, 0, 0] = np.nan                                           # in the second word of the bit rows
    for c in (cuts[2.0], 1e6):
        out = hip.cluster_poses_grouped(torch.from_numpy(bad).to(DEV), 65, c, want_rmsd=True)
        _assert_equals_statement(out, bad, 1, 65, c, 0, ('nan', c))
        lab = out['label'].cpu().numpy()
        size = out['size'][0].cpu().numpy()
        assert size[lab[3]] == 1 and size[lab[64]] == 1 and int(out['size'].sum()) == 65
        assert torch.isnan(out['rmsd'][0, 3]).all() and torch.isnan(out['rmsd'][0, :, 64]).all()


@pytest.mark.gpu
def test_grouped_call_equals_per_group_calls():
    """G = 3 groups in one call against three G = 1 calls: torch.equal on label, centre, size, count and the rmsd matrix."""
    from ab_opt_amd import hip
    for _, S, n in [s for s in SHAPES if s[0] == 3]:
        x, cuts, _ = case(3, S, n)
        xd = torch.from_numpy(x).to(DEV)
        for cap in (0, 2):
            got = hip.cluster_poses_grouped(xd, S, cuts[1.5], max_clusters=cap, want_rmsd=True)
            for g in range(3):
                one = hip.cluster_poses_grouped(xd[g * S:(g + 1) * S], S, cuts[1.5], max_clusters=cap, want_rmsd=True)
                assert torch.equal(got['label'][g * S:(g + 1) * S], one['label']), (S, n, cap, g)
                for k in ('centre', 'size', 'count', 'rmsd'):
                    assert torch.equal(got[k][g:g + 1], one[k]), (S, n, cap, g, k)


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    """S = 16385 (ABOPT_EUNSUPPORTED), a negative and a NaN cutoff, n = 0, max_clusters < 0 (ABOPT_EINVAL) and a short workspace (ABOPT_EWORKSPACE) through
    the C entry point: the return codes, and label / centre / size / count / rmsd keep the pattern they were filled with.  The Python wrapper raises."""
    from ab_opt_amd import hip
    L_ = hip.lib()
    G, S, n = 2, 65, 7
    x, cuts, _ = case(1, 130, 7)
    xd = torch.from_numpy(x).to(DEV)
    fill = lambda *shape: torch.full(shape, 77, dtype=torch.int32, device=DEV)
    label, centre, size, count = fill(G * S), fill(G * S), fill(G * S), fill(G)
    rmsd = torch.full((G, S, S), 77.0, device=DEV)
    need = hip.lib().abopt_cluster_ws_bytes(G, S)
    assert need == G * S * 2 * 8 + G * S * 4 and L_.abopt_cluster_ws_bytes(1, 16385) == 0 and L_.abopt_cluster_ws_bytes(0, 5) == 0
    assert L_.abopt_cluster_ws_bytes(1, 16384) == 16384 * 256 * 8 + 16384 * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def call(G=G, S=S, n=n, cutoff=2.0, cap=0, ws_bytes=need):
        return L_.abopt_cluster_poses_grouped(hip.ptr(xd), G, S, n, cutoff, cap, hip.ptr(ws), ws_bytes, hip.ptr(label), hip.ptr(centre), hip.ptr(size),
                                              hip.ptr(count), hip.ptr(rmsd), hip.stream())
    assert call(G=1, S=16385) == 3 and '16385' in L_.abopt_last_error().decode()
    assert call(cutoff=-1.0) == 1 and call(cutoff=float('nan')) == 1 and call(cutoff=float('inf')) == 1
    assert 'cutoff' in L_.abopt_last_error().decode()
    assert call(n=0) == 1 and call(S=0) == 1 and call(cap=-1) == 1 and call(G=-1) == 1
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
        hip.cluster_poses_grouped(torch.zeros(16385, 1, 3, device=DEV), 16385, 1.0)
    with pytest.raises(ValueError, match='finite and >= 0'):
        hip.cluster_poses_grouped(xd, 65, -2.0)
    empty = hip.cluster_poses_grouped(torch.zeros(0, 7, 3, device=DEV), 5, 1.0)
    assert empty['label'].shape == (0,) and empty['count'].shape == (0,)


# ------------------------------------------------------------------------------------------ GPU: the clustered screen
def _pair_gap_cutoff(ca):
    """A cutoff that merges exactly the closest pair of poses: halfway between the two smallest float64 pairwise RMSDs; the margin (relative to the
    cutoff) is asserted > 1e-3, as for every input of this file."""
    rm = pair_rmsd_f64(ca.detach().cpu().numpy())
    r = np.sort(rm[np.triu_indices(rm.shape[0], 1)])
    cut = 0.5 * (r[0] + r[1])
    assert r[1] - cut > 1e-3 * cut, ('the closest two pairs of poses are too close to one another to place a cutoff between them', r[:3])
    return float(cut)


def _stage1(dock, one, P, seed):
    from ab_opt_amd import geometry, hip, sampler
    rep = lambda t, n: t.expand(n, *t.shape[1:]).contiguous()
    gen = one['generate_flag'][0]
    t1 = sampler.sample_replicated(dock, one, P, dict(sample_structure=True, sample_sequence=False, seed=screen.stage_seed(seed, 'dock'), rng_offset=0))[0]
    g1 = rep(gen[None], P)
    pos, mask = geometry.reconstruct_backbone_partially(rep(one['pos_heavyatom'], P), hip.so3_exp(t1[0]), t1[1], torch.where(g1, t1[2], rep(one['aa'], P)),
                                                        rep(one['chain_nb'], P), rep(one['res_nb'], P), rep(one['mask_heavyatom'], P), g1)
    return t1[1][:, gen], pos, mask


def _stages23(dock, design, one, pose_pos, pose_mask, S, k, D, contig, seed):
    """Stages 2 and 3 of the screen on the given poses, written out with the public calls (tests/test_screen.py: _composition, from its second stage on)."""
    from ab_opt_amd import geometry, hip, sampler
    rep = lambda t, n: t.expand(n, *t.shape[1:]).contiguous()
    aa, cn, rn = one['aa'], one['chain_nb'], one['res_nb']
    gen = one['generate_flag'][0]
    P = pose_pos.shape[0]
    dflag = gen & generate_mask_from_str(contig, gen)
    cx = [dict(one, pos_heavyatom=pose_pos[i:i + 1], mask_heavyatom=pose_mask[i:i + 1], generate_flag=dflag[None]) for i in range(P)]
    t2 = sampler.sample_grouped(design, cx, S, dict(sample_structure=False, sample_sequence=True, seed=screen.stage_seed(seed, 'design'), rng_offset=0))[0]
    g2 = rep(dflag[None], P * S)
    aa2 = torch.where(g2, t2[2], rep(aa, P * S))
    des_pos, des_mask = geometry.reconstruct_backbone_partially(pose_pos.repeat_interleave(S, 0), hip.so3_exp(t2[0]), t2[1], aa2, rep(cn, P * S), rep(rn, P * S),
                                                                pose_mask.repeat_interleave(S, 0), g2)
    ppl = t2[4].to(DEV).view(P, S)
    chosen = torch.sort(ppl, dim=1, stable=True)[1][:, :k]
    out = dict(seqs=t2[2][:, dflag].view(P, S, -1), ppl=ppl, chosen=chosen)
    rows = (torch.arange(P, device=DEV)[:, None] * S + chosen).reshape(-1)
    npos, nmask, naa = des_pos[rows], des_mask[rows], aa2[rows]
    cx = [dict(one, pos_heavyatom=npos[i:i + 1], mask_heavyatom=nmask[i:i + 1], aa=naa[i:i + 1], generate_flag=gen[None]) for i in range(P * k)]
    t3 = sampler.sample_grouped(dock, cx, D, dict(sample_structure=True, sample_sequence=False, seed=screen.stage_seed(seed, 'redock'), rng_offset=0))[0]
    g3 = rep(gen[None], P * k * D)
    rpos, rmask = geometry.reconstruct_backbone_partially(npos.repeat_interleave(D, 0), hip.so3_exp(t3[0]), t3[1], torch.where(g3, t3[2], naa.repeat_interleave(D, 0)),
                                                          rep(cn, P * k * D), rep(rn, P * k * D), nmask.repeat_interleave(D, 0), g3)
    grp = screen.chain_groups(one['fragment_type'][0])
    dq, sc, ca = [], [], []
    for i in range(P * k):
        sl = slice(i * D, (i + 1) * D)
        dq.append(hip.dockq_lite(rpos[sl], rmask[sl], npos[i], nmask[i], grp, check=False))
        sc.append(hip.commonness_score(t3[1][sl][:, gen]))
        ca.append(t3[1][sl][:, gen].contiguous())
    out.update(dockq=torch.stack(dq).view(P, k, D, 4), redock_score=torch.stack(sc).view(P, k, D), prmsd=t3[3].to(DEV).view(P, k, D))
    return out, ca


@pytest.mark.gpu
def test_zero_cutoff_screen_is_the_unclustered_screen_bit_for_bit(screen_models):
    """cluster_cutoff = 0.0 makes every pose its own cluster, in pose order: every field the unclustered screen returns is torch.equal, cluster_centre is
    arange(P), and the unclustered result has none of the new keys."""
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    kw = dict(screen_workers.SCREEN)
    P = kw['num_poses']
    plain = screen.optimize_antibody(dock, design, one, poses_per_launch=2, **kw)
    zero = screen.optimize_antibody(dock, design, one, poses_per_launch=2, cluster_cutoff=0.0, **kw)
    new = {'cluster_label', 'cluster_centre', 'cluster_size'}
    assert set(zero) == set(plain) | new and not (set(plain) & (new | {'redock_cluster_frac', 'redock_clusters'}))
    for name, v in plain.items():
        assert torch.equal(zero[name], v), name
    ar = torch.arange(P, device=DEV)
    assert torch.equal(zero['cluster_centre'], ar) and torch.equal(zero['cluster_label'], ar) and zero['cluster_size'].tolist() == [1] * P


@pytest.mark.gpu
def test_clustered_screen_equals_the_composition_of_public_calls(screen_models):
    """optimize_antibody(cluster_cutoff, max_clusters, redock_cutoff) against stage 1 -> sampler.cluster_poses -> the public calls on the centres, bit for
    bit.  The hash-filled dock model's poses are not known to fall into modes, so the cutoff is placed from the float64 RMSDs of the stage-1 poses
    themselves: halfway between the closest and the second closest pair, which merges exactly one pair (C = P - 1 uncapped); max_clusters = 3 then gives
    1 < C = 3 < P = 5 with one pose left over (label -1).  redock_cluster_frac / redock_clusters equal single-group calls per design."""
    from ab_opt_amd import hip, sampler
    P, S, k, D, contig, seed = 5, 3, 2, 3, '33-39', 5
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    pose_ca, pose_pos, pose_mask = _stage1(dock, one, P, seed)
    cutoff = _pair_gap_cutoff(pose_ca)
    cl = sampler.cluster_poses(pose_ca, cutoff, max_clusters=3)
    wl, wc, ws = greedy_f64(pose_ca.cpu().numpy(), cutoff, 3)
    assert cl['label'].tolist() == wl.tolist() and cl['centre'].tolist() == wc.tolist() and cl['size'].tolist() == ws.tolist()
    C = len(wc)
    assert C == 3 and ws.tolist() == [2, 1, 1] and (wl == -1).sum() == 1
    want, redock_ca = _stages23(dock, design, one, pose_pos[cl['centre']], pose_mask[cl['centre']], S, k, D, contig, seed)
    rc = 2.0
    res = screen.optimize_antibody(dock, design, one, P, S, D, contig=contig, screened_per_pose=k, seed=seed, poses_per_launch=P, screen_by='ppl',
                                   cluster_cutoff=cutoff, max_clusters=3, redock_cutoff=rc)
    assert torch.equal(res['pose_ca'], pose_ca) and torch.equal(res['pose_score'], hip.commonness_score(pose_ca))
    for name in ('label', 'centre', 'size'):
        assert torch.equal(res['cluster_' + name], cl[name]), name
    for name, v in want.items():
        assert res[name].shape == v.shape and v.shape[0] == C and torch.equal(res[name], v), name
    for name in ('aar', 'dockq_mean', 'dockq_std', 'prmsd_mean', 'prmsd_std', 'redock_cluster_frac', 'redock_clusters'):
        assert res[name].shape[0] == C, name
    frac, num = [], []
    for ca in redock_ca:
        one_group = hip.cluster_poses_grouped(ca, D, rc)
        frac.append(one_group['size'].max().float() / D)
        num.append(one_group['count'][0].long())
    assert torch.equal(res['redock_cluster_frac'], torch.stack(frac).view(C, k)) and torch.equal(res['redock_clusters'], torch.stack(num).view(C, k))
    assert ((res['redock_cluster_frac'] >= 1.0 / D) & (res['redock_cluster_frac'] <= 1.0)).all()
    assert screen.screen_filter(res).shape == (C, k)


@pytest.mark.gpu
def test_clustered_screen_does_not_depend_on_poses_per_launch_or_ranks(tmp_path, monkeypatch, screen_models):
    """The clustered screen (cutoff placed as in test_clustered_screen_equals_the_composition_of_public_calls: C = P - 1 = 4 clusters; re-docks clustered
    too) with all, 1 and 2 centres per launch, and on two gloo ranks sharing cuda:0 (4 centres split 2 + 2, the poses split 3 + 2 before the
    clustering), bit for bit -- ABOPT_PAIR_TERMS=0 / ABOPT_CORE_NO_SPLIT=1 pin one arithmetic form, as in tests/test_screen.py."""
    harness.pin_denoiser_form(monkeypatch)
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    P = screen_workers.SCREEN['num_poses']
    cutoff = _pair_gap_cutoff(_stage1(dock, one, P, screen_workers.SCREEN['seed'])[0])
    ref = harness.screen_is_launch_size_invariant(screen_models, dict(cluster_cutoff=cutoff, redock_cutoff=pose_cluster_workers.REDOCK_CUTOFF))
    assert ref['cluster_centre'].shape == (P - 1,) and ref['seqs'].shape[0] == P - 1 and ref['pose_ca'].shape[0] == P
    (tmp_path / 'cutoff.txt').write_text(repr(cutoff))
    harness.two_ranks_return(pose_cluster_workers.clustered_screen_worker, tmp_path, dict(clustered=ref))
