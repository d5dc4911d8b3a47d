"""Backbone conformation: abopt_backbone_conformation_grouped, its binding (hip.backbone_conformation_grouped,
hip.check_backbone_conformation, hip.rama_regions), sampler.backbone_conformation / sampler.conformation_summary and the tables of ab_opt_amd.model.

The definition is restated in tests/backbone_statement.py.  have, rama, ss, state, partner and count are integers and torsion, bond are fp32 formed with every
step rounded once in a stated association: the device has to EQUAL the float32 statement, the integers as integers and the two fp32 outputs on their int32
view.  Random atoms hold no structure, so the inputs are planted (a NeRF builder, bridges placed atom by atom, degenerate cases written down), and the tests
first assert on the statement that every state, every pattern alternative, every reason for "undefined" and every count column was reached."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import backbone_statement as st
import scorer_harness as harness
import screen_workers
from ab_opt_amd import hip, model, sampler
from scorer_harness import DEV, screen_models                      # noqa: F401 (screen_models: the fixture)

# (G, S, L, A, link given, seqs given, eight regions, far from the origin, other hb_cutoff): every (G, S) of {(1, 1), (3, 2), (2, 5)}, L of {1, 2, 3, 6, 63, 64, 65,
# 130, 300} (the block of 64 donors / acceptors and its neighbours, more residues than the 256 threads of the workgroup) and the bound 512, A of {4, 5, 15}
CASES = [(1, 1, 1, 4, False, True, False, False, False), (3, 2, 1, 5, True, False, False, False, False), (3, 2, 2, 5, False, True, False, False, False),
         (2, 5, 2, 15, True, True, True, False, False), (2, 5, 3, 5, True, True, False, False, False), (1, 1, 3, 4, False, False, False, True, False),
         (3, 2, 6, 5, True, True, True, False, False), (1, 1, 6, 15, False, True, False, False, True), (1, 1, 63, 15, True, True, False, False, False),
         (3, 2, 63, 5, False, True, True, False, True), (3, 2, 64, 4, True, True, False, False, False), (1, 1, 64, 5, False, False, True, True, False),
         (2, 5, 65, 5, True, True, True, False, False), (1, 1, 65, 15, False, True, False, False, True), (1, 1, 130, 5, False, True, True, True, False),
         (2, 3, 130, 15, True, True, False, False, True), (3, 2, 130, 4, True, False, True, False, False), (1, 1, 300, 5, True, True, True, False, False),
         (1, 1, 300, 4, False, True, False, True, False), (3, 2, 300, 15, True, True, True, False, False), (1, 1, 512, 5, True, True, True, False, False),
         (3, 2, 512, 4, False, True, False, False, False)]
U = 2.0 ** -24
FLOATS = ('torsion', 'bond')


# ------------------------------------------------------------------------------------------ the statements, computed once
@functools.lru_cache(maxsize=None)
def want(case, shared=False, no_regions=False):
    """the float32 statement of a case -> (dict of stacked outputs, tally); shared: the first candidate's mask and sequence serve its whole group; no_regions:
    K = 0"""
    c = st.case(*case)
    S = case[1]
    mask, seqs = (c['mask'][::S], None if c['seqs'] is None else c['seqs'][::S]) if shared else (c['mask'], c['seqs'])
    return st.grouped(c['pos'], mask, c['rows'], seqs, c['link'], np.zeros((0, 8), np.float32) if no_regions else c['regions'], c['hb_cutoff'], S)[:2]


def assert_every_rule_is_reached():
    """over the whole table, on the float64 statements the generator kept: every rule of backbone_statement.RULES met at least once"""
    tally = dict.fromkeys(st.RULES, 0)
    for case in CASES:
        for ref in st.case(*case)['ref']:
            for rule, v in ref['tally'].items():
                tally[rule] += v
    for rule in st.RULES:
        assert tally[rule] > 0, (rule, 'never reached')
    return tally


def tensors(case, shared=False):
    c = st.case(*case)
    S = case[1]
    t = {k: None if c[k] is None else torch.from_numpy(c[k]).to(DEV) for k in ('pos', 'mask', 'rows', 'seqs', 'link', 'regions')}
    if shared:
        t['mask'] = t['mask'][::S].contiguous()
        t['seqs'] = None if t['seqs'] is None else t['seqs'][::S].contiguous()
    return t, c['hb_cutoff']


def _bits(res):
    """the fp32 outputs as their int32 bit pattern: torch.equal on them is bit for bit"""
    return {k: v.view(torch.int32) if v.dtype == torch.float32 else v for k, v in res.items()}


def _assert_equal(got, ref, tag):
    for name, dtype in (('torsion', torch.float32), ('bond', torch.float32), ('have', torch.uint8), ('rama', torch.uint8), ('ss', torch.uint8),
                        ('state', torch.uint8), ('partner', torch.int32), ('count', torch.int32)):
        assert got[name].dtype == dtype, (tag, name)
        g = got[name].cpu().numpy()
        if name in FLOATS:
            w = ref[name]
            assert g.shape == w.shape, (tag, name, g.shape, w.shape)
            bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
            assert not len(bad), (tag, name, bad[:4], g[tuple(bad[0])], w[tuple(bad[0])])
        else:
            w = ref[name]
            assert g.shape == w.shape and np.array_equal(g.astype(np.int64), w), (tag, name, np.argwhere(g.astype(np.int64) != w)[:4])


# ------------------------------------------------------------------------------------------ CPU
def _run(x, seqs=None, link=None, rows=None, mask=None, dt=np.float64, **kw):
    L, A = x.shape[:2]
    return st.statement(x.astype(np.float32), np.ones((L, A), bool) if mask is None else mask, np.ones(L, bool) if rows is None else rows, seqs, link, dtype=dt, **kw)


def _letters(state):
    return ''.join(st.SS_LETTERS[s] if s < 6 else '-' for s in state)


def _degrees(r, k):
    return np.degrees(np.arctan2(r['torsion'][:, 2 * k + 1].astype(np.float64), r['torsion'][:, 2 * k].astype(np.float64)))


def test_statement_on_hand_built_segments():
    """Each rule once, in both arithmetics; the expected figures are computed from the formulas here."""
    for dt, tol in ((np.float64, 1e-4), (np.float32, 2e-3)):
        # the torsions put into the builder are the ones read back (in degrees; the inputs are rounded to fp32: 6e-7 A on a lever of an Angstrom is 3e-5 degrees; the
        # fp32 arithmetic adds 42 u = 1.4e-4 degrees, torsion_bound below); the ideal peptide geometry too
        for phi, psi, om in ((-57.0, -47.0, 180.0), (-120.0, 130.0, 180.0), (60.0, 45.0, 0.0), (-100.0, 130.0, 140.0)):
            r = _run(st.nerf([phi] * 5, [psi] * 5, [om] * 5), dt=dt)
            wrap = lambda a, b: np.abs((a - b + 180.0) % 360.0 - 180.0)
            assert (wrap(_degrees(r, 0)[1:], phi) < tol).all() and (wrap(_degrees(r, 1)[:-1], psi) < tol).all() and (wrap(_degrees(r, 2)[:-1], om) < tol).all()
            assert r['have'].tolist() == [62, 63, 63, 63, 1] and not r['torsion'][0, :2].any() and not r['torsion'][4, 2:].any() and not r['bond'][4].any()
            assert np.allclose(r['bond'][:4, 0], st.BOND['c_n'], atol=1e-5)
            assert np.allclose(r['bond'][:4, 1], math.cos(math.radians(st.ANGLE['ca_c_n'])), atol=1e-5)
            assert np.allclose(r['bond'][:4, 2], math.cos(math.radians(st.ANGLE['c_n_ca'])), atol=1e-5)
        # an alpha helix: E(i, i + 4) = -2.21 and nothing else below the cutoff; H on residues 1 .. 10 and nothing else
        r = _run(st.nerf([-57.0] * 12, [-47.0] * 12), dt=dt)
        e = r['e']
        assert all(abs(e[i, i + 4] + 2.21) < 0.01 for i in range(8)) and all(abs(e[i, i + 3] - 0.15) < 0.01 for i in range(9))
        assert all(abs(e[i, i + 5] + 0.16) < 0.01 for i in range(7)) and int(r['hb'].sum()) == 8
        assert _letters(r['state']) == 'CHHHHHHHHHHC' and (r['ss'][1:11] == st.SS['h4'] | st.SS['turn']).all() and (r['rama'][1:11] == 0).all()
        assert (r['partner'] == -1).all()
        c = dict(zip(st.COUNTS, r['count']))
        assert (c['part'], c['phipsi'], c['region0'], c['outliers'], c['omega'], c['cis'], c['twisted'], c['H'], c['C'], c['hb_donor'], c['hb_acceptor']) == \
            (12, 10, 10, 0, 11, 0, 0, 10, 2, 8, 8)
        # ... with a stricter cutoff there is no bond; with Pro at 6 that donor has no H: the 4-turn at 2 is gone, and the helix holds all the
        # same -- residues 1 .. 4 by the turns at 0 and 1, 4 .. 7 by those at 3 and 4
        assert _letters(_run(st.nerf([-57.0] * 12, [-47.0] * 12), dt=dt, hb_cutoff=-2.5)['state']) == 'C' * 12
        seqs = np.zeros(12, np.uint8)
        seqs[6] = st.PRO
        r = _run(st.nerf([-57.0] * 12, [-47.0] * 12), seqs, dt=dt)
        assert int(r['hb'].sum()) == 7 and not r['hb'][2, 6] and _letters(r['state']) == 'CHHHHHHHHHHC' and r['tally']['hb/no_h_proline'] == 1
        assert r['tally']['turn/4'] == 7
        # ... an unlinked step 5 takes the turns that span it (at 2 .. 5), the torsions that need it, and the H of residue 6
        link = np.ones(12, bool)
        link[5] = False
        r = _run(st.nerf([-57.0] * 12, [-47.0] * 12), link=link, dt=dt)
        assert _letters(r['state']) == 'CHHHHCCHHHHC' and r['have'][5] == 1 and r['have'][6] == 62 and r['tally']['turn/unlinked'] == 3
        # ... a row that is not scored gets nothing, and is a partner all the same
        rows = np.ones(12, bool)
        rows[[0, 4]] = False
        r = _run(st.nerf([-57.0] * 12, [-47.0] * 12), rows=rows, dt=dt)
        assert _letters(r['state']) == '-HHH-HHHHHHC' and r['rama'][4] == 255 and r['have'][4] == 0 and not r['torsion'][4].any() and r['partner'][4].tolist() == [-1, -1]
        assert dict(zip(st.COUNTS, r['count']))['hb_acceptor'] == 6 and dict(zip(st.COUNTS, r['count']))['hb_donor'] == 7
        # a 3-10 helix is G; a strand is nothing
        r = _run(st.nerf([-49.0] * 10, [-26.0] * 10), dt=dt)
        assert all(abs(r['e'][i, i + 3] + 2.97) < 0.01 for i in range(7)) and _letters(r['state']) == 'CGGGGGGGGC'
        r = _run(st.nerf([-120.0] * 6, [130.0] * 6), dt=dt)
        apart = np.abs(np.arange(6)[:, None] - np.arange(6)[None, :])
        assert _letters(r['state']) == 'CCCCCC' and (r['rama'][1:5] == 1).all() and not r['hb'].any()
        # (residues three or more apart are beyond the 9 A rule; of the others the strongest is C=O of i with N-H of i + 2, -0.44: no bond)
        assert np.isnan(r['e'][apart >= 3]).all() and r['tally']['hb/ca_far'] == 9 and \
            abs(np.nanmin(r['e']) + 0.444) < 0.01
        # helix_5 (I) and a lone 3-turn (T)
        assert _letters(_run(st.MODULES['pi'][1](5, None)[0], dt=dt)['state']) == 'CIIIIIIIC'
        assert _letters(_run(st.MODULES['turn'][1](5, None)[0], dt=dt)['state']) == 'CTTCCC'
        # the four bridge alternatives, each planted alone between i = 2 and j = 7: the planted bonds have the ideal energy
        e_ideal = 27.888 * (1 / 2.9 + 1 / 3.13 - 1 / 1.9 - 1 / 4.13)
        # (seen from j, the first parallel alternative of i is the second and vice versa; each antiparallel alternative is its own mirror image)
        for form, col, bonds, seen in (('par_a', 0, ((1, 7), (7, 3)), dict(par_a=1, par_b=1)), ('par_b', 0, ((6, 2), (2, 8)), dict(par_a=1, par_b=1)),
                                       ('anti_a', 1, ((2, 7), (7, 2)), dict(anti_a=2)), ('anti_b', 1, ((1, 8), (6, 3)), dict(anti_b=2))):
            link = np.ones(10, bool)
            link[4] = False
            r = _run(st.two_strands(form), link=link, dt=dt)
            assert sorted(map(tuple, np.argwhere(r['hb']))) == sorted(bonds), form
            assert {f: r['tally'][f'bridge/{f}'] for f in ('par_a', 'par_b', 'anti_a', 'anti_b')} == dict(dict(par_a=0, par_b=0, anti_a=0, anti_b=0), **seen), form
            assert _letters(r['state']) == 'CCECCCCECC' and r['partner'][2, col] == 7 and r['partner'][7, col] == 2 and r['partner'][2, 1 - col] == -1
            assert r['ss'][2] == (st.SS['par'], st.SS['anti'])[col]
            assert np.allclose([r['e'][b] for b in bonds], e_ideal, atol=1e-3)
            # ... beside an unlinked step 2 there is no bridge: residue 3 has no H, which takes a bond of two of the alternatives; the other two keep their
            # bonds and are refused because the bridge needs the step
            link[2] = False
            r = _run(st.two_strands(form), link=link, dt=dt)
            gone = any(d == 3 for _, d in bonds)
            assert _letters(r['state']) == 'C' * 10 and (r['partner'] == -1).all() and int(r['hb'].sum()) == (1 if gone else 2)
            assert r['tally']['bridge/unlinked'] == (0 if gone else 2), form
        # both ways into the clamp: a distance below 0.5 A, and an energy below -9.9 with every distance above 0.5 A (27.888 (1/1.6 + 1/1.83 - 1/0.6 - 1/2.83))
        r = _run(st.MODULES['clamps'][1](5, None)[0], dt=dt)
        assert 27.888 * (1 / 1.6 + 1 / 1.83 - 1 / 0.6 - 1 / 2.83) < -9.9
        assert r['hb'][1, 7] and r['hb'][8, 3] and r['e'][1, 7] == dt(st.CLAMP) and r['e'][8, 3] == dt(st.CLAMP) and r['close'][1, 7] and not r['close'][8, 3]
        assert r['tally']['hb/close'] == 1 and r['tally']['hb/floor'] == 1
        # the Ramachandran classes of the default table and of none; a Gly outlier; cis before Pro and before a non-Pro; twisted
        x, types, _ = st.MODULES['misc'][1](5, None)
        seqs = np.zeros(15, np.uint8)
        for off, letter in types.items():
            seqs[off] = st.AA.index(letter)
        r = _run(x, seqs, dt=dt)
        c = dict(zip(st.COUNTS, r['count']))
        assert r['rama'].tolist() == [255, 2, 3, 3, 1, 1, 1, 1, 1, 3, 3, 3, 3, 3, 255]
        assert (c['outliers'], c['outliers_gly'], c['cis'], c['cis_nonpro'], c['twisted'], c['omega']) == (7, 1, 2, 1, 1, 14)
        assert abs(r['torsion'][7, 5] - math.sin(math.radians(140.0))) < 1e-5 and abs(r['torsion'][8, 5] - math.sin(math.radians(160.0))) < 1e-5
        assert _run(x, seqs, dt=dt, regions=st.regions_array(st.EIGHT_REGIONS))['rama'].tolist() == [255, 2, 3, 3, 1, 1, 1, 1, 1, 3, 4, 5, 6, 7, 255]
        r0 = _run(x, seqs, dt=dt, regions=np.zeros((0, 8), np.float32))
        assert r0['rama'].tolist() == [255] + [0] * 13 + [255] and dict(zip(st.COUNTS, r0['count']))['outliers'] == 13
        # exact cases: a planar trans peptide gives cos = -1 and sin = 0 exactly; collinear and coincident atoms leave the torsion undefined, never NaN
        r = _run(st.exact_segment(), dt=dt)
        assert r['torsion'][0, 4] == -1.0 and r['torsion'][0, 5] == 0.0 and r['have'].tolist() == [62, 63, 57, 63, 40, 1]
        assert r['bond'][2, 1] == -1.0 and r['bond'][4, 0] > 0 and r['bond'][4, 1] == 0.0 and r['tally']['bond/ang_zero'] == 1
        assert r['tally']['psi/rho0'] == 2 and r['tally']['omega/rho0'] == 2 and r['tally']['phi/rho0'] == 1
        assert all(np.isfinite(r[k]).all() for k in FLOATS)
        # atoms that take no part: masked out, NaN, inf -- the quantities that need them are undefined, the rest stands
        x = st.nerf([-57.0] * 12, [-47.0] * 12).astype(np.float32)
        mask = np.ones((12, 5), bool)
        mask[3, 1] = False
        x[5, 3, 1] = np.nan
        x[7, 0, 2] = np.inf
        mask[9, :4] = False
        r = _run(x, mask=mask, dt=dt)
        # 2 lacks omega and the angle at N of 3 (CA of 3); 3 keeps the length and the angle at N of 4; 6 and 8 keep phi alone (N of 7, all of 9); 7 lacks phi and psi
        assert r['have'][[2, 3, 4]].tolist() == [27, 40, 63] and r['have'][5] == 63 and r['have'][[6, 7, 8, 9, 10]].tolist() == [1, 60, 1, 0, 62]
        assert r['state'][9] == 255 and r['tally']['residue/absent'] == 1 and not r['hb'][5].any() and not r['hb'][:, 6].any()
        assert all(np.isfinite(r[k]).all() for k in FLOATS)
        # coordinates moved by 1000 A: the same integers
        far = _run(st.nerf([-57.0] * 12, [-47.0] * 12) + np.array(st.SHIFT), dt=dt)
        assert _letters(far['state']) == 'CHHHHHHHHHHC'


def test_planted_inputs_reach_every_rule():
    tally = assert_every_rule_is_reached()
    print(tally)
    print('redraws', sum(st.case(*case)['redraws'] for case in CASES))
    for case in CASES:                                                                  # no candidate was dropped, every one satisfies the condition
        c = st.case(*case)
        assert c['pos'].shape[0] == case[0] * case[1] == len(c['ref']) and all(st.condition(ref) == [] for ref in c['ref'])


def test_redraw_on_a_violated_condition():
    """a candidate whose float64 statement violates the condition is recognised: a bond energy AT the cutoff, a torsion ON a region's bound"""
    x = st.nerf([-57.0] * 12, [-47.0] * 12)
    r = _run(x)
    assert st.condition(r) == []
    assert 'hb' in st.condition(_run(x, hb_cutoff=float(np.float32(r['e'][0, 4])) + 5e-4))
    assert 'plane' in st.condition(_run(st.nerf([-60.0] * 5, [-47.0] * 5)))              # phi = -60 = 120 - 180: on the line of alpha-L's upper phi bound
    assert 'twisted' in st.condition(_run(st.nerf([-60.0] * 5, [-47.0] * 5, [150.0] * 5)))      # omega = 150: |sin| = 0.5, the threshold itself


def torsion_bound(flat):
    """Bound on |fp32 - float64| of cos and sin of a torsion, from the roundings of the rule (u = 2^-24; s = `flat`, the smaller sine of the two bond angles):
    a difference of two coordinates, a product, a sum, a root, a quotient are each rounded once, to relative u.  A component of n = b x b' carries 4 u |b| |b'|
    (two products of rounded differences, one difference), so |dn| <= 7 u |b| |b'| = (7 u / s) |n|.  x = n1 . n2 then carries |n1| |n2| (7 u / s + 7 u / s + 3 u)
    (the dot product's own three products and two sums: 3 u), and y = |b2| (b1 . n2) carries |b1| |b2| |n2| (7 u / s + 4 u + 4 u) = |n1| |n2| (7 u / s + 8 u) / s
    (|b2| is good to 3 u, the last product to u; |n1| = s1 |b1| |b2|).  Dividing by rho = |n1| |n2| and adding 3 u for rho's own roundings and the quotient:
      |d cos|, |d sin| <= u (7 / s^2 + 22 / s + 6),          x 1.01 for the second-order terms."""
    return U * (7.0 / flat ** 2 + 22.0 / flat + 6.0) * 1.01


LENGTH_BOUND = 4 * U * 1.01         # relative: section 6.10's bound of a distance
COSINE_BOUND = 13 * U * 1.01        # absolute: (u . w) carries 5 u |u| |w| (rounded differences, three products, two sums), |u| |w| 7 u relative, the quotient u


@pytest.mark.parametrize('case', [c for c in CASES if c[2] >= 63 and c[:2] == (1, 1)] + [(3, 2, 63, 5, False, True, True, False, True)])
def test_float32_statement_agrees_with_float64(case):
    """Under the condition on the inputs (asserted on the float64 statement; the generator re-draws a candidate that violates it) the float32 statement's
    integers -- have, rama, ss, state, partner, count, and the relation hb itself -- EQUAL the float64 statement's, and cos, sin, the bond length and the two
    bond cosines are within the bounds derived from the rule's roundings.  The largest difference and the largest bound are printed; DESIGN.md section 6.13
    records them."""
    c = st.case(*case)
    S = case[1]
    worst = dict(torsion=(0.0, 0.0), length=(0.0, 0.0), cosine=(0.0, 0.0))
    for k, ref in enumerate(c['ref']):
        g = k // S
        assert st.condition(ref) == []
        a = st.statement(c['pos'][k], c['mask'][k], c['rows'][g], None if c['seqs'] is None else c['seqs'][k], None if c['link'] is None else c['link'][g],
                         c['regions'], c['hb_cutoff'], np.float32)
        for name in st.INTEGERS + ('hb', 'gate', 'close'):
            assert np.array_equal(a[name], ref[name]), (name, np.argwhere(a[name] != ref[name])[:4])
        d_t = np.abs(a['torsion'].astype(np.float64) - ref['torsion']).reshape(-1, 3, 2).max(-1)
        b_t = np.where(np.isfinite(ref['flat']), torsion_bound(np.where(np.isfinite(ref['flat']), ref['flat'], 1.0)), 0.0)
        assert (d_t <= b_t).all(), (d_t - b_t).max()
        d_b = np.abs(a['bond'].astype(np.float64) - ref['bond'])
        assert (d_b[:, 0] <= LENGTH_BOUND * ref['bond'][:, 0]).all() and (d_b[:, 1:] <= COSINE_BOUND).all(), d_b.max(0)
        with np.errstate(invalid='ignore', divide='ignore'):
            rel_len = np.where(ref['bond'][:, 0] > 0, d_b[:, 0] / ref['bond'][:, 0], 0.0)
        for name, d, b in (('torsion', d_t.max(), b_t.max()), ('length', rel_len.max(), LENGTH_BOUND), ('cosine', d_b[:, 1:].max(), COSINE_BOUND)):
            worst[name] = (max(worst[name][0], float(d)), max(worst[name][1], float(b)))
    print(f'{case}: largest |fp32 - float64| (largest bound): cos / sin of a torsion {worst["torsion"][0]:.2e} ({worst["torsion"][1]:.2e}), bond length (relative) '
          f'{worst["length"][0]:.2e} ({worst["length"][1]:.2e}), bond cosine {worst["cosine"][0]:.2e} ({worst["cosine"][1]:.2e})')


def test_rama_regions_round_trip_and_refusals():
    r = hip.rama_regions()
    assert r.dtype == torch.float32 and r.shape == (3, 8) and not r.is_cuda and np.array_equal(r.numpy(), st.regions_array(st.RAMA_REGIONS))
    r8 = hip.rama_regions(st.EIGHT_REGIONS)
    assert r8.shape == (8, 8) and np.array_equal(r8.numpy(), st.regions_array(st.EIGHT_REGIONS))
    back = np.degrees(np.arctan2(r8.numpy()[:, 1::2].astype(np.float64), r8.numpy()[:, 0::2].astype(np.float64)))
    assert np.allclose((back - np.array(st.EIGHT_REGIONS) + 180.0) % 360.0 - 180.0, 0.0, atol=1e-5)
    assert hip.rama_regions([]).shape == (0, 8)
    assert np.array_equal(hip.rama_regions([(200.0, 300.0, -400.0, -300.0)]).numpy(), st.regions_array([(-160.0, -60.0, -40.0, 60.0)]))      # modulo 360
    for bad, word in (([(10.0, 10.0, 0.0, 90.0)], 'phi arc'), ([(0.0, 90.0, 30.0, 30.0)], 'psi arc'), ([(0.0, 180.0, 0.0, 90.0)], 'phi arc'),
                      ([(0.0, 90.0, 100.0, -70.0)], 'psi arc'), ([(0.0, 90.0, 90.0, 0.0)], 'psi arc'), ([(0.0, float('nan'), 0.0, 90.0)], 'non-finite'),
                      ([(0.0, 90.0, 0.0)], 'rows of'), ([(0.0, 90.0, 0.0, 90.0)] * 9, 'at most 8')):
        with pytest.raises(ValueError, match=word):
            hip.rama_regions(bad)


def test_bad_arguments_are_refused_before_any_launch():
    """check_backbone_conformation names the argument; every ValueError of the wrapper on CPU tensors (nothing has touched a device), the refusal of a CPU tensor
    once everything else is valid, and ABOPT_EINVAL / ABOPT_EUNSUPPORTED of the C entry on dummy pointers that are never dereferenced."""
    assert hip.check_backbone_conformation() == dict(K=0, hb_cutoff=-0.5)
    assert hip.check_backbone_conformation(512, 15, hip.rama_regions(), 0) == dict(K=3, hb_cutoff=0.0)
    for kw, word in ((dict(L=513), 'L=513'), (dict(L=0), 'L=0'), (dict(A=3), 'A=3'), (dict(A=16), 'A=16'), (dict(hb_cutoff=0.1), 'hb_cutoff'),
                     (dict(hb_cutoff=float('nan')), 'hb_cutoff'), (dict(hb_cutoff=float('-inf')), 'hb_cutoff'), (dict(regions=torch.zeros(9, 8)), 'regions'),
                     (dict(regions=torch.zeros(3, 4)), 'regions'), (dict(regions=torch.zeros(8)), 'regions'), (dict(regions=torch.zeros(3, 8, dtype=torch.int32)), 'regions')):
        with pytest.raises(ValueError, match=word):
            hip.check_backbone_conformation(**kw)
    assert hip.BACKBONE_MAX_ROWS == st.MAX_ROWS == hip.lib().abopt_backbone_max_rows() and hip.BACKBONE_COUNTS == st.COUNTS
    pos, mask, rows = torch.zeros(4, 6, 5, 3), torch.ones(4, 6, 5, dtype=torch.bool), torch.ones(2, 6, dtype=torch.bool)
    sq = torch.zeros(4, 6, dtype=torch.uint8)
    call = hip.backbone_conformation_grouped
    with pytest.raises(ValueError, match='whole groups'):
        call(pos[:3], mask[:3], rows)
    with pytest.raises(ValueError, match='1 .. 15'):
        call(torch.zeros(4, 6, 16, 3), torch.ones(4, 6, 16, dtype=torch.bool), rows)
    with pytest.raises(ValueError, match='N, CA, C, O'):
        call(pos[:, :, :3], mask[:, :, :3], rows)
    with pytest.raises(ValueError, match='neither per candidate nor per group'):
        call(pos, mask[:3], rows)
    with pytest.raises(ValueError, match='L=513'):
        call(torch.zeros(2, 513, 4, 3), torch.ones(2, 513, 4, dtype=torch.bool), torch.ones(2, 513, dtype=torch.bool))
    for bad in (sq[:3], sq[:, :5], sq.float(), sq[0]):
        with pytest.raises(ValueError, match='seqs'):
            call(pos, mask, rows, seqs=bad)
    for bad in (torch.ones(4, 6, dtype=torch.bool), torch.ones(2, 5, dtype=torch.bool)):
        with pytest.raises(ValueError, match=r'link .* must be \(G, L\)'):
            call(pos, mask, rows, link=bad)
    for bad in (torch.zeros(9, 8), torch.zeros(3, 4), torch.zeros(3, 8, dtype=torch.int64)):
        with pytest.raises(ValueError, match='regions'):
            call(pos, mask, rows, regions=bad)
    with pytest.raises(ValueError, match='hb_cutoff'):
        call(pos, mask, rows, hb_cutoff=1.0)
    with pytest.raises(TypeError):
        call(pos, mask, rows, cutoff=1.0)
    with pytest.raises(RuntimeError, match='HIP device only'):                          # everything valid: the CPU tensor is refused before anything is allocated
        call(pos, mask, rows, seqs=sq[:2], link=torch.ones(2, 6, dtype=torch.bool), regions=hip.rama_regions())
    batch = dict(fragment_type=torch.ones(2, 6, dtype=torch.long), generate_flag=torch.zeros(2, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match='rows'):
        sampler.backbone_conformation(batch, pos, mask, rows='designed')

    L_ = hip.lib()
    dummy = (ctypes.c_char * 16)()
    a = ctypes.c_void_p(ctypes.addressof(dummy))

    def entry(G=2, S=3, L=9, A=5, K=3, hb_cutoff=-0.5, pos=a, rows=a, regions=a, count=a):
        return L_.abopt_backbone_conformation_grouped(pos, a, 0, rows, None, 0, None, regions, K, G, S, L, A, hb_cutoff, a, a, a, a, a, a, a, count, None)
    for kw, word in ((dict(A=3), 'N, CA, C, O'), (dict(A=16), '16'), (dict(L=0), 'bad dims'), (dict(G=-1), 'bad dims'), (dict(S=-1), 'bad dims'),
                     (dict(hb_cutoff=0.5), 'hb_cutoff'), (dict(hb_cutoff=float('nan')), 'hb_cutoff'), (dict(K=-1), 'regions'), (dict(K=9), 'regions'),
                     (dict(G=65536, S=1), '65535'), (dict(pos=None), 'NULL'), (dict(rows=None), 'NULL'), (dict(regions=None), 'NULL'), (dict(count=None), 'NULL')):
        assert entry(**kw) == 1 and word in L_.abopt_last_error().decode(), (kw, L_.abopt_last_error().decode())
    assert entry(L=513) == 3 and '512' in L_.abopt_last_error().decode()                # ABOPT_EUNSUPPORTED, before any launch
    assert entry(L=513, G=0) == 3 and entry(L=513, K=9) == 1                            # ... after the value checks, before the no-op
    assert entry(G=0) == 0 and entry(S=0) == 0 and entry(G=0, pos=None) == 0            # no-ops, between the value checks and the pointer checks
    assert entry(G=0, hb_cutoff=0.5) == 1


def test_binding_and_header_agree_on_the_new_entry():
    """The export list still equals the header (tests/test_abi.py checks every signature; this names the new ones), ABI 59."""
    from test_abi import parse_header, signature_mismatches
    protos = parse_header()[0]
    assert {'abopt_backbone_conformation_grouped', 'abopt_backbone_max_rows'} <= set(protos) and set(hip.EXPORTS) == set(protos)
    assert signature_mismatches(hip._SIGNATURES, protos) == {}
    assert hip.ABI_VERSION == 59 and hip.lib().abopt_abi_version() == 59
    assert len(protos['abopt_backbone_conformation_grouped'][1]) == 23 and protos['abopt_backbone_max_rows'][1] == []


def test_tables():
    assert model.SS_LETTERS == st.SS_LETTERS == 'HEGITC' and model.RAMA_REGIONS == st.RAMA_REGIONS and len(model.RAMA_REGIONS) == 3
    assert model.AA_LETTERS.index('P') == st.PRO == 12 and model.AA_LETTERS.index('G') == st.GLY == 5
    reg = st.regions_array(model.RAMA_REGIONS)
    inside = lambda phi, psi: st.statement(*_one_residue(phi, psi), regions=reg, dtype=np.float64)['rama'][1]
    assert [inside(-57.0, -47.0), inside(-120.0, 130.0), inside(60.0, 45.0), inside(60.0, -150.0), inside(-100.0, 70.0)] == [0, 1, 2, 3, 3]


def _one_residue(phi, psi):
    x = st.nerf([phi] * 3, [psi] * 3).astype(np.float32)
    return x, np.ones((3, 5), bool), np.ones(3, bool)


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_device_equals_the_float32_statement(case):
    """The integers as integers and torsion, bond on their int32 view against the float32 statement: masks and sequences per candidate, and the first candidate's
    shared by its group; seqs, link NULL and given; three and eight regions, and none (K = 0); another hb_cutoff; coordinates 1000 A from the origin; L up to
    the bound of 512 -- as the table of cases says."""
    assert_every_rule_is_reached()                                                      # on the statement, before any device call
    t, cutoff = tensors(case)
    _assert_equal(hip.backbone_conformation_grouped(**t, hb_cutoff=cutoff), want(case)[0], case)
    if case[7]:
        assert float(t['pos'][torch.isfinite(t['pos'])].abs().max()) > 900
    if case[1] > 1:
        t, cutoff = tensors(case, shared=True)
        _assert_equal(hip.backbone_conformation_grouped(**t, hb_cutoff=cutoff), want(case, shared=True)[0], (case, 'shared mask and sequences'))
    if case[2] in (3, 65, 300):
        t, cutoff = tensors(case)
        none = dict(t, regions=torch.zeros(0, 8, device=DEV))
        _assert_equal(hip.backbone_conformation_grouped(**none, hb_cutoff=cutoff), want(case, no_regions=True)[0], (case, 'K = 0'))
    if not case[6] and case[8] is False:                                                # regions=None is the default table, hb_cutoff's default is -0.5
        t, _ = tensors(case)
        _assert_equal(hip.backbone_conformation_grouped(**dict(t, regions=None)), want(case)[0], (case, 'defaults'))


@pytest.mark.gpu
def test_one_past_the_bound_is_refused():
    L = hip.BACKBONE_MAX_ROWS + 1
    pos, mask, rows = torch.zeros(1, L, 4, 3, device=DEV), torch.ones(1, L, 4, dtype=torch.bool, device=DEV), torch.ones(1, L, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError, match='L=513'):
        hip.backbone_conformation_grouped(pos, mask, rows)
    a = lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.zeros(64, device=DEV)
    rc = hip.lib().abopt_backbone_conformation_grouped(a(pos), a(mask), 0, a(rows), None, 0, None, None, 0, 1, 1, L, 4, -0.5, *[a(out)] * 8, hip.stream())
    assert rc == 3 and '512' in hip.lib().abopt_last_error().decode()
    torch.cuda.synchronize()
    assert not out.any()


@pytest.mark.gpu
def test_wide_sequences_and_empty_call():
    case = (2, 5, 65, 5, True, True, True, False, False)
    t, cutoff = tensors(case)
    wide = t['seqs'].long()
    wide = torch.where(wide == 255, 100000, wide)                                       # any integer dtype, values outside 0 .. 255 saturate to "no type"
    ref = want(case)[0]
    _assert_equal(hip.backbone_conformation_grouped(**dict(t, seqs=wide), hb_cutoff=cutoff), ref, 'int64 sequences')
    other = dict(t, mask=t['mask'].to(torch.uint8), rows=t['rows'].long(), link=t['link'].long(), regions=t['regions'].double())
    _assert_equal(hip.backbone_conformation_grouped(**other, hb_cutoff=cutoff), ref, 'other dtypes')
    empty = hip.backbone_conformation_grouped(t['pos'][:0], t['mask'][:0], t['rows'][:0])
    assert empty['torsion'].shape == (0, 65, 6) and empty['count'].shape == (0, 24) and empty['partner'].shape == (0, 65, 2) and empty['state'].shape == (0, 65)


@pytest.mark.gpu
def test_many_candidates():
    """1100 candidates of L = 65 of ten distinct structures."""
    case, reps = (2, 5, 65, 5, True, True, True, False, False), 110
    G, S = case[:2]
    t, cutoff = tensors(case)
    rep = lambda a: a.view(G, 1, S, *a.shape[1:]).expand(G, reps, S, *a.shape[1:]).reshape(G * reps * S, *a.shape[1:])
    got = hip.backbone_conformation_grouped(**dict(t, pos=rep(t['pos']), mask=rep(t['mask']), seqs=rep(t['seqs'])), hb_cutoff=cutoff)
    idx = (np.arange(G)[:, None, None] * S + np.arange(S)[None, None, :] + np.zeros((1, reps, 1), dtype=np.int64)).reshape(-1)
    _assert_equal(got, {k: v[idx] for k, v in want(case)[0].items()}, 'many candidates')


def _call(cutoff):
    return lambda **t: _bits(hip.backbone_conformation_grouped(**t, hb_cutoff=cutoff))


@pytest.mark.gpu
def test_grouped_call_equals_per_group_calls():
    for case in ((3, 2, 130, 4, True, False, True, False, False), (2, 5, 65, 5, True, True, True, False, False), (3, 2, 63, 5, False, True, True, False, True)):
        t, cutoff = tensors(case)
        fixed = dict(regions=t.pop('regions'))                                          # the table belongs to the call, not to a group
        harness.grouped_equals_per_group(lambda **kw: _call(cutoff)(**kw, **fixed), [(case, case[0], case[1], t)], {'rows', 'link'})


@pytest.mark.gpu
def test_call_is_capturable():
    """The call recorded with torch.cuda.graph (one launch, no memset node) and replayed on OTHER inputs copied into the static tensors gives what the eager call
    gives on them."""
    case = (2, 5, 65, 5, True, True, True, False, False)
    t, cutoff = tensors(case)
    o = st.case(*case, seed=1)
    other = {k: torch.from_numpy(o[k]).to(DEV) for k in ('pos', 'mask', 'rows', 'seqs', 'link')}
    first, held = harness.capture_replays_on_other_inputs(_call(cutoff), t, other)
    view = lambda r: {k: v.view(torch.float32) if k in FLOATS else v for k, v in r.items()}
    _assert_equal(view(first), want(case)[0], 'replay on the captured inputs')
    assert not torch.equal(held['count'], first['count']), 'the other inputs give other counts'
    ref = st.grouped(o['pos'], o['mask'], o['rows'], o['seqs'], o['link'], o['regions'], o['hb_cutoff'], case[1])[0]
    _assert_equal(view(held), ref, 'replay on the other inputs')


@pytest.mark.gpu
def test_repeat_calls_are_bit_identical():
    t, cutoff = tensors((1, 1, 300, 5, True, True, True, False, False))
    first = _call(cutoff)(**t)
    for _ in range(5):
        harness.assert_same_results(_call(cutoff)(**t), first, 'repeat')


@pytest.mark.gpu
def test_summary_matches_counts():
    """sampler.conformation_summary against numpy on the statement: the shares, the counts and freq per group; the angles in degrees against arctan2."""
    case = (2, 5, 65, 5, True, True, True, False, False)
    G, S, L = case[:3]
    t, cutoff = tensors(case)
    out = hip.backbone_conformation_grouped(**t, hb_cutoff=cutoff)
    got = sampler.conformation_summary(out, groups=G)
    ref = want(case)[0]
    n = dict(zip(st.COUNTS, ref['count'].T))
    assert np.array_equal(n['part'], (ref['state'] != 255).sum(1)) and all(np.array_equal(n[c], (ref['state'] == k).sum(1)) for k, c in enumerate(st.SS_LETTERS))
    assert n['H'].sum() > 0 and n['E'].sum() > 0 and n['outliers'].sum() > 0 and n['cis'].sum() > 0
    for name, cols in (('helix', 'HGI'), ('strand', 'E'), ('coil', 'TC')):
        assert got[name].dtype == torch.float64 and np.allclose(got[name].cpu().numpy(), sum(n[c] for c in cols) / n['part'], rtol=1e-12), name
    assert np.allclose((got['helix'] + got['strand'] + got['coil']).cpu().numpy(), 1.0)
    for name, c in (('scored', 'part'), ('outliers', 'outliers'), ('cis', 'cis'), ('cis_nonpro', 'cis_nonpro'), ('twisted', 'twisted'), ('hbonds', 'hb_donor')):
        assert got[name].dtype == torch.int32 and got[name].cpu().tolist() == n[c].tolist(), name
    held = (ref['state'] <= 1).reshape(G, S, L).sum(1)
    assert got['freq'].dtype == torch.int32 and np.array_equal(got['freq'].cpu().numpy(), held) and held.max() > 0
    assert all(got[k] is out[k] for k in out)
    empty = sampler.conformation_summary({k: v[:0] for k, v in out.items()}, groups=0)
    assert empty['freq'].shape == (0, L) and empty['helix'].shape == (0,)


@pytest.mark.gpu
def test_screen_stages_scored_by_the_public_calls(screen_models):
    """The poses and re-docks of the screen's three stages (scorer_harness.stages) through sampler.backbone_conformation: the poses as one group of P, the
    re-docks as P k groups of D sharing their design's sequence -- the one grouped call equals the single-group calls design by design (so a result does not
    depend on how many candidates a launch holds) and the float32 statement on two of them; the angles are atan2 of the kernel's cos and sin."""
    P, S, k, D, contig, seed = 4, 3, 2, 3, '33-39', 5
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    L = one['aa'].shape[1]
    pose_pos, pose_mask, rpos, rmask = harness.stages(dock, design, one, P, S, k, D, contig, seed)
    link = sampler.backbone_links(one['chain_nb'], one['res_nb'])
    scored = one['generate_flag'].bool()
    poses = sampler.backbone_conformation(one, pose_pos, pose_mask, seqs=one['aa'])
    raw = hip.backbone_conformation_grouped(pose_pos, pose_mask, scored, seqs=one['aa'], link=link)
    harness.assert_same_results(_bits({n: poses[n] for n in raw}), _bits(raw), 'poses')
    assert poses['freq'].shape == (1, L) and poses['phi'].shape == (P, L) and int(poses['scored'].min()) > 0
    defined = (raw['have'] & 1) != 0
    assert torch.equal(torch.isnan(poses['phi']), ~defined)
    assert torch.allclose(poses['phi'][defined], torch.rad2deg(torch.atan2(raw['torsion'][..., 1], raw['torsion'][..., 0]))[defined])
    many = {name: one[name].expand(P * k, L) for name in ('fragment_type', 'chain_nb', 'res_nb', 'generate_flag')}
    seqs = one['aa'].expand(P * k, L)
    redocks = sampler.backbone_conformation(many, rpos, rmask, seqs=seqs)
    assert redocks['torsion'].shape == (P * k * D, L, 6) and redocks['freq'].shape == (P * k, L) and redocks['count'].shape == (P * k * D, 24)
    for i in range(P * k):
        sl = slice(i * D, (i + 1) * D)
        alone = sampler.backbone_conformation(one, rpos[sl], rmask[sl], seqs=one['aa'])
        for name, v in alone.items():
            whole = redocks[name][i:i + 1] if name == 'freq' else redocks[name][sl]
            bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64) if x.dtype == torch.float64 else x
            assert torch.equal(bits(whole), bits(v)), (i, name)
    for c in (0, P * k * D - 1):
        ref = st.statement(rpos[c].cpu().numpy(), rmask[c].cpu().numpy(), scored[0].cpu().numpy(), one['aa'][0].cpu().numpy(), link[0].cpu().numpy())
        _assert_equal({n: redocks[n][c:c + 1] for n in FLOATS + st.INTEGERS}, {n: ref[n][None] for n in FLOATS + st.INTEGERS}, ('re-dock', c))
    assert (redocks['state'][:, ~scored[0]] == 255).all() and int(redocks['count'][:, 0].min()) > 0
