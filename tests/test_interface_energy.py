"""Interface energetics: abopt_interface_energy_grouped, its binding (hip.interface_energy_grouped, hip.check_interface_energy,
hip.default_residue_charge), sampler.interface_energy / sampler.energy_summary and the tables of ab_opt_amd.model.

The definition is restated in tests/interface_energy_statement.py.  `count` is integers and `energy` is fp32 formed in a stated order with every step rounded
once: the device has to EQUAL the float32 statement, count as integers and energy on its int32 view.  Random backbones hold almost no hydrogen bond and no salt
bridge, so the generator plants them, and the tests first assert on the statement that every term was counted and every reason for skipping one was met."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import interface_energy_statement as st
import scorer_harness as harness
import screen_workers
from ab_opt_amd import hip, model, sampler, screen
from scorer_harness import DEV, screen_models                      # noqa: F401 (screen_models: the fixture)

# (G, S, L, A, link given, custom tables, far from the origin, other knobs): every (G, S) of {(1, 1), (3, 2), (2, 5)}, L of {1, 2, 7, 63, 64, 65, 130, 300} (the
# tile of 64 owners / partners and its neighbours, several slices of a single candidate at 300), A of {4, 5, 15} (at 4 the centres fall back to CA)
CASES = [(1, 1, 1, 4, False, False, False, False), (3, 2, 1, 5, True, True, False, False), (3, 2, 2, 5, False, False, False, False),
         (2, 5, 2, 15, True, True, False, False), (2, 5, 7, 5, True, True, False, False), (1, 1, 7, 4, False, True, True, False),
         (1, 1, 63, 15, True, False, False, False), (3, 2, 63, 5, False, True, False, True), (3, 2, 64, 4, True, True, False, False),
         (1, 1, 64, 5, False, False, True, False), (2, 5, 65, 5, True, True, False, False), (1, 1, 65, 15, False, True, False, True),
         (1, 1, 130, 5, False, True, True, False), (2, 3, 130, 15, True, False, False, True), (3, 2, 130, 4, True, True, False, False),
         (1, 1, 300, 5, True, True, False, False), (1, 1, 300, 4, False, False, True, False), (3, 2, 300, 15, True, True, False, False)]
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------ the statements, computed once
@functools.lru_cache(maxsize=None)
def want(case, shared=False):
    """the float32 statement of a case -> (energy, count, tally); shared: the first candidate's mask and sequence serve its whole group"""
    c = st.case(*case)
    S = case[1]
    mask, seqs = (c['mask'][::S], c['seqs'][::S]) if shared else (c['mask'], c['seqs'])
    return st.grouped(c['pos'], mask, c['group'], seqs, c['link'], c['charge'], c['pair_table'], c['knobs'], S)[:3]


def assert_every_rule_is_reached():
    """over the whole table, on the float64 statements the generator kept: every term counted and every reason for skipping one met at least once"""
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
    t = {k: None if c[k] is None else torch.from_numpy(c[k]).to(DEV) for k in ('pos', 'mask', 'group', 'seqs', 'link', 'charge', 'pair_table')}
    if shared:
        t['mask'], t['seqs'] = t['mask'][::S].contiguous(), t['seqs'][::S].contiguous()
    return t, c['knobs']


def _bits(res):
    """energy as its int32 bit pattern: torch.equal on it is bit for bit"""
    return dict(energy=res['energy'].view(torch.int32), count=res['count'])


def _assert_equal(got, energy, count, tag):
    assert got['energy'].dtype == torch.float32 and got['count'].dtype == torch.int32
    g_n = got['count'].cpu().numpy().astype(np.int64)
    assert g_n.shape == count.shape and np.array_equal(g_n, count), (tag, np.argwhere(g_n != count)[:4])
    g_e = got['energy'].cpu().numpy()
    bad = np.argwhere(g_e.view(np.int32) != energy.view(np.int32))
    assert g_e.shape == energy.shape and not len(bad), (tag, bad[:4], g_e[tuple(bad[0])], energy[tuple(bad[0])])


# ------------------------------------------------------------------------------------------ CPU
def hand_built(o_dist=2.9, shift=0.0):
    """Four residues: 0 on no side, whose C and O point the hydrogen of residue 1 along +x; 1 on side 1, N at the origin; 2 on no side, far away; 3 on side 2,
    its O at o_dist from that N along +x, its C 1.23 A beyond, its N masked out (so it has no hydrogen of its own), all of it moved by `shift` along x.  The CB
    of 1 and 3 are 5.4 A apart.  Every type is A."""
    pos = np.zeros((4, 5, 3))
    pos[0] = [[-3, 6, 0], [-2, 5, 0], [-1.0, 5, 0], [-2.23, 5, 0], [-2, 4, 1]]
    pos[1] = [[0, 0, 0], [-0.5, 1.4, 0], [-2, 1.5, 0], [-2.5, 2.5, 0], [-0.5, 2, 1.2]]
    pos[2] = 100.0 + np.arange(15).reshape(5, 3)
    pos[3] = [[o_dist + 3.3, 1.2, 0], [o_dist + 2.0, 1.3, 0], [o_dist + 1.23, 0, 0], [o_dist, 0, 0], [4.9, 2, 1.2]]
    pos[3, :, 0] += shift
    mask = np.ones((4, 5), bool)
    mask[3, 0] = False
    return dict(pos=pos.astype(np.float32), mask=mask, group=np.array([0, 1, 0, 2]), seqs=np.zeros(4, np.uint8))


def test_statement_on_hand_built_pairs():
    """Each rule on a pair built by hand, in both arithmetics; the expected figures are computed from the formulas here."""
    aa = st.AA.index
    for dt, tol in ((np.float64, 1e-6), (np.float32, 1e-5)):
        run = lambda b, **kw: st.statement(b['pos'], b['mask'], b['group'], b['seqs'], dtype=dt, **kw)
        # an ideal bond: O 2.9 A from N along the H direction, C 1.23 A beyond it
        e_ideal = 27.888 * (1 / 2.9 + 1 / 3.13 - 1 / 1.9 - 1 / 4.13)
        assert -3.0 < e_ideal < -2.8
        r = run(hand_built())
        assert abs(r['energy'][1, 0] - e_ideal) < tol and abs(r['energy'][3, 0] - e_ideal) < tol
        assert r['count'].tolist() == [[0] * 5, [1, 0, 0, 0, 1], [0] * 5, [0, 1, 0, 0, 1]]
        assert not r['energy'][[0, 2]].any() and not r['energy'][:, 1:].any()
        # the clamp, both ways: a distance below 0.5 A (O 0.2 A from H), and an energy below -9.9 with every distance above 0.5 A (O 0.6 A from H)
        for o_dist, rule in ((1.2, 'hb/close'), (1.6, 'hb/floor')):
            r = run(hand_built(o_dist))
            assert r['tally'][rule] == 1 and r['energy'][1, 0] == dt(st.CLAMP) and r['energy'][3, 0] == dt(st.CLAMP) and r['count'][1, 0] == 1
        assert 27.888 * (1 / 1.6 + 1 / 1.83 - 1 / 0.6 - 1 / 2.83) < -9.9
        # a bond weaker than the cutoff is none; with a cutoff of 0 it is one
        e_weak = 27.888 * (1 / 6.0 + 1 / 6.23 - 1 / 5.0 - 1 / 7.23)
        assert -0.5 < e_weak < 0
        r = run(hand_built(6.0))
        assert not r['count'][:, :2].any() and not r['energy'][:, 0].any() and r['tally']['hb/weak'] == 1
        r = run(hand_built(6.0), knobs=dict(hb_cutoff=0.0))
        assert r['count'][1, 0] == 1 and abs(r['energy'][1, 0] - e_weak) < tol
        # proline has no H; there is no H across an unlinked step; none without the previous residue's O
        b = hand_built()
        r = run(dict(b, seqs=np.array([0, aa('P'), 0, 0], np.uint8)))
        assert not r['count'][:, :2].any() and r['tally']['hb/no_h_proline'] == 1
        r = run(b, link=np.array([0, 1, 1, 1]))
        assert not r['count'][:, :2].any() and r['tally']['hb/no_h_unlinked'] == 1
        m = b['mask'].copy()
        m[0, 3] = False
        r = run(dict(b, mask=m))
        assert not r['count'][:, :2].any() and r['tally']['hb/no_h_atom'] == 2              # (residue 3, whose N is masked out, is the other one)
        # the 9 A rule between the CA is part of the definition: the same bond with the acceptor's CA moved away is none
        far_ca = dict(b, pos=b['pos'].copy())
        far_ca['pos'][3, 1] = [9.0, 3.0, 0]
        assert not run(far_ca)['count'][:, :2].any() and run(far_ca)['tally']['hb/ca_far'] == 1
        # K - D: a salt bridge inside 7 A between the centres, none outside; the Coulomb term inside 15 A
        kd = np.array([0, aa('K'), 0, aa('D')], np.uint8)
        coulomb = lambda qq, d: 332.0637 * qq / (4.0 * max(d * d, 9.0))
        r = run(dict(hand_built(), seqs=kd))
        assert r['count'][:, 2:4].tolist() == [[0, 0], [1, 0], [0, 0], [1, 0]]
        assert abs(r['energy'][1, 1] - coulomb(-1, 5.4)) < tol and abs(r['energy'][3, 1] - coulomb(-1, 5.4)) < tol
        r = run(dict(hand_built(shift=3.0), seqs=kd))
        assert not r['count'][:, 2:4].any() and abs(r['energy'][1, 1] - coulomb(-1, 8.4)) < tol and r['tally']['elec/not_salt'] == 2
        r = run(dict(hand_built(shift=20.0), seqs=kd))
        assert not r['count'].any() and not r['energy'].any() and r['tally']['elec/beyond'] == 2
        # ... the distance floor d_min: two centres 1 A apart score as if 3 A apart
        close = dict(hand_built(), seqs=kd)
        close['pos'] = close['pos'].copy()
        close['pos'][3, 4] = close['pos'][1, 4] + np.float32([1.0, 0, 0])
        assert abs(run(close)['energy'][1, 1] - coulomb(-1, 3.0)) < tol
        # a like-charge pair
        r = run(dict(hand_built(), seqs=np.array([0, aa('K'), 0, aa('R')], np.uint8)))
        assert r['count'][:, 2:4].tolist() == [[0, 0], [0, 1], [0, 0], [0, 1]] and abs(r['energy'][1, 1] - coulomb(1, 5.4)) < tol
        # a NaN charge takes the type out
        q = st.default_charge()
        q[aa('D')] = np.nan
        r = run(dict(hand_built(), seqs=kd), charge=q)
        assert not r['count'][:, 2:4].any() and not r['energy'][:, 1].any()
        # an asymmetric pair table: the row is the owner's; a NaN entry adds nothing but the partner is counted; outside 8 A nothing
        t = np.zeros((21, 21), np.float32)
        t[aa('A'), aa('C')], t[aa('C'), aa('A')] = 1.5, -2.25
        ac = np.array([0, aa('A'), 0, aa('C')], np.uint8)
        r = run(dict(hand_built(), seqs=ac), pair_table=t)
        assert r['energy'][:, 2].tolist() == [0, 1.5, 0, -2.25] and r['count'][:, 4].tolist() == [0, 1, 0, 1]
        t[aa('A'), aa('C')] = np.nan
        r = run(dict(hand_built(), seqs=ac), pair_table=t)
        assert r['energy'][:, 2].tolist() == [0, 0, 0, -2.25] and r['count'][:, 4].tolist() == [0, 1, 0, 1]
        r = run(dict(hand_built(shift=3.0), seqs=ac), pair_table=t)
        assert not r['energy'][:, 2].any() and not r['count'][:, 4].any()
        # a byte >= 20 reads entry 20 of both tables
        t[aa('A'), 20], q20 = 3.0, st.default_charge()
        q20[20] = -1.0
        for byte in (20, 21, 255):
            r = run(dict(hand_built(), seqs=np.array([0, aa('A'), 0, byte], np.uint8)), pair_table=t)
            assert r['energy'][1, 2] == 3.0
            r = run(dict(hand_built(), seqs=np.array([0, aa('K'), 0, byte], np.uint8)), charge=q20)
            assert r['count'][1, 2] == 1 and r['count'][3, 2] == 1
        # bonded neighbours are skipped for every term: residues 1 and 3 made adjacent (2 dropped), linked and not
        adj = {k: np.delete(v, 2, 0) for k, v in dict(hand_built(), seqs=kd).items()}
        assert not run(adj)['count'].any() and run(adj)['tally']['pair/bonded'] == 2
        r = run(adj, link=np.array([1, 0, 0]))
        assert r['count'][1].tolist() == [1, 0, 1, 0, 1] and r['count'][2].tolist() == [0, 1, 1, 0, 1]
        # without CB (A = 4, or CB masked out) the centre is CA
        no_cb = dict(hand_built(), seqs=kd)
        r4 = run(dict(no_cb, pos=no_cb['pos'][:, :4], mask=no_cb['mask'][:, :4]))
        m = no_cb['mask'].copy()
        m[:, 4] = False
        d_ca = float(np.linalg.norm(no_cb['pos'][1, 1].astype(np.float64) - no_cb['pos'][3, 1].astype(np.float64)))
        for r in (r4, run(dict(no_cb, mask=m))):
            assert abs(r['energy'][1, 1] - coulomb(-1, d_ca)) < tol and r['tally']['centre/ca'] == 2


def test_planted_inputs_reach_every_rule():
    tally = assert_every_rule_is_reached()
    print(tally)
    assert sum(st.case(*case)['redraws'] for case in CASES) > 0, 'the table never exercised a re-draw'
    for case in CASES:                                                                  # no candidate was dropped, every one satisfies the condition
        c = st.case(*case)
        assert c['pos'].shape[0] == case[0] * case[1] == len(c['ref']) and all(st.condition(ref) == [] for ref in c['ref'])


def pair_bounds(ref, scale):
    """Bounds on |fp32 - float64| per PAIR term, from the roundings of the rule (u = 2^-24, M = `scale`, the largest |coordinate|):
    every difference of two coordinates, every product, sum, square root and quotient is rounded once, to relative u; a distance is so good to 4 u relative
    (a rounded difference per coordinate, relative to the distance after the squares are summed: 1 u; three squares and two sums: 2.5 u; halved by the root,
    plus its own u -- in all under 4 u), an inverse distance to 5 u.  The constructed H carries in addition an ABSOLUTE error: its unit vector is good to 6 u
    per coordinate (a difference, the length to 4 u, a quotient) and the sum N + that is rounded at the magnitude of the coordinate, u (M + 1) per coordinate;
    sqrt(3) times that, dH = sqrt(3) u (M + 7), moves r_CH and r_OH, so 1 / r by dH / r^2.  The sum of four inverse distances takes three more roundings of
    partial sums no larger than S = their sum of magnitudes, and the product with 27.888 one more:
      |dE_hb| <= 27.888 (9 u S + (1 / r_CH^2 + 1 / r_OH^2) dH)          (a pair with a distance below 0.5 A is exact; max(E, -9.9) only shrinks a difference),
      |dE_elec| <= 10 u |E|    (q q, its product with 332.0637, d2 to 5 u, its product with eps, the quotient)          and a table entry is exact.
    -> (hb (L, L), elec (L, L)), each x 1.01 for the second-order terms."""
    inv = ref['inv']
    dH = math.sqrt(3.0) * U * (scale + 7.0)
    S = inv['on'] + inv['ch'] + inv['oh'] + inv['cn']
    with np.errstate(invalid='ignore'):
        hb = np.where(ref['close'], 0.0, 27.888 * (9 * U * S + (inv['ch'] ** 2 + inv['oh'] ** 2) * dH)) * 1.01
    return hb, 10 * U * np.abs(ref['e_elec']) * 1.01


@pytest.mark.parametrize('case', [c for c in CASES if c[2] >= 63 and c[:2] == (1, 1)] + [(3, 2, 63, 5, False, True, False, True)])
def test_float32_statement_agrees_with_float64(case):
    """Under the condition on the inputs (no float64 bond energy within 1e-3 kcal/mol of hb_cutoff, no squared distance within 1e-4 relative of a squared cutoff or
    of 81, no bond distance within 1e-4 relative of 0.5 A -- asserted on the statement, the generator re-draws a candidate that violates it) the float32
    statement COUNTS what the float64 statement counts, takes the same terms, and every pair term is within the bound derived from the rule's roundings; a
    residue's sum is within the sum of its terms' bounds plus n u times the sum of their magnitudes (a recursive sum of n terms).  The largest difference and
    the largest bound are printed; DESIGN.md section 6.10 records them."""
    c = st.case(*case)
    S = case[1]
    worst = dict(hb=(0.0, 0.0), elec=(0.0, 0.0), res=(0.0, 0.0))
    for k, ref in enumerate(c['ref']):
        g = k // S
        assert st.condition(ref) == []
        a = st.statement(c['pos'][k], c['mask'][k], c['group'][g], c['seqs'][k], None if c['link'] is None else c['link'][g], c['charge'], c['pair_table'], c['knobs'],
                         np.float32)
        assert np.array_equal(a['count'], ref['count']), np.argwhere(a['count'] != ref['count'])[:4]
        for name in ('bond', 'elec', 'adds', 'gate', 'close'):
            assert np.array_equal(a[name], ref[name]), name
        scale = float(np.abs(c['pos'][k][np.isfinite(c['pos'][k])]).max())
        hb_bound, el_bound = pair_bounds(ref, scale)
        d_hb = np.abs(np.where(ref['gate'], a['e_don'].astype(np.float64) - ref['e_don'], 0.0))
        d_el = np.abs(a['e_elec'].astype(np.float64) - ref['e_elec'])
        assert (d_hb <= hb_bound)[ref['gate']].all(), (d_hb - hb_bound).max()
        assert (d_el <= el_bound).all(), (d_el - el_bound).max()
        assert np.array_equal(a['e_pair'].astype(np.float64), ref['e_pair'])
        bond = ref['bond']
        terms = np.stack([bond.sum(1) + bond.sum(0), ref['elec'].sum(1), ref['adds'].sum(1)], 1)
        mag = np.stack([np.where(bond, np.abs(ref['e_don']), 0).sum(1) + np.where(bond, np.abs(ref['e_don']), 0).sum(0), np.abs(ref['e_elec']).sum(1),
                        np.abs(ref['e_pair']).sum(1)], 1)
        own = np.stack([np.where(bond, hb_bound, 0).sum(1) + np.where(bond, hb_bound, 0).sum(0), el_bound.sum(1), np.zeros(len(bond))], 1)
        budget = own + terms * U * mag * 1.01
        d_res = np.abs(a['energy'].astype(np.float64) - ref['energy'])
        assert (d_res <= budget).all(), (d_res - budget).max()
        for name, d, b in (('hb', d_hb, hb_bound[ref['gate']]), ('elec', d_el, el_bound), ('res', d_res, budget)):
            worst[name] = (max(worst[name][0], float(d.max(initial=0.0))), max(worst[name][1], float(np.max(b, initial=0.0))))
    print(f'{case}: largest |fp32 - float64| (largest bound): per hydrogen bond {worst["hb"][0]:.2e} ({worst["hb"][1]:.2e}), per charge pair '
          f'{worst["elec"][0]:.2e} ({worst["elec"][1]:.2e}), per residue sum {worst["res"][0]:.2e} ({worst["res"][1]:.2e}) kcal/mol')


def test_bad_arguments_are_refused_before_any_launch():
    """check_interface_energy names the knob; every ValueError of the wrapper on CPU tensors (nothing has touched a device), the refusal of a CPU tensor once
    everything else is valid, and ABOPT_EINVAL of the C entry on dummy pointers that are never dereferenced."""
    assert hip.check_interface_energy() == dict(hb_cutoff=-0.5, elec_cutoff=15.0, salt_cutoff=7.0, pair_cutoff=8.0, eps=4.0, d_min=3.0) == st.KNOBS
    assert hip.check_interface_energy(hb_cutoff=0, pair_cutoff=0)['hb_cutoff'] == 0.0
    for name, bads in (('hb_cutoff', (0.1, float('nan'), float('-inf'))), ('elec_cutoff', (-1.0, float('nan'), float('inf'))), ('salt_cutoff', (-1.0, float('inf'))),
                       ('pair_cutoff', (-0.5, float('nan'))), ('eps', (0.0, -4.0, float('inf'))), ('d_min', (0.0, -1.0, float('nan')))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                hip.check_interface_energy(**{name: bad})
    pos, mask, group = torch.zeros(4, 6, 5, 3), torch.ones(4, 6, 5, dtype=torch.bool), torch.ones(2, 6, dtype=torch.int32)
    sq = torch.zeros(4, 6, dtype=torch.uint8)
    call = hip.interface_energy_grouped
    with pytest.raises(ValueError, match='whole groups'):
        call(pos[:3], mask[:3], group, sq[:3])
    with pytest.raises(ValueError, match='1 .. 15'):
        call(torch.zeros(4, 6, 16, 3), torch.ones(4, 6, 16, dtype=torch.bool), group, sq)
    with pytest.raises(ValueError, match='N, CA, C, O'):
        call(pos[:, :, :3], mask[:, :, :3], group, sq)
    with pytest.raises(ValueError, match='neither per candidate nor per group'):
        call(pos, mask[:3], group, sq)
    for bad in (sq[:3], sq[:, :5], sq.float(), sq[0]):
        with pytest.raises(ValueError, match='seqs'):
            call(pos, mask, group, bad)
    for bad in (torch.zeros(20), torch.zeros(21, 1), torch.zeros(21, dtype=torch.int32)):
        with pytest.raises(ValueError, match='charge'):
            call(pos, mask, group, sq, charge=bad)
    for bad in (torch.zeros(21), torch.zeros(20, 20), torch.zeros(21, 21, dtype=torch.int64)):
        with pytest.raises(ValueError, match='pair_table'):
            call(pos, mask, group, sq, pair_table=bad)
    for bad in (torch.ones(4, 6, dtype=torch.bool), torch.ones(2, 5, dtype=torch.bool)):
        with pytest.raises(ValueError, match=r'link .* must be \(G, L\)'):
            call(pos, mask, group, sq, link=bad)
    with pytest.raises(ValueError, match='hb_cutoff'):
        call(pos, mask, group, sq, hb_cutoff=1.0)
    with pytest.raises(ValueError, match='eps'):
        call(pos, mask, group, sq, eps=0.0)
    with pytest.raises(TypeError):
        call(pos, mask, group, sq, cutoff=1.0)
    with pytest.raises(RuntimeError, match='HIP device only'):                          # everything valid: the CPU tensor is refused before anything is allocated
        call(pos, mask, group, sq[:2], pair_table=model.hydrophobic_contact_table(), link=torch.ones(2, 6, dtype=torch.bool))
    batch = dict(fragment_type=torch.ones(2, 6, dtype=torch.long), generate_flag=torch.zeros(2, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match='groups'):
        sampler.interface_energy(batch, sq, pos, mask, groups='designed')

    L_ = hip.lib()
    dummy = (ctypes.c_char * 16)()
    a = ctypes.c_void_p(ctypes.addressof(dummy))
    knobs = dict(hb_cutoff=-0.5, elec_cutoff=15.0, salt_cutoff=7.0, pair_cutoff=8.0, eps=4.0, d_min=3.0)

    def entry(G=2, S=3, L=9, A=5, pos=a, charge=a, count=a, **kn):
        k = dict(knobs, **kn)
        return L_.abopt_interface_energy_grouped(pos, a, 0, a, a, 0, None, charge, None, G, S, L, A, k['hb_cutoff'], k['elec_cutoff'], k['salt_cutoff'],
                                                 k['pair_cutoff'], k['eps'], k['d_min'], a, count, None)
    for kw, word in ((dict(A=3), 'N, CA, C, O'), (dict(A=16), '16'), (dict(L=0), 'bad dims'), (dict(G=-1), 'bad dims'), (dict(S=-1), 'bad dims'),
                     (dict(hb_cutoff=0.5), 'hb_cutoff'), (dict(hb_cutoff=float('nan')), 'hb_cutoff'), (dict(elec_cutoff=-1.0), 'elec_cutoff'),
                     (dict(salt_cutoff=float('inf')), 'salt_cutoff'), (dict(pair_cutoff=float('nan')), 'pair_cutoff'), (dict(eps=0.0), 'eps'),
                     (dict(d_min=0.0), 'd_min'), (dict(d_min=-1.0), 'd_min'), (dict(G=65536, S=1), '65535'), (dict(pos=None), 'NULL'), (dict(charge=None), 'NULL'),
                     (dict(count=None), 'NULL')):
        assert entry(**kw) == 1 and word in L_.abopt_last_error().decode(), (kw, L_.abopt_last_error().decode())
    assert entry(G=0) == 0 and entry(S=0) == 0 and entry(G=0, pos=None) == 0            # no-ops, between the value checks and the pointer checks
    assert entry(G=0, eps=0.0) == 1


def test_binding_and_header_agree_on_the_new_entry():
    """The export list still equals the header (tests/test_abi.py checks every signature; this names the new one), ABI 59."""
    from test_abi import parse_header, signature_mismatches
    protos = parse_header()[0]
    assert 'abopt_interface_energy_grouped' in protos and set(hip.EXPORTS) == set(protos) and signature_mismatches(hip._SIGNATURES, protos) == {}
    assert hip.ABI_VERSION == 59 and hip.lib().abopt_abi_version() == 59
    assert len(protos['abopt_interface_energy_grouped'][1]) == 22


def test_tables():
    q = hip.default_residue_charge()
    assert q.dtype == torch.float32 and q.shape == (21,) and not q.is_cuda and hip.default_residue_charge() is q
    assert np.array_equal(q.numpy(), st.default_charge()) and tuple(q.tolist()) == model.RESIDUE_CHARGE
    by = dict(zip(model.AA_LETTERS, model.RESIDUE_CHARGE))
    assert {c for c, v in by.items() if v == 1.0} == set('KR') and {c for c, v in by.items() if v == -1.0} == set('DE') and sum(map(abs, by.values())) == 4
    t = model.hydrophobic_contact_table()
    assert t.dtype == torch.float32 and t.shape == (21, 21) and np.array_equal(t.numpy(), st.hydrophobic_table()) and torch.equal(t, t.T)
    assert int((t == -1).sum()) == 49 and int((t == 0).sum()) == 441 - 49 and t[model.AA_LETTERS.index('L'), model.AA_LETTERS.index('W')] == -1


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_device_equals_the_float32_statement(case):
    """count as integers and energy on its int32 view against the float32 statement: masks and sequences per candidate, and the first candidate's shared by its
    group; link NULL and given, the pair table NULL and given, a NaN charge entry, NaN / inf coordinates, masked-out N, CA, C, O and CB, the sides interleaved,
    coordinates 1000 A from the origin -- as the table of cases says."""
    assert_every_rule_is_reached()                                                      # on the statement, before any device call
    t, knobs = tensors(case)
    energy, count, _ = want(case)
    _assert_equal(hip.interface_energy_grouped(**t, **knobs), energy, count, case)
    if case[6]:
        assert float(t['pos'][torch.isfinite(t['pos'])].abs().max()) > 900
    if case[1] > 1:
        t, knobs = tensors(case, shared=True)
        energy, count, _ = want(case, shared=True)
        _assert_equal(hip.interface_energy_grouped(**t, **knobs), energy, count, (case, 'shared mask and sequences'))
    if case[2] >= 63:                                                                   # a condition on the inputs: the case holds something of every term
        assert (count[..., :4].sum((0, 1)) > 0).all() and (energy[..., 0] < 0).any() and (energy[..., 1] > 0).any() and (energy[..., 1] < 0).any()


@pytest.mark.gpu
def test_wide_sequences_and_empty_call():
    case = (2, 5, 65, 5, True, True, False, False)
    t, knobs = tensors(case)
    wide = t['seqs'].long()
    wide = torch.where(wide == 255, 100000, wide)                                       # any integer dtype, values outside 0 .. 255 saturate to "no type"
    energy, count, _ = want(case)
    _assert_equal(hip.interface_energy_grouped(**dict(t, seqs=wide), **knobs), energy, count, 'int64 sequences')
    _assert_equal(hip.interface_energy_grouped(**dict(t, mask=t['mask'].to(torch.uint8), group=t['group'].long(), link=t['link'].long()), **knobs), energy, count,
                  'other dtypes')
    empty = hip.interface_energy_grouped(t['pos'][:0], t['mask'][:0], t['group'][:0], t['seqs'][:0])
    assert empty['energy'].shape == (0, 65, 3) and empty['count'].shape == (0, 65, 5)
    # the placeholder table counts hydrophobic contacts with a minus sign
    hyd = hip.interface_energy_grouped(**dict(t, pair_table=model.hydrophobic_contact_table()), **knobs)
    c = st.case(*case)
    e, n, _, _ = st.grouped(c['pos'], c['mask'], c['group'], c['seqs'], c['link'], c['charge'], st.hydrophobic_table(), c['knobs'], case[1])
    _assert_equal(hyd, e, n, 'hydrophobic_contact_table')
    assert (e[..., 2] < 0).any() and (e[..., 2] == np.round(e[..., 2])).all()


@pytest.mark.gpu
def test_many_candidates():
    """1100 candidates of L = 65 (more workgroups than one row of the grid's slices) of ten distinct structures."""
    case, reps = (2, 5, 65, 5, True, True, False, False), 110
    G, S = case[:2]
    t, knobs = tensors(case)
    rep = lambda a: a.view(G, 1, S, *a.shape[1:]).expand(G, reps, S, *a.shape[1:]).reshape(G * reps * S, *a.shape[1:])
    got = hip.interface_energy_grouped(**dict(t, pos=rep(t['pos']), mask=rep(t['mask']), seqs=rep(t['seqs'])), **knobs)
    idx = (np.arange(G)[:, None, None] * S + np.arange(S)[None, None, :] + np.zeros((1, reps, 1), dtype=np.int64)).reshape(-1)
    energy, count, _ = want(case)
    _assert_equal(got, energy[idx], count[idx], 'many candidates')


def _call(knobs):
    return lambda **t: _bits(hip.interface_energy_grouped(**t, **knobs))


@pytest.mark.gpu
def test_grouped_call_equals_per_group_calls():
    for case in ((3, 2, 130, 4, True, True, False, False), (2, 5, 65, 5, True, True, False, False), (3, 2, 63, 5, False, True, False, True)):
        t, knobs = tensors(case)
        fixed = dict(charge=t.pop('charge'), pair_table=t.pop('pair_table'))               # the two tables belong to the call, not to a group
        harness.grouped_equals_per_group(lambda **kw: _call(knobs)(**kw, **fixed), [(case, case[0], case[1], t)], {'group', 'link'})


@pytest.mark.gpu
def test_call_is_capturable():
    """The call recorded with torch.cuda.graph (one launch, no memset node) and replayed on OTHER inputs copied into the static tensors gives what the eager call
    gives on them."""
    case = (2, 5, 65, 5, True, True, False, False)
    t, knobs = tensors(case)
    o = st.case(*case, seed=1)
    other = {k: torch.from_numpy(o[k]).to(DEV) for k in ('pos', 'mask', 'group', 'seqs', 'link')}
    first, held = harness.capture_replays_on_other_inputs(_call(knobs), t, other)
    energy, count, _ = want(case)
    _assert_equal(dict(energy=first['energy'].view(torch.float32), count=first['count']), energy, count, 'replay on the captured inputs')
    assert not torch.equal(held['count'], first['count']), 'the other inputs give other counts'
    e, n, _, _ = st.grouped(o['pos'], o['mask'], o['group'], o['seqs'], o['link'], o['charge'], o['pair_table'], o['knobs'], case[1])
    _assert_equal(dict(energy=held['energy'].view(torch.float32), count=held['count']), e, n, 'replay on the other inputs')


@pytest.mark.gpu
def test_repeat_calls_are_bit_identical():
    t, knobs = tensors((1, 1, 300, 5, True, True, False, False))
    first = _call(knobs)(**t)
    for _ in range(5):
        harness.assert_same_results(_call(knobs)(**t), first, 'repeat')


@pytest.mark.gpu
def test_energy_summary_counts_each_pair_once():
    """sampler.energy_summary against numpy on the statement: the integer counts summed over side 1 equal those summed over side 2 (each pair is seen from both
    ends) and the PAIRS of the statement; the float64 sums over side 1; freq per group."""
    case = (2, 5, 65, 5, True, True, False, False)
    G, S, L = case[:3]
    t, knobs = tensors(case)
    c = st.case(*case)
    out = hip.interface_energy_grouped(**t, **knobs)
    got = sampler.energy_summary(out, t['group'])
    energy, count, _ = want(case)
    side = np.repeat(c['group'], S, 0)
    s1, s2 = (side == 1)[..., None], (side == 2)[..., None]
    n1, n2 = np.where(s1, count, 0).sum(1), np.where(s2, count, 0).sum(1)
    assert np.array_equal(n1[:, 0], n2[:, 1]) and np.array_equal(n1[:, 1], n2[:, 0]) and np.array_equal(n1[:, 2:], n2[:, 2:])
    assert np.array_equal(n1[:, 0] + n1[:, 1], [int(r['bond'].sum()) for r in c['ref']])
    for name, col in (('salt_bridges', 2), ('like_pairs', 3), ('pair_contacts', 4)):
        assert got[name].dtype == torch.int32 and got[name].cpu().tolist() == n1[:, col].tolist(), name
    assert got['hbonds'].cpu().tolist() == (n1[:, 0] + n1[:, 1]).tolist() and got['hbonds'].sum() > 0 and got['salt_bridges'].sum() > 0
    e1 = np.where(s1, energy.astype(np.float64), 0.0).sum(1)
    for name, col in (('e_hb', 0), ('e_elec', 1), ('e_pair', 2)):
        assert got[name].dtype == torch.float32 and np.allclose(got[name].cpu().numpy(), e1[:, col], rtol=1e-6, atol=1e-6), name
    assert np.allclose(got['e_total'].cpu().numpy(), e1.sum(1), rtol=1e-6, atol=1e-6)
    held = (count[..., :3].sum(-1) > 0).reshape(G, S, L).sum(1)
    assert got['freq'].dtype == torch.int32 and np.array_equal(got['freq'].cpu().numpy(), held) and held.max() > 0
    assert got['energy_res'] is out['energy'] and got['count_res'] is out['count']


@pytest.mark.gpu
def test_screen_stages_scored_by_the_public_calls(screen_models):
    """The poses and re-docks of the screen's three stages (scorer_harness.stages) through sampler.interface_energy: the poses as one group of P, the re-docks
    as P k groups of D sharing their design's sequence -- the one grouped call equals the single-group calls design by design (so a result does not depend on
    how many candidates a launch holds) and the float32 statement on two of them; the summaries are what energy_summary makes of the raw call."""
    P, S, k, D, contig, seed = 4, 3, 2, 3, '33-39', 5
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    L = one['aa'].shape[1]
    pose_pos, pose_mask, rpos, rmask = harness.stages(dock, design, one, P, S, k, D, contig, seed)
    grp = screen.chain_groups(one['fragment_type'])
    link = sampler.backbone_links(one['chain_nb'], one['res_nb'])
    table = model.hydrophobic_contact_table()
    poses = sampler.interface_energy(one, one['aa'], pose_pos, pose_mask, pair_table=table)
    raw = hip.interface_energy_grouped(pose_pos, pose_mask, grp, one['aa'], pair_table=table, link=link)
    harness.assert_same_results({n: v for n, v in poses.items() if n.endswith('_res')}, dict(energy_res=raw['energy'], count_res=raw['count']), 'poses')
    harness.assert_same_results({n: v for n, v in poses.items() if not n.endswith('_res')},
                                {n: v for n, v in sampler.energy_summary(raw, grp).items() if not n.endswith('_res')}, 'summary')
    many = {name: one[name].expand(P * k, L) for name in ('fragment_type', 'chain_nb', 'res_nb', 'generate_flag')}
    seqs = one['aa'].expand(P * k, L)
    redocks = sampler.interface_energy(many, seqs, rpos, rmask, pair_table=table)
    assert redocks['energy_res'].shape == (P * k * D, L, 3) and redocks['freq'].shape == (P * k, L)
    for i in range(P * k):
        sl = slice(i * D, (i + 1) * D)
        alone = sampler.interface_energy(one, one['aa'], rpos[sl], rmask[sl], pair_table=table)
        for name, v in alone.items():
            whole = redocks[name][i:i + 1] if name == 'freq' else redocks[name][sl]
            assert torch.equal(whole.view(torch.int32) if whole.dtype == torch.float32 else whole, v.view(torch.int32) if v.dtype == torch.float32 else v), (i, name)
    for c in (0, P * k * D - 1):
        ref = st.statement(rpos[c].cpu().numpy(), rmask[c].cpu().numpy(), grp[0].cpu().numpy(), one['aa'][0].cpu().numpy(), link[0].cpu().numpy(), None,
                           st.hydrophobic_table())
        _assert_equal(dict(energy=redocks['energy_res'][c:c + 1], count=redocks['count_res'][c:c + 1]), ref['energy'][None], ref['count'][None], ('re-dock', c))
    assert (redocks['freq'][:, grp[0] == 0] == 0).all() and redocks['pair_contacts'].sum() > 0
