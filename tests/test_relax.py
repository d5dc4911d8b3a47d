"""Relax of docked candidates (include/abopt.h: abopt_relax_grouped): the float64 statement against finite differences and hand-worked
cases, the conditions the kernel cases have to meet (checked on the statement, before anything is sent to a device), and the kernel against the statement."""
import functools

import numpy as np
import pytest
import torch

import relax_statement as rs
import scorer_harness as harness
import screen_workers
from scorer_harness import DEV, dev

ULP = 2.0 ** -23                                                    # of 1.0 in fp32
NOISE = 1e-13                                                       # an energy below it is the rounding of a move by zero force
PLACEMENTS = {'origin': (0.0, 0.0, 0.0), 'far': rs.OFFSET}
CASE_IDS = ['G%dS%d-L%d-A%d-i%d' % c for c in rs.CASES]


def ulp32(x):
    """the spacing of fp32 at |x|"""
    return float(np.spacing(np.float32(abs(x))))


def knobs_of(c):
    return {n: c[n] for n in rs.KNOBS}


@functools.lru_cache(maxsize=None)
def reference(i, place):
    """(case i at a placement, its float64 statement): computed once, shared by the tests, never written to"""
    c = rs.case(*rs.CASES[i], offset=PLACEMENTS[place])
    return c, rs.statement(c['pos'], c['mask'], c['move'], c['link'], c['iters'], **knobs_of(c))


@functools.lru_cache(maxsize=None)
def yardstick(i, place):
    c = reference(i, place)[0]
    return rs.statement(c['pos'], c['mask'], c['move'], c['link'], c['iters'], dtype=np.float32, **knobs_of(c))


def one_candidate(atoms, move, link=None, **kn):
    """a hand-made candidate: atoms {(residue, slot): xyz}, every other slot masked out"""
    L = max(r for r, _ in atoms) + 1
    pos, mask = np.zeros((1, L, 3, 3)), np.zeros((1, L, 3), bool)
    for (r, p), x in atoms.items():
        pos[0, r, p], mask[0, r, p] = x, True
    base = dict(w_bond=0.0, w_ca=0.0, w_clash=0.0, w_tether=0.0, clash_d=3.0, step=0.1, max_shift=10.0, max_angle=10.0)
    return pos, mask, np.array([move], bool), None if link is None else np.array([link], bool), dict(base, **kn)


# ------------------------------------------------------------------------------------------ CPU: the statement
def test_forces_are_central_differences_of_the_energy():
    """-dE/dx of the float64 statement against (E(x - h) - E(x + h)) / 2h on a small case with every term switched on: every component within 1e-6 of the
    largest force component (relative to that one number, not component by component: a component near zero has no relative error to speak of).  clash_d is put
    into the widest gap of the pair distances near 3 A, so that no pair sits within h of the branch point of max(clash_d - d, 0)."""
    c = rs.case(1, 1, 7, 5, 0)
    pos, part = c['pos'][0], rs.taking_part(c['pos'], c['mask'])[0]
    moved = c['move'][0] & part.any(-1)
    y = np.where(part[..., None], pos, 0.0)
    flat = y[part]
    d = np.sqrt(((flat[:, None] - flat[None]) ** 2).sum(-1))
    near = np.sort(d[(d > 2.5) & (d < 3.5)])
    gap = int(np.argmax(np.diff(near)))
    kn = dict(knobs_of(c), clash_d=float(0.5 * (near[gap] + near[gap + 1])), w_tether=0.3)
    assert near[gap + 1] - near[gap] > 1e-2
    y0 = y + np.random.default_rng(3).normal(size=y.shape) * 0.1     # a tether that pulls
    E, f, pairs = rs.forces(y, y0, part, moved, c['link'][0], kn)
    assert pairs > 0 and E[0] > 0 and E[1] > 0 and E[3] > 0
    h, worst = 1e-5, 0.0
    for r, p in np.argwhere(part & moved[:, None]):
        for k in range(3):
            lo, hi = y.copy(), y.copy()
            lo[r, p, k] -= h
            hi[r, p, k] += h
            fd = (rs.forces(lo, y0, part, moved, c['link'][0], kn)[0].sum() - rs.forces(hi, y0, part, moved, c['link'][0], kn)[0].sum()) / (2 * h)
            worst = max(worst, abs(fd - f[r, p, k]))
    assert worst <= 1e-6 * np.abs(f).max(), (worst, np.abs(f).max())
    assert not f[~(part & moved[:, None])].any()                   # nothing acts on what does not move


def test_hand_case_two_atoms_under_the_clash_distance():
    """Two atoms 2 A apart under clash_d = 3 with w_clash = 0.7: E = 0.7 (3 - 2)^2, the moved one is pushed straight away with 2 * 0.7 * 1 and shifts by
    step * F; a second iteration starts from d = 2.14."""
    pos, mask, move, link, kn = one_candidate({(0, 1): (0.0, 0.0, 0.0), (1, 1): (0.0, 2.0, 0.0)}, [True, False], w_clash=0.7)
    st = rs.statement(pos, mask, move, link, 1, **kn)
    assert np.allclose(st['energy'][0, 0], [0, 0, 0.7, 0], atol=1e-15)
    assert np.allclose(st['f0'][0, 0, 1], [0, -1.4, 0], atol=1e-15)
    assert np.allclose(st['pos'][0, 0, 1], [0, -0.14, 0], atol=1e-15) and np.array_equal(st['pos'][0, 1], pos[0, 1])
    assert np.allclose(st['energy'][0, 1], [0, 0, 0.7 * 0.86 ** 2, 0], atol=1e-12)
    capped = rs.statement(pos, mask, move, link, 1, **dict(kn, max_shift=0.05))
    assert np.allclose(capped['pos'][0, 0, 1], [0, -0.05, 0], atol=1e-15)
    assert rs.statement(pos, mask, move, link, 1, **dict(kn, clash_d=2.0))['energy'].sum() == 0          # d = clash_d: no clash


def test_hand_case_one_stretched_bond():
    """C of residue 0 and N of residue 1 at 2.329 A, one ideal bond length too far, w_bond = 0.5: E = 0.5, the moved residue's C is pulled towards the N with
    2 * 0.5 * 1; without the link nothing acts.  The CA pair at 3.80 A adds nothing."""
    atoms = {(0, 1): (-1.0, 0.0, 0.0), (0, 2): (0.0, 0.0, 0.0), (1, 0): (2.329, 0.0, 0.0), (1, 1): (2.8, 0.0, 0.0)}
    pos, mask, move, link, kn = one_candidate(atoms, [True, False], link=[True, False], w_bond=0.5, w_ca=3.0)
    st = rs.statement(pos, mask, move, link, 1, **kn)
    assert np.allclose(st['energy'][0, 0], [0.5, 0, 0, 0], atol=1e-12)
    assert np.allclose(st['f0'][0, 0, 2], [1.0, 0, 0], atol=1e-12) and not st['f0'][0, 0, 1].any()
    # F = (1, 0, 0) on two atoms: D = 0.1 * 1 / 2; the force lies on the line through the centre: no torque
    assert np.allclose(st['pos'][0, 0, 1:], [[-0.95, 0, 0], [0.05, 0, 0]], atol=1e-12)
    assert rs.statement(pos, mask, move, None, 1, **kn)['energy'].sum() == 0


def test_hand_case_a_pure_torque():
    """N and C of the moved residue at (-1, 0, 0) and (1, 0, 0); a static atom 2 A below the N and one 2 A above the C, clash_d = 2.5, w_clash = 1: forces
    (0, 1, 0) and (0, -1, 0), F = 0, tau = (0, 0, -2), I = 2, w = step * tau / I = (0, 0, -0.1): the residue turns by 0.1 rad about z and does not shift."""
    atoms = {(0, 0): (-1.0, 0.0, 0.0), (0, 2): (1.0, 0.0, 0.0), (1, 1): (-1.0, -2.0, 0.0), (2, 1): (1.0, 2.0, 0.0)}
    pos, mask, move, link, kn = one_candidate(atoms, [True, False, False], w_clash=1.0, clash_d=2.5)
    st = rs.statement(pos, mask, move, link, 1, **kn)
    assert np.allclose(st['f0'][0, 0, [0, 2]], [[0, 1, 0], [0, -1, 0]], atol=1e-15)
    assert np.allclose(st['angle'][0, 0, 0], 0.1) and np.allclose(st['shift'][0, 0, 0], 0.0)
    t = -0.1
    assert np.allclose(st['pos'][0, 0, [0, 2]], [[-np.cos(t), -np.sin(t), 0], [np.cos(t), np.sin(t), 0]], atol=1e-12)
    capped = rs.statement(pos, mask, move, link, 1, **dict(kn, max_angle=0.03))
    assert np.allclose(capped['pos'][0, 0, 2], [np.cos(0.03), -np.sin(0.03), 0], atol=1e-12)


@pytest.mark.parametrize('i', range(len(rs.CASES)), ids=CASE_IDS)
def test_cases_exercise_what_they_claim(i):
    """On the float64 statement, at both placements: every multi-residue case has clashing pairs and a violated bond, with iterations a residue above and one
    below each cap; the total energy falls in every iteration; no candidate's clash count at clash_d rises from input to output.  At the origin: the map does not
    expand -- run from inputs perturbed by up to 1e-4 A per atom it ends within 2e-4 A of the unperturbed run."""
    G, S, L, A, iters = rs.CASES[i]
    for place in PLACEMENTS:
        c, st = reference(i, place)
        kn = knobs_of(c)
        assert np.isfinite(st['pos'][st['part']]).all() and np.isfinite(st['energy']).all()
        if L == 1:
            assert st['moved'].all() and st['energy'].sum() == 0 and np.array_equal(st['pos'][st['part']], c['pos'][st['part']])
            continue
        assert st['clash_pairs'][:, 0].sum() > 0 and (st['energy'][:, 0, 0] > kn['w_bond'] * 0.3 ** 2).any(), 'no clash or no bond off by 0.3 A'
        tot = st['total']
        assert ((np.diff(tot, axis=1) < 0) | (tot[:, :-1] <= 1e-12)).all() and (tot[:, -1] <= np.maximum(tot[:, 0], 1e-12)).all(), 'the energy rose'
        assert (st['clash_pairs'][:, 1] <= st['clash_pairs'][:, 0]).all(), st['clash_pairs'].T
        if iters:
            mv = np.broadcast_to(st['moved'][:, None, :], st['shift'].shape)
            for name, cap in (('shift', kn['max_shift']), ('angle', kn['max_angle'])):
                v = st[name][mv]
                assert (v > cap).any() and ((v > 0) & (v < cap)).any(), (name, 'no residue at the cap, or none below it')
            assert (tot[:, -1] < tot[:, 0]).any()
    if L >= 7:                                                                   # the irregular inputs the generator promises
        part = st['part']
        assert (~part.any(-1)).any() and (part.sum(-1)[st['moved']] == 1).any() and (c['mask'] & ~part).any() and (A == 3 or not c['mask'][:, :, 3:].all())
    c, st = reference(i, 'origin')
    rng = np.random.default_rng(7)
    bumped = c['pos'] + rng.uniform(-1.0, 1.0, size=c['pos'].shape) * (1e-4 / np.sqrt(3.0))
    st2 = rs.statement(bumped, c['mask'], c['move'], c['link'], c['iters'], **knobs_of(c))
    sel = st['part'] & st['moved'][..., None]
    assert np.sqrt((((st2['pos'] - st['pos'])[sel]) ** 2).sum(-1)).max() <= 2e-4


def intra_residue_drift(before, after, part):
    """(N, L): the largest change of a distance between two participating atoms of one residue"""
    def dist(x):
        x = np.where(part[..., None], x, 0.0)
        return np.sqrt(((x[:, :, :, None, :] - x[:, :, None, :, :]) ** 2).sum(-1))
    both = part[:, :, :, None] & part[:, :, None, :]
    return np.where(both, np.abs(dist(after) - dist(before)), 0.0).max((-1, -2))


@pytest.mark.parametrize('i', [k for k, c in enumerate(rs.CASES) if c[4] > 0], ids=[n for n, c in zip(CASE_IDS, rs.CASES) if c[4] > 0])
def test_statement_moves_residues_rigidly(i):
    """every intra-residue distance of the float64 output equals the input's to 1e-9 A, and something moved"""
    c, st = reference(i, 'origin')
    assert intra_residue_drift(c['pos'], st['pos'], st['part']).max() <= 1e-9
    if c['pos'].shape[1] > 1:
        assert np.abs((st['pos'] - c['pos'])[st['part'] & st['moved'][..., None]]).max() > 1e-3
    assert np.array_equal(st['pos'][~st['moved']], c['pos'][~st['moved']], equal_nan=True)


def test_check_relax_refuses_each_bad_knob():
    """hip.check_relax validates without a device; each refusal is a ValueError that names the argument"""
    from ab_opt_amd import hip
    good = hip.check_relax()
    assert good == dict(w_bond=1.0, w_ca=1.0, w_clash=1.0, w_tether=0.05, clash_cutoff=3.0, step=0.2, max_shift=0.5, max_angle=0.2, iters=50, max_moved=None)
    for name in ('w_bond', 'w_ca', 'w_clash', 'w_tether', 'clash_cutoff', 'step', 'max_shift', 'max_angle'):
        for bad in (-0.5, float('nan'), float('inf')):
            with pytest.raises(ValueError, match=rf'^{name} must be finite and >= 0 \(got {bad!r}\)$'):
                hip.check_relax(**{name: bad})
    for name in ('max_shift', 'max_angle'):
        with pytest.raises(ValueError, match=rf'^{name} must be > 0$'):
            hip.check_relax(**{name: 0.0})
    for bad in (-1, 1025, 2.5, True):
        with pytest.raises(ValueError, match=r'^iters must be an integer in 0 \.\. 1024 \(got'):
            hip.check_relax(iters=bad)
    for bad in (0, 257, 1.5):
        with pytest.raises(ValueError, match=r'^max_moved must be an integer in 1 \.\. 256 \(got'):
            hip.check_relax(max_moved=bad)
    assert hip.check_relax(w_clash=0, iters=0, max_moved=256)['max_moved'] == 256 and hip.RELAX_MAX_MOVED == rs.MAX_MOVED
    with pytest.raises(RuntimeError, match='HIP device only'):                   # a CPU tensor is refused before anything is allocated
        hip.relax_grouped(torch.zeros(1, 2, 3, 3), torch.ones(1, 2, 3, dtype=torch.bool), torch.ones(1, 2, dtype=torch.bool))


# ------------------------------------------------------------------------------------------ GPU: the kernel
def relax(c, **over):
    """hip.relax_grouped on a case's arrays -> (pos, energy) as float64 / float32 numpy"""
    from ab_opt_amd import hip
    pos, mask, move, link = dev(c, 'pos', 'mask', 'move', 'link')
    kn = knobs_of(c)
    kn['clash_cutoff'] = kn.pop('clash_d')
    res = hip.relax_grouped(pos.float(), mask, move, **dict(dict(link=link, iters=c['iters'], **kn), **over))
    return res['pos'].double().cpu().numpy(), res['energy'].cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def held_to_the_statement(tag, c, st, y32, got, energy):
    """the rule of test_kernel_against_the_float64_statement for one call: st / y32 the float64 / float32 statements of the case c, got / energy the device's"""
    sel = st['part'] & st['moved'][..., None]
    if c['iters'] == 0:
        sel = sel & False
    assert np.array_equal(bits(got)[~sel], bits(c['pos'])[~sel]), 'an atom that does not move lost its bits'
    finite = st['pos'][st['part']]
    err = np.abs(got - st['pos'])[sel].max() if sel.any() else 0.0
    e32 = np.abs(y32['pos'] - st['pos'])[sel].max() if sel.any() else 0.0
    bound = 4.0 * e32 + 2.0 * ulp32(np.abs(finite).max())
    print(f'relax {tag}: device {err:.3e}  e32 {e32:.3e}  ratio {err / e32 if e32 else 0.0:.2f}  bound {bound:.3e}')
    want = st['energy']
    real = want > NOISE
    rel = lambda e: (np.abs(e - want) / np.where(real, want, 1.0))[real].max() if real.any() else 0.0
    r32, rdev = rel(y32['energy']), rel(energy.astype(np.float64))
    print(f'relax {tag}: energy device {rdev:.3e}  e32 {r32:.3e}  ratio {rdev / r32 if r32 else 0.0:.2f}')
    assert err <= bound, (err, e32, bound)
    assert (energy[want == 0] == 0).all() and (np.abs(energy[~real]) <= NOISE).all()
    assert rdev <= max(4.0 * r32, 4.0 * ULP), (rdev, r32)


@pytest.mark.gpu
@pytest.mark.parametrize('place', list(PLACEMENTS))
@pytest.mark.parametrize('i', range(len(rs.CASES)), ids=CASE_IDS)
def test_kernel_against_the_float64_statement(i, place):
    """Atoms that do not move or take no part keep their bits.  Moved atoms: with e32 the float32 statement's largest coordinate error against float64 on this
    case, the device's error is <= 4 e32 + 2 ulp of the largest |coordinate|; every energy term: its error relative to its float64 value is <= 4 times the float32
    statement's largest such error on this case (one number per case, as e32 is), with a floor of 4 fp32 ulps; a term that float64 puts below 1e-13 A^2 is rounding
    noise of an update with zero force (0 or 1e-34 in float64, 1e-16 in fp32) and must stay below it.  The figures are printed before they are asserted."""
    c, st = reference(i, place)
    held_to_the_statement(f'{CASE_IDS[i]} {place}', c, st, yardstick(i, place), *relax(c))


@pytest.mark.gpu
def test_zero_iterations_copy_the_input():
    """iters = 0: the output equals the input bit for bit, NaN coordinates and masked-out atoms included, and both energy rows are the input's"""
    for i in (k for k, c in enumerate(rs.CASES) if c[4] == 0):
        c, st = reference(i, 'far')
        got, energy = relax(c)
        assert np.array_equal(bits(got), bits(c['pos']))
        assert np.array_equal(energy[:, 0], energy[:, 1]) and energy[:, 0, 2].max() > 0
    c, _ = reference(CASE_IDS.index('G2S5-L7-A15-i20'), 'origin')
    got, energy = relax(c, iters=0)
    assert np.array_equal(bits(got), bits(c['pos']))


@pytest.mark.gpu
def test_device_moves_residues_rigidly():
    """Every intra-residue distance drifts by <= (iters + 2) ulps of the residue's extent -- its largest intra-residue distance, 2.5 to 6 A -- plus, once and
    whatever iters is, 4 ulps of the residue's largest |coordinate|.  The second term is the grid the result is stored on, not a drift: the inputs lie on it, and
    an output coordinate is (c + v) + o, two roundings of at most half an ulp of that size each, so each coordinate of an atom is off by at most 1 ulp, the
    difference of two atoms by 2 ulps per coordinate, and its projection on the unit vector between them by 2 (|ux| + |uy| + |uz|) <= 2 sqrt(3) < 4 ulps.  At the
    far placement that floor is 2.4e-4 A and says little; at the origin it is 1e-5 A and the first term is what is tested."""
    for name in ('G2S5-L7-A15-i20', 'G1S1-L63-A5-i20', 'G1S1-L130-A15-i20', 'G3S2-L64-A3-i3', 'G3S2-L64-A15-i3'):
        for place in PLACEMENTS:
            c, st = reference(CASE_IDS.index(name), place)
            got, _ = relax(c)
            part = st['part']
            drift = intra_residue_drift(c['pos'], got, part)
            x = np.where(part[..., None], c['pos'], 0.0)
            both = part[:, :, :, None] & part[:, :, None, :]
            extent = np.where(both, np.sqrt(((x[:, :, :, None, :] - x[:, :, None, :, :]) ** 2).sum(-1)), 0.0).max((-1, -2))
            largest = np.abs(x).max((-1, -2))
            spacing = lambda v: np.spacing(np.maximum(v, 1e-30).astype(np.float32)).astype(np.float64)
            term, floor = (c['iters'] + 2) * spacing(extent), 4.0 * spacing(largest)
            over_floor = np.maximum(drift - floor, 0.0)
            print(f'relax rigidity {name} {place}: worst drift {drift.max():.3e} A; largest drift / (the two terms) {(drift / (term + floor))[st["moved"]].max():.3f}; '
                  f'largest (drift - floor) / ((iters + 2) ulps of the extent) {(over_floor / term)[st["moved"] & (extent > 0)].max():.3f}')
            assert (drift <= term + floor)[st['moved']].all() and drift[~st['moved']].max() == 0


@pytest.mark.gpu
def test_repeat_calls_are_bit_identical():
    for name in ('G2S5-L7-A15-i20', 'G3S2-L130-A5-i3'):
        c, _ = reference(CASE_IDS.index(name), 'far')
        a, b = relax(c), relax(c)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


@pytest.mark.gpu
def test_in_place_equals_out_of_place():
    """out = pos relaxes in place: the same bits as a call that writes to a tensor of its own, which leaves its input untouched"""
    from ab_opt_amd import hip
    for name in ('G2S5-L7-A15-i20', 'G3S2-L64-A3-i3', 'G2S5-L130-A3-i0'):
        c, _ = reference(CASE_IDS.index(name), 'origin')
        pos, mask, move, link = dev(c, 'pos', 'mask', 'move', 'link')
        pos = pos.float()
        kn = knobs_of(c)
        kn['clash_cutoff'] = kn.pop('clash_d')
        kept = pos.clone()
        apart = hip.relax_grouped(pos, mask, move, link=link, iters=c['iters'], **kn)
        assert np.array_equal(bits(pos.cpu().numpy()), bits(kept.cpu().numpy()))
        same = hip.relax_grouped(pos, mask, move, link=link, iters=c['iters'], out=pos, **kn)
        assert same['pos'] is pos
        assert np.array_equal(bits(pos.cpu().numpy()), bits(apart['pos'].cpu().numpy())) and torch.equal(same['energy'], apart['energy'])


def _inputs(c):
    t = dict(zip(('pos', 'mask', 'move', 'link'), dev(c, 'pos', 'mask', 'move', 'link')))
    t['pos'] = t['pos'].float().nan_to_num(nan=5.0)         # torch.equal of the harness: a NaN would never compare equal; the callers mask that atom out instead
    return t


def _call(c):
    from ab_opt_amd import hip
    kn = knobs_of(c)
    kn['clash_cutoff'] = kn.pop('clash_d')
    return lambda **t: hip.relax_grouped(**t, iters=c['iters'], **kn)


@pytest.mark.gpu
def test_nan_coordinate_is_as_good_as_masked_out():
    """a NaN coordinate takes an atom out exactly as a cleared mask byte does: the same bits on every atom that takes part, the same energies.  (The harness
    compares with torch.equal, so the tests that use it mask that atom out and make its coordinate finite.)"""
    c, _ = reference(CASE_IDS.index('G2S5-L7-A15-i20'), 'origin')
    masked = dict(c, mask=c['mask'] & np.isfinite(c['pos']).all(-1), pos=np.nan_to_num(c['pos'], nan=5.0))
    a, b = relax(c), relax(masked)
    sel = rs.taking_part(c['pos'], c['mask'])
    assert np.array_equal(bits(a[0])[sel], bits(b[0])[sel]) and np.array_equal(bits(a[1]), bits(b[1]))


@pytest.mark.gpu
def test_grouped_call_equals_per_group_calls():
    for name in ('G3S2-L7-A5-i3', 'G2S5-L65-A5-i1', 'G3S2-L130-A5-i3'):
        c, _ = reference(CASE_IDS.index(name), 'origin')
        G, S = rs.CASES[CASE_IDS.index(name)][:2]
        masked = dict(c, mask=c['mask'] & np.isfinite(c['pos']).all(-1))
        harness.grouped_equals_per_group(_call(c), [(name, G, S, _inputs(masked))], {'move', 'link'})


@pytest.mark.gpu
def test_shared_mask_equals_expanded_mask():
    """mask (G, L, A) shared by the S candidates of a group against the same mask repeated per candidate: the same bits; and the float64 statement"""
    from ab_opt_amd import hip
    for name in ('G3S2-L64-A3-i3', 'G2S5-L7-A15-i20'):
        i = CASE_IDS.index(name)
        G, S = rs.CASES[i][:2]
        c, _ = reference(i, 'origin')
        pos = np.nan_to_num(c['pos'], nan=5.0)                      # finite everywhere: which atoms take part is then the mask's word alone
        shared = dict(c, pos=pos, mask=c['mask'][::S])
        a, b = relax(shared), relax(dict(shared, mask=np.repeat(shared['mask'], S, 0)))
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
        st = rs.statement(pos, shared['mask'], c['move'], c['link'], c['iters'], **knobs_of(c))
        sel = st['part'] & st['moved'][..., None]
        assert np.abs(a[0] - st['pos'])[sel].max() < 1e-4 and np.allclose(a[1], st['energy'], rtol=1e-4, atol=1e-30)


@pytest.mark.gpu
def test_call_is_capturable():
    """one launch, nothing allocated by the library, no memset node: recorded with torch.cuda.graph and replayed on other inputs it gives what the eager call gives"""
    i = CASE_IDS.index('G2S5-L65-A5-i1')
    c, _ = reference(i, 'origin')
    other = rs.case(*rs.CASES[i], seed=4242)
    clean = lambda d: dict(d, mask=d['mask'] & np.isfinite(d['pos']).all(-1))
    first, held = harness.capture_replays_on_other_inputs(_call(c), _inputs(clean(c)), _inputs(clean(other)))
    assert not torch.equal(first['pos'], held['pos'])


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    """A NULL pointer, A = 2, a negative weight, iters = 1025 through the C entry point: ABOPT_EINVAL with a message; more moved residues than the cap:
    ABOPT_EUNSUPPORTED; the outputs keep the pattern they were filled with.  A candidate with more moved residues than the caller's max_moved comes back
    unchanged with NaN energies.  The Python wrapper raises ValueError for the same."""
    from ab_opt_amd import hip
    L_ = hip.lib()
    assert L_.abopt_relax_max_moved() == hip.RELAX_MAX_MOVED
    i = CASE_IDS.index('G2S5-L65-A5-i1')
    G, S, L, A, iters = rs.CASES[i]
    c, st = reference(i, 'origin')
    pos, mask, move, link = dev(c, 'pos', 'mask', 'move', 'link')
    pos = pos.float()
    out = torch.full_like(pos, 77.0)
    energy = torch.full((G * S, 2, 4), 77.0, device=DEV)
    kn = knobs_of(c)

    def call(pos_in=pos, G=G, S=S, L=L, A=A, max_moved=64, iters=iters, **over):
        k = dict(kn, **over)
        return L_.abopt_relax_grouped(hip.ptr(pos_in, optional=True), hip.ptr(out), hip.ptr(mask), 0, hip.ptr(move), hip.ptr(link), G, S, L, A, max_moved,
                                      *[k[n] for n in rs.KNOBS], iters, hip.ptr(energy), hip.stream())
    assert call(pos_in=None) == 1 and 'NULL' in L_.abopt_last_error().decode()
    assert call(A=2) == 1 and 'N, CA, C' in L_.abopt_last_error().decode()
    assert call(A=16) == 1 and call(L=0) == 1 and call(G=-1) == 1 and call(G=65536, S=1) == 1
    for name in rs.KNOBS:
        assert call(**{name: -1.0}) == 1 and name in L_.abopt_last_error().decode()
        assert call(**{name: float('nan')}) == 1
    assert call(max_shift=0.0) == 1 and call(max_angle=0.0) == 1
    assert call(iters=1025) == 1 and '1024' in L_.abopt_last_error().decode() and call(iters=-1) == 1
    assert call(max_moved=0) == 1
    assert call(L=300, max_moved=257) == 3 and '256' in L_.abopt_last_error().decode()                     # ABOPT_EUNSUPPORTED
    assert call(G=0) == 0 and call(S=0) == 0                                                              # no-ops
    torch.cuda.synchronize()
    assert (out == 77).all() and (energy == 77).all()
    assert call(max_moved=1000) == 0                                            # min(max_moved, L) = 65 <= 256
    torch.cuda.synchronize()
    sel = st['part'] & st['moved'][..., None]
    assert np.abs(out.double().cpu().numpy() - st['pos'])[sel].max() < 1e-4 and np.isfinite(energy.cpu().numpy()).all()
    few = int(st['moved'].sum(1).max()) - 1                                     # one fewer than the fullest candidate moves
    assert call(max_moved=few) == 0
    torch.cuda.synchronize()
    over = st['moved'].sum(1) > few
    e = energy.cpu().numpy()
    assert over.any() and np.isnan(e[over]).all() and np.isfinite(e[~over]).all()
    assert np.array_equal(bits(out.cpu().numpy())[over], bits(c['pos'])[over])
    with pytest.raises(ValueError, match='3 .. 15'):
        hip.relax_grouped(pos[:, :, :2], mask[:, :, :2], move)
    with pytest.raises(ValueError, match='w_clash'):
        hip.relax_grouped(pos, mask, move, w_clash=-1.0)
    with pytest.raises(ValueError, match='iters'):
        hip.relax_grouped(pos, mask, move, iters=1025)
    with pytest.raises(ValueError, match='link'):
        hip.relax_grouped(pos, mask, move, link=link[:, :64])
    with pytest.raises(ValueError, match='whole groups'):
        hip.relax_grouped(pos[:9], mask[:9], move)
    with pytest.raises(ValueError, match='out must be'):
        hip.relax_grouped(pos, mask, move, out=out[:5])


@pytest.mark.gpu
def test_rows_longer_than_one_tile_of_static_spheres():
    """L = 600: the static residues' bounding spheres are staged in tiles of 512, so the second tile is restaged in every iteration behind two more barriers.  The
    case of CASES (static and moved residues in both tiles) is held to the statement by test_kernel_against_the_float64_statement.  Here: with the moved
    residues confined to the first 512, the link between 511 and 512 cut and the last 88 residues carried 1000 A away, every pair of the second tile is pruned
    and adds exactly +0 -- the call equals, bit for bit, the single-tile call on the first 512 residues alone.  Brought back, those residues change the result."""
    i = CASE_IDS.index('G1S1-L600-A3-i3')
    c, _ = reference(i, 'origin')
    cut = dict(c, move=c['move'].copy(), link=c['link'].copy())
    cut['move'][:, 512:] = False
    cut['link'][:, 511] = False
    cut['move'][:, 500:512] = True                                          # moved residues next to the tile's edge, within reach of the other side
    away = dict(cut, pos=cut['pos'].copy())
    away['pos'][:, 512:] += 1000.0
    head = {k: (v[:, :512] if k in ('pos', 'mask', 'move', 'link') else v) for k, v in cut.items()}
    head['link'] = head['link'].copy()
    head['link'][:, 511] = False
    two, one, near = relax(away), relax(head), relax(cut)
    assert np.array_equal(bits(two[0][:, :512]), bits(one[0])) and np.array_equal(bits(two[1]), bits(one[1]))
    assert np.array_equal(bits(two[0][:, 512:]), bits(away['pos'][:, 512:]))
    assert not np.array_equal(bits(near[0][:, :512]), bits(one[0])) and near[1][0, 0, 2] > one[1][0, 0, 2]
    st = rs.statement(cut['pos'], cut['mask'], cut['move'], cut['link'], cut['iters'], **knobs_of(cut))
    y32 = rs.statement(cut['pos'], cut['mask'], cut['move'], cut['link'], cut['iters'], dtype=np.float32, **knobs_of(cut))
    held_to_the_statement('L600, moved residues at the edge of the tile', cut, st, y32, *near)


@pytest.mark.gpu
def test_largest_workgroup():
    """max_moved = 256 with A = 15 and L = 300: the largest LDS a call can ask for (157,728 bytes).  The bound only sizes the arrays: the same bits as with the
    bound at the number of moved residues, and the statement's result."""
    c = rs.case(1, 1, 300, 15, 1)
    n = int((c['move'][0] & rs.taking_part(c['pos'], c['mask'])[0].any(-1)).sum())
    big, small = relax(c, max_moved=256), relax(c, max_moved=n)
    assert 24 < n < 256 and np.array_equal(bits(big[0]), bits(small[0])) and np.array_equal(bits(big[1]), bits(small[1]))
    st = rs.statement(c['pos'], c['mask'], c['move'], c['link'], c['iters'], **knobs_of(c))
    y32 = rs.statement(c['pos'], c['mask'], c['move'], c['link'], c['iters'], dtype=np.float32, **knobs_of(c))
    held_to_the_statement('L300 A15 max_moved 256', c, st, y32, *big)


@pytest.mark.gpu
def test_many_candidates():
    """1100 candidates of L = 7, more than four workgroups per CU: candidate n of the big call equals the same candidate in a call of its group alone"""
    from ab_opt_amd import hip
    c = rs.case(2, 5, 7, 5, 3)
    reps = 110
    big = dict(c, pos=np.tile(c['pos'], (reps, 1, 1, 1)), mask=np.tile(c['mask'], (reps, 1, 1)), move=np.tile(c['move'], (reps, 1)), link=np.tile(c['link'], (reps, 1)))
    assert big['pos'].shape[0] == 1100
    a, b = relax(big), relax(c)
    assert np.array_equal(bits(a[0]), bits(np.tile(b[0], (reps, 1, 1, 1)))) and np.array_equal(bits(a[1]), bits(np.tile(b[1], (reps, 1, 1))))
    st = rs.statement(c['pos'], c['mask'], c['move'], c['link'], c['iters'], **knobs_of(c))
    sel = st['part'] & st['moved'][..., None]
    assert np.abs(b[0] - st['pos'])[sel].max() < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize('move', ['generated', 'antibody'])
def test_relax_candidates_lowers_what_the_scorer_counts(move):
    """sampler.relax_candidates on the screen's synthetic complex with four generated residues pushed 1.5 A towards the antigen: clashes_after <= clashes_before
    and breaks_after <= breaks_before with at least one strict, and all four counts are what the float64 statement's output gives."""
    from ab_opt_amd import sampler, screen
    one = screen_workers.complex_(DEV)
    pos, mask = one['pos_heavyatom'].float().clone(), one['mask_heavyatom'].bool()
    gen = one['generate_flag'][0].bool()
    ft = one['fragment_type'][0]
    rows = torch.nonzero(gen)[:, 0][2:6]
    ag = pos[0, ft == 3][:, 1].mean(0)
    push = ag - pos[0, rows, 1].mean(0)
    pos[0, rows] += 1.5 * push / push.norm()
    kn = dict(w_bond=1.0, w_ca=1.0, w_clash=1.0, w_tether=0.05, clash_cutoff=3.0, step=0.05, max_shift=0.1, max_angle=0.05, iters=40)
    res = sampler.relax_candidates(one, pos, mask, move=move, **kn)
    mv = gen[None] if move == 'generated' else screen.chain_groups(one['fragment_type']) == 1
    link = sampler.backbone_links(one['chain_nb'], one['res_nb'])
    sk = {('clash_d' if n == 'clash_cutoff' else n): float(np.float32(v)) for n, v in kn.items() if n != 'iters'}
    st = rs.statement(pos.double().cpu().numpy(), mask.cpu().numpy(), mv.cpu().numpy(), link.cpu().numpy(), kn['iters'], **sk)
    sel = st['part'] & st['moved'][..., None]
    assert np.abs(res['pos'].double().cpu().numpy() - st['pos'])[sel].max() < 1e-3
    counts = {}
    for tag, p in (('before', pos), ('after', torch.from_numpy(st['pos']).float().to(DEV))):
        g = sampler.interface_geometry(one, p.nan_to_num(), mask, groups='generated', clash_cutoff=3.0, bond_max=2.0)
        counts[tag] = (int(g['clash'][0]), int(g['breaks'][0]))
    got = {t: (int(res[f'clashes_{t}'][0]), int(res[f'breaks_{t}'][0])) for t in ('before', 'after')}
    print(f'relax_candidates move={move}: clashes, breaks {got["before"]} -> {got["after"]}; the statement predicts {counts["after"]}')
    assert got == counts
    assert got['after'][0] <= got['before'][0] and got['after'][1] <= got['before'][1] and got['after'] != got['before']
