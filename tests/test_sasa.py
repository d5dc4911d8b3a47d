"""Buried surface area: abopt_sasa_grouped / hip.sasa_grouped / hip.sphere_points / sampler.slot_radii / sampler.buried_surface.

The definition (include/abopt.h: abopt_sasa_grouped) is restated below for ONE candidate in numpy float32 (`sasa_f32`), every operation in the definition's order
and rounded once, and in float64 (`sasa_f64`).  The device results have to EQUAL sasa_f32: the point counts as integers, the areas bit for bit.  A test that hides
a dead kernel is the risk with such inputs -- almost every point of a protein-like blob is hidden -- so every case with two sides first asserts, on the float32
statement, that at least 3 % of all points are free-exposed and at least 2 % of the free-exposed points are hidden by the other side (`case`)."""
import functools

import numpy as np
import pytest
import torch

import scorer_harness as harness
import screen_workers
from ab_opt_amd import hip, sampler, screen
from scorer_harness import DEV, dev

PROBE = 1.4
RADII = (1.55, 1.70, 1.70, 1.52, 1.70)                    # N, CA, C, O, CB; every further slot 1.70
SHIFT = (900.0, -700.0, 500.0)
MIN_FREE, MIN_BURIED = 0.03, 0.02                         # the two caps on the inputs
# (G, S, L, A, n): every (G, S) of {(1, 1), (3, 2), (2, 5)}, L of {1, 2, 7, 63, 64, 65, 130}, A of {1, 5, 15} and n of {1, 63, 64, 65, 96, 128, 200}; the largest
# float32 statements (cost ~ G S (L A)^2 n) on a few corners only
CASES = [(1, 1, 1, 1, 1), (1, 1, 1, 5, 64), (3, 2, 2, 1, 63), (2, 5, 2, 5, 128), (1, 1, 7, 1, 65), (3, 2, 7, 5, 96), (2, 5, 7, 15, 200), (3, 2, 63, 5, 63),
         (1, 1, 63, 15, 64), (2, 5, 64, 1, 65), (1, 1, 64, 5, 200), (2, 5, 65, 5, 64), (3, 2, 65, 1, 1), (1, 1, 65, 15, 96), (1, 1, 65, 15, 200),
         (3, 2, 130, 1, 128), (1, 1, 130, 5, 128), (1, 1, 130, 15, 1)]
FAR_CASES = [(3, 2, 2, 1, 63), (3, 2, 7, 5, 96), (2, 5, 64, 1, 65), (1, 1, 63, 15, 64), (1, 1, 65, 5, 200), (1, 1, 130, 5, 128)]


# ------------------------------------------------------------------------------------------ the statement
def _sasa(dt, pos, mask, group, radius, dirs, probe, k, margins=False):
    """The definition for ONE candidate in the arithmetic `dt`: pos (L, A, 3), mask (L, A), group (L,), radius (L, A), dirs (n, 3), probe, k.
    -> dict(pts [4] int64, area [L, 2] dt, res / slot [M]: the participating atoms in (residue, slot) order, own / other [M, n] bool: the two verdicts of every
    point [, margin [M, n]: min over the occluders j of | |q - c_j| - R_j |])."""
    pos, radius, dirs = np.asarray(pos).astype(dt), np.asarray(radius).astype(dt), np.asarray(dirs).astype(dt)
    mask, group = np.asarray(mask).astype(bool), np.asarray(group)
    probe, k = dt(probe), dt(k)
    L, n = pos.shape[0], dirs.shape[0]
    with np.errstate(invalid='ignore'):
        part = mask & np.isin(group, (1, 2))[:, None] & np.isfinite(pos).all(-1) & (radius > 0) & (radius <= 16)         # a NaN radius fails both comparisons
    res, slot = np.nonzero(part)
    M = res.size
    c = pos[res, slot]                                                  # (M, 3)
    R = radius[res, slot] + probe                                       # step 1
    T = R * R                                                           # step 2
    side = group[res]
    own, other = np.zeros((M, n), dtype=bool), np.zeros((M, n), dtype=bool)
    margin = np.full((M, n), np.inf) if margins else None
    step = max(1, int(4e6 // max(1, n * M)))                            # target atoms at a time: ~16 MB per temporary
    for lo in range(0, M, step):
        hi = min(M, lo + step)
        q = c[lo:hi, None, :] + R[lo:hi, None, None] * dirs[None, :, :]                                                   # step 3: one multiply, one add
        dx, dy, dz = (q[:, :, None, e] - c[None, None, :, e] for e in range(3))                                           # step 4
        d2 = (dx * dx + dy * dy) + dz * dz                              # step 5
        hid = d2 < T[None, None, :]                                     # step 6
        notself = np.arange(M)[None, :] != np.arange(lo, hi)[:, None]   # j != i
        hid &= notself[:, None, :]
        same = side[None, :] == side[lo:hi, None]
        own[lo:hi] = (hid & same[:, None, :]).any(-1)
        other[lo:hi] = (hid & ~same[:, None, :]).any(-1)
        if margins:
            m = np.abs(np.sqrt(d2) - R[None, None, :])
            margin[lo:hi] = np.where(notself[:, None, :], m, np.inf).min(-1, initial=np.inf)
    free, cplx = (~own).sum(1), (~own & ~other).sum(1)
    pts = np.array([free[side == 1].sum(), free[side == 2].sum(), cplx[side == 1].sum(), cplx[side == 2].sum()], dtype=np.int64)
    area = np.zeros((L, 2), dtype=dt)
    kt = k * T                                                          # the inner product is rounded first
    tf, tc = free.astype(dt) * kt, cplx.astype(dt) * kt                 # then the product with the count
    for m in range(M):                                                  # then the sum: np.nonzero lists the atoms by residue, slots ascending
        area[res[m], 0] = area[res[m], 0] + tf[m]
        area[res[m], 1] = area[res[m], 1] + tc[m]
    out = dict(pts=pts, area=area, res=res, slot=slot, own=own, other=other)
    if margins:
        out['margin'] = margin
    return out


def sasa_f32(pos, mask, group, radius, dirs, probe, k, **kw):
    """The definition for ONE candidate in numpy float32, every operation in the definition's order."""
    return _sasa(np.float32, pos, mask, group, radius, dirs, probe, k, **kw)


def sasa_f64(pos, mask, group, radius, dirs, probe, k, **kw):
    """The same in float64 (on the same fp32 inputs)."""
    return _sasa(np.float64, pos, mask, group, radius, dirs, probe, k, **kw)


def dirs_of(n):
    return hip.sphere_points(n).numpy()


def k_of(n):
    return np.float32(4.0 * np.pi / n)


def statement(pos, mask, group, radius, S, n, probe=PROBE):
    """sasa_f32 over G groups of S candidates: pos (G*S, L, A, 3), mask (G*S, L, A) or (G, L, A), group (G, L), radius (G, L, A), (L, A) or (A,)
    -> (pts [G*S, 4] int64, area [G*S, L, 2] float32)."""
    N, (G, L), A = pos.shape[0], group.shape, pos.shape[2]
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float32), (G, L, A))
    pts, area = np.zeros((N, 4), dtype=np.int64), np.zeros((N, L, 2), dtype=np.float32)
    for c in range(N):
        g = c // S
        one = sasa_f32(pos[c], mask[c] if mask.shape[0] == N else mask[g], group[g], radius[g], dirs_of(n), probe, k_of(n))
        pts[c], area[c] = one['pts'], one['area']
    return pts, area


# ------------------------------------------------------------------------------------------ the inputs
def radii_of(A):
    return np.array([RADII[a] if a < len(RADII) else 1.70 for a in range(A)], dtype=np.float32)


def _raw(G, S, L, A, seed, sep=6.0):
    """Two CA random walks of 3.8 A steps per candidate, the second shifted `sep` A along x; the first max(1, L // 3) residues are side 1; atoms normal(0.9 A)
    around their CA (1.2 A at A = 15).  From L = 7 on (as tests/test_interface_geometry.py): one residue without atoms, two residues with group 0, slots from 4 on
    masked in with probability 0.7, and in odd groups two residues per walk change sides.  -> pos float64 (G*S, L, A, 3), mask (G*S, L, A), group (G, L) int32."""
    rng = np.random.default_rng(seed)
    N, n1 = G * S, max(1, L // 3)
    group = np.full((G, L), 2, dtype=np.int32)
    for g in range(G):
        group[g, :n1] = 1
        if g % 2 and L >= 7:
            group[g, rng.permutation(n1)[:2]] = 2
            group[g, n1 + rng.permutation(L - n1)[:2]] = 1
        if L >= 7:
            group[g, rng.permutation(L)[:2]] = 0
    pos = np.zeros((N, L, A, 3))
    mask = rng.random((N, L, A)) < 0.7
    mask[:, :, :4] = True
    for c in range(N):
        first = np.arange(L) < n1
        step = rng.normal(size=(L, 3))
        step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
        ca = np.zeros((L, 3))
        for sel, origin in ((first, np.zeros(3)), (~first, np.array([sep, 0.0, 0.0]))):
            ca[sel] = origin + np.cumsum(step[sel], 0)
        pos[c] = ca[:, None] + rng.normal(size=(L, A, 3)) * (1.2 if A == 15 else 0.9)
        if L >= 7:
            mask[c, rng.integers(L)] = False
    return pos, mask, group


def shares(pts):
    """(free-exposed share of all points, share of the free-exposed points that the other side hides) from the point counts, given the total separately."""
    free, cplx = pts[:, :2].sum(), pts[:, 2:].sum()
    return free, (free - cplx) / max(1, free)


def _points_total(mask, group, S, n):
    N = mask.shape[0]
    return sum(int((mask[c] & np.isin(group[c // S], (1, 2))[:, None]).sum()) for c in range(N)) * n


@functools.lru_cache(maxsize=None)
def case(G, S, L, A, n, far=False):
    """Inputs built once per shape and shared by the tests -> dict(pos fp32, mask, group, radius (A,), pts, area: the float32 statement).  far: the same structure
    rotated and moved by SHIFT.  The seed is the first whose inputs meet the two caps (two-sided cases: L >= 2)."""
    for seed in range(50):
        pos, mask, group = _raw(G, S, L, A, 1000 * seed + 31 * L + 7 * A + 3 * G + S)
        if far:
            rot = np.linalg.qr(np.random.default_rng(99).normal(size=(3, 3)))[0]
            pos = pos @ rot.T + np.array(SHIFT)
        pos = pos.astype(np.float32)
        pts, area = statement(pos, mask, group, radii_of(A), S, n)
        free, buried = shares(pts)
        total = _points_total(mask, group, S, n)
        if L < 2 or (free >= MIN_FREE * total and buried >= MIN_BURIED):
            break
    if L >= 2:                                                          # a condition on the inputs, not on the code
        assert free >= MIN_FREE * total and buried >= MIN_BURIED, (G, S, L, A, n, free / total, buried)
    return dict(pos=pos, mask=mask, group=group, radius=radii_of(A), pts=pts, area=area, free_share=free / max(1, total), buried_share=buried)


def _bits(res):
    """pts and area of a result, the areas as their int32 bit patterns: torch.equal on them is bit for bit"""
    return dict(pts=res['pts'], area=res['area'].view(torch.int32))


def _assert_equals_statement(got, pts, area, tag):
    assert got['pts'].dtype == torch.int32 and got['area'].dtype == torch.float32
    g_pts, g_area = got['pts'].cpu().numpy().astype(np.int64), got['area'].cpu()
    assert np.array_equal(g_pts, pts), (tag, g_pts[:4], pts[:4])
    want = torch.from_numpy(np.ascontiguousarray(area))
    bad = (g_area.view(torch.int32) != want.view(torch.int32)).nonzero()
    assert torch.equal(g_area.view(torch.int32), want.view(torch.int32)), (tag, bad[:4], g_area[tuple(bad[0])] if len(bad) else None)


def _run(c, n, probe=PROBE, **over):
    t = dict(zip(('pos', 'mask', 'group', 'radius'), dev(c, 'pos', 'mask', 'group', 'radius')))
    t.update(over)
    return hip.sasa_grouped(t['pos'], t['mask'], t['group'], t['radius'], probe=probe, points=n)


# ------------------------------------------------------------------------------------------ CPU
def test_statement_on_two_spheres():
    """Two equal atoms of opposite sides at centre distance d along e: a point of the first is hidden iff u.e > d / (2 R) (|q - c2|^2 = R^2 - 2 R d u.e + d^2 < R^2),
    a point of the second iff -u.e > d / (2 R); counted independently in float64 from sphere_points(n), with d chosen so that no direction lies within 1e-6 of the
    plane.  Both statements give that count.  A small atom wholly inside a large one has 0 exposed points; two atoms 50 A apart have all points exposed."""
    r, probe = 1.7, 1.4
    R = float(np.float32(np.float32(r) + np.float32(probe)))
    e = np.array([2.0, -1.0, 2.0]) / 3.0
    for n in (1, 64, 96, 200):
        u = dirs_of(n).astype(np.float64)
        ue = u @ e
        d = next(d for d in np.arange(2.0, 6.0, 0.137) if np.abs(np.abs(ue) - d / (2 * R)).min() > 1e-6)
        hid1, hid2 = int((ue > d / (2 * R)).sum()), int((-ue > d / (2 * R)).sum())
        assert n < 64 or (0 < hid1 < n and 0 < hid2 < n)
        pos = np.stack([np.zeros(3), d * e])[:, None, :].astype(np.float32)          # (2, 1, 3); d e is not exact in fp32, by far less than the 1e-6 margin
        for group, want in (([1, 2], [n, n, n - hid1, n - hid2]), ([1, 1], [2 * n - hid1 - hid2, 0, 2 * n - hid1 - hid2, 0])):
            for f in (sasa_f32, sasa_f64):
                got = f(pos, np.ones((2, 1), bool), np.array(group), np.full((2, 1), r, np.float32), dirs_of(n), probe, k_of(n))
                assert got['pts'].tolist() == want, (n, group, f.__name__)
        # the exposed area of a lone sphere is n k R^2 = 4 pi R^2 to fp32 rounding
        lone = sasa_f32(pos[:1], np.ones((1, 1), bool), np.array([1]), np.full((1, 1), r, np.float32), dirs_of(n), probe, k_of(n))
        assert lone['pts'].tolist() == [n, 0, n, 0] and abs(float(lone['area'][0, 0]) / (4 * np.pi * R * R) - 1) < 1e-6
        assert lone['area'][0, 0] == lone['area'][0, 1]
    n = 96
    inside = np.array([[[0.0, 0.0, 0.0]], [[0.3, 0.2, -0.1]]], dtype=np.float32)
    for f in (sasa_f32, sasa_f64):
        got = f(inside, np.ones((2, 1), bool), np.array([1, 2]), np.array([[6.0], [1.0]], np.float32), dirs_of(n), probe, k_of(n))
        assert got['pts'].tolist() == [n, n, n, 0]                                   # the small atom is exposed when free, wholly hidden in the complex
        assert got['area'][1, 0] > 0 and got['area'][1, 1] == 0
        apart = f(np.array([[[0.0, 0.0, 0.0]], [[50.0, 0.0, 0.0]]], np.float32), np.ones((2, 1), bool), np.array([1, 2]), np.full((2, 1), r, np.float32),
                  dirs_of(n), probe, k_of(n))
        assert apart['pts'].tolist() == [n, n, n, n]


@pytest.mark.parametrize('L,A,n', [(7, 5, 96), (33, 15, 65), (65, 5, 64)])
def test_float32_statement_agrees_with_float64(L, A, n):
    """On the generator's cases, at the origin and moved by 900 A, the two statements agree on every point whose float64 margin min_j | |q - c_j| - R_j | is at
    least 2^-18 (max |coordinate| + max R): 64 ulps of the largest magnitude entering q (derived in csrc/sasa.hip).  The number of points below the margin, and
    of disagreements among them, is printed."""
    for far in (False, True):
        pos, mask, group = _raw(1, 1, L, A, 5 + L)
        if far:
            pos = pos + np.array(SHIFT)
        pos = pos.astype(np.float32)
        rad = np.broadcast_to(radii_of(A), (L, A))
        a = sasa_f32(pos[0], mask[0], group[0], rad, dirs_of(n), PROBE, k_of(n))
        b = sasa_f64(pos[0], mask[0], group[0], rad, dirs_of(n), PROBE, k_of(n), margins=True)
        bound = 2.0 ** -18 * (np.abs(pos[0][mask[0]]).max() + rad.max() + PROBE)
        safe = b['margin'] >= bound
        differ = (a['own'] != b['own']) | (a['other'] != b['other'])
        print(f'L={L} A={A} n={n} far={far}: {differ.size} points, {(~safe).sum()} within {bound:.2e} A of a sphere, {differ.sum()} verdicts differ')
        assert not (differ & safe).any()
        assert np.array_equal(a['res'], b['res']) and safe.mean() > 0.9                 # the condition leaves nearly every point under test


def test_sphere_points_are_unit_and_deterministic():
    for n in (1, 2, 63, 64, 96, 128, 1024):
        p = hip.sphere_points(n)
        assert p.shape == (n, 3) and p.dtype == torch.float32 and not p.is_cuda
        assert (p.double().norm(dim=1) - 1).abs().max() < 2e-7
        assert hip.sphere_points(n) is p                                                # cached
        k = np.arange(n, dtype=np.float64)
        z = 1 - (2 * k + 1) / n
        rho, phi = np.sqrt(1 - z * z), k * np.pi * (3 - np.sqrt(5))
        want = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1)
        assert np.abs(p.numpy().astype(np.float64) - want).max() < 1e-7
        assert np.array_equal(p.numpy()[:, 2], z.astype(np.float32))                    # z is a single rounding of the float64 value
    assert abs(float(hip.sphere_points(128).mean(0).norm())) < 0.02                    # spread over the whole sphere
    for bad in (0, 1025, -3):
        with pytest.raises(ValueError, match='1 .. 1024'):
            hip.sphere_points(bad)


def test_slot_radii():
    r = sampler.slot_radii(15)
    assert r.dtype == torch.float32 and r.shape == (15,) and not r.is_cuda
    assert r[:5].tolist() == [np.float32(v) for v in (1.55, 1.70, 1.70, 1.52, 1.70)] and (r[5:] == 0).all()
    assert sampler.slot_radii(3).tolist() == [np.float32(v) for v in (1.55, 1.70, 1.70)]
    assert sampler.slot_radii(5, atoms=4).tolist() == [np.float32(v) for v in (1.55, 1.70, 1.70, 1.52)] + [0.0]
    assert sampler.slot_radii(1).shape == (1,)
    with pytest.raises(ValueError):
        sampler.slot_radii(0)
    with pytest.raises(ValueError):
        sampler.slot_radii(5, atoms=6)


def test_probe_is_validated_without_a_device():
    """hip.check_probe_radius, hip.sasa_grouped and sampler.buried_surface refuse a negative / non-finite probe, a bad point count and malformed
    shapes with ValueError before anything touches a device: the tensors here live on the CPU."""
    assert hip.check_probe_radius('x', 0) == 0.0 and hip.check_probe_radius('x', '1.4') == 1.4
    for bad in (-0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='probe'):
            hip.check_probe_radius('probe', bad)
    pos, mask, group = torch.zeros(4, 6, 5, 3), torch.ones(4, 6, 5, dtype=torch.bool), torch.ones(2, 6, dtype=torch.int32)
    rad = sampler.slot_radii(5)
    for bad in (-1.0, float('nan')):
        with pytest.raises(ValueError, match='probe'):
            hip.sasa_grouped(pos, mask, group, rad, probe=bad)
    for bad in (0, 1025):
        with pytest.raises(ValueError, match='1 .. 1024'):
            hip.sasa_grouped(pos, mask, group, rad, points=bad)
    with pytest.raises(ValueError, match='1 .. 15'):
        hip.sasa_grouped(torch.zeros(4, 6, 16, 3), torch.ones(4, 6, 16, dtype=torch.bool), group, torch.ones(16))
    with pytest.raises(ValueError, match='whole groups'):
        hip.sasa_grouped(pos[:3], mask[:3], group, rad)
    with pytest.raises(ValueError, match='radius'):
        hip.sasa_grouped(pos, mask, group, torch.ones(4))
    with pytest.raises(ValueError, match='neither per candidate nor per group'):
        hip.sasa_grouped(pos, mask[:3], group, rad)
    with pytest.raises(RuntimeError, match='HIP device only'):                          # everything valid: the CPU tensor is refused before anything is allocated
        hip.sasa_grouped(pos, mask, group, rad)
    batch = dict(fragment_type=torch.ones(2, 6, dtype=torch.long), generate_flag=torch.zeros(2, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match='groups'):
        sampler.buried_surface(batch, pos, mask, groups='sides')
    with pytest.raises(ValueError, match='probe'):
        sampler.buried_surface(batch, pos, mask, probe=-1.0)


# ------------------------------------------------------------------------------------------ GPU: the call
@pytest.mark.gpu
@pytest.mark.parametrize('G,S,L,A,n', CASES)
def test_counts_and_areas_equal_the_float32_statement(G, S, L, A, n):
    """pts as integers and area bit for bit against sasa_f32, over the group layouts, the tile boundaries of the occluder walk (L = 63, 64, 65, 130), both atom
    widths of the kernel (A <= 5, A > 5) and both point widths (n <= 128, n > 128) with partial last passes (n = 1, 63, 65, 96, 200)."""
    c = case(G, S, L, A, n)
    print(f'free-exposed share {c["free_share"]:.3f}, buried share of the free-exposed points {c["buried_share"]:.3f}')
    _assert_equals_statement(_run(c, n), c['pts'], c['area'], (G, S, L, A, n))
    assert c['pts'][:, :2].sum() > 0
    full = np.broadcast_to(c['radius'], (G, L, A))                                      # radius as (G, L, A) and as (L, A): the same call
    for rad in (full, full[0]):
        _assert_equals_statement(_run(c, n, radius=torch.from_numpy(rad.copy()).to(DEV)), c['pts'], c['area'], 'radius shape')


@pytest.mark.gpu
@pytest.mark.parametrize('G,S,L,A,n', FAR_CASES)
def test_far_from_the_origin(G, S, L, A, n):
    """The same inputs rotated and moved by (900, -700, 500) A: the statement is recomputed on the moved fp32 coordinates and must be met bit for bit (the absolute
    slack of the prune has to carry the coarser ulp of such coordinates)."""
    c = case(G, S, L, A, n, True)
    assert np.abs(c['pos']).max() > 600
    _assert_equals_statement(_run(c, n), c['pts'], c['area'], (G, S, L, A, n))


@pytest.mark.gpu
def test_pruning_never_changes_a_verdict():
    """Where the bounding spheres are extreme: a 12 A probe (every residue reaches every other), a 0 probe, radii of 0.1 and of 16 A side by side, and a residue
    whose atoms lie 40 A apart (its sphere swallows the structure)."""
    G, S, L, A, n = 1, 1, 65, 5, 64
    base = case(G, S, L, A, n)
    for probe in (12.0, 0.0):
        pts, area = statement(base['pos'], base['mask'], base['group'], base['radius'], S, n, probe=probe)
        _assert_equals_statement(_run(base, n, probe=probe), pts, area, f'probe {probe}')
    rad = np.broadcast_to(base['radius'], (G, L, A)).copy()
    rad[0, ::3] = 0.1
    rad[0, 1::7, 2] = 16.0
    c = dict(base, radius=rad)
    pts, area = statement(c['pos'], c['mask'], c['group'], rad, S, n)
    assert pts[:, 2:].sum() > 0
    _assert_equals_statement(_run(c, n), pts, area, 'radii 0.1 and 16')
    pos = base['pos'].copy()
    r = int(np.nonzero(base['group'][0] == 1)[0][2])
    pos[0, r, 0] += np.float32(20.0)
    pos[0, r, 1] -= np.float32(20.0)
    c = dict(base, pos=pos)
    pts, area = statement(pos, c['mask'], c['group'], c['radius'], S, n)
    _assert_equals_statement(_run(c, n), pts, area, 'a residue 40 A wide')


@pytest.mark.gpu
def test_many_candidates_run_one_slice_each():
    """1100 candidates (more than four per CU: every candidate is ONE workgroup) of ten distinct structures, and one candidate of 260 residues, which is split over
    the most slices (64: four or five participating residues each, some slices of the group-0 residues' neighbours shorter)."""
    G, S, L, A, n = 2, 5, 7, 5, 96
    c = case(G, S, L, A, n)
    reps = 110
    pos, mask = (torch.from_numpy(c[k]).to(DEV).view(G, 1, S, *c[k].shape[1:]).expand(G, reps, S, *c[k].shape[1:]).reshape(G * reps * S, *c[k].shape[1:])
                 for k in ('pos', 'mask'))
    got = hip.sasa_grouped(pos, mask, torch.from_numpy(c['group']).to(DEV), torch.from_numpy(c['radius']).to(DEV), probe=PROBE, points=n)
    idx = (np.arange(G)[:, None, None] * S + np.arange(S)[None, None, :] + np.zeros((1, reps, 1), dtype=np.int64)).reshape(-1)
    _assert_equals_statement(got, c['pts'][idx], c['area'][idx], 'many candidates')
    pos, mask, group = _raw(1, 1, 260, 2, 77)
    pos = pos.astype(np.float32)
    one = dict(pos=pos, mask=mask, group=group, radius=radii_of(2))
    pts, area = statement(pos, mask, group, one['radius'], 1, 64)
    assert pts[0, 0] > pts[0, 2] > 0
    _assert_equals_statement(_run(one, 64), pts, area, 'one candidate over 64 slices')


@pytest.mark.gpu
def test_degenerate_inputs():
    """A side with no atoms; every atom masked out; a NaN coordinate and a NaN / 0 / negative / 17 A radius (all take no part: count 0, no occlusion); one lone atom
    (all n points exposed both ways); G = 0 and S = 0."""
    G, S, L, A, n = 1, 1, 7, 5, 96
    base = case(G, S, L, A, n)

    def check(c, tag):
        pts, area = statement(c['pos'], c['mask'], c['group'], c['radius'], S, n)
        got = _run(c, n)
        _assert_equals_statement(got, pts, area, tag)
        return pts, area

    one_side = dict(base, group=np.where(base['group'] == 2, 0, base['group']).astype(np.int32))
    pts, _ = check(one_side, 'no side 2')
    assert pts[0, 1] == 0 and pts[0, 3] == 0 and pts[0, 0] == pts[0, 2] > 0
    empty_side = dict(base, mask=base['mask'] & (base['group'][0] == 1)[None, :, None])
    pts, area = check(empty_side, 'side 2 without atoms')
    assert pts[0, 0] == pts[0, 2] and (area[0, base['group'][0] == 2] == 0).all()
    pts, area = check(dict(base, mask=np.zeros_like(base['mask'])), 'every atom masked out')
    assert not pts.any() and not area.any()
    pos = base['pos'].copy()
    pos[0, 1, 1, 2] = np.nan
    pos[0, 4, 0, 0] = np.inf
    rad = np.broadcast_to(base['radius'], (G, L, A)).copy()
    rad[0, 0, 0], rad[0, 2, 1], rad[0, 3, 2], rad[0, 5, 3] = np.nan, 0.0, -1.0, 17.0
    pts, area = check(dict(base, pos=pos, radius=rad), 'NaN coordinate, NaN / 0 / negative / 17 A radius')
    assert np.isfinite(area).all()
    masked = base['mask'].copy()
    masked[0, 1, 1] = masked[0, 4, 0] = masked[0, 0, 0] = masked[0, 2, 1] = masked[0, 3, 2] = masked[0, 5, 3] = False
    pts2, area2 = statement(base['pos'], masked, base['group'], base['radius'], S, n)     # ... exactly as if those atoms were masked out
    assert np.array_equal(pts, pts2) and np.array_equal(area.view(np.int32), area2.view(np.int32))
    lone = dict(pos=np.array([[[[3.0, -2.0, 1.0]]]], dtype=np.float32), mask=np.ones((1, 1, 1), bool), group=np.array([[2]], dtype=np.int32), radius=radii_of(1))
    pts, area = check(lone, 'one lone atom')
    assert pts.tolist() == [[0, n, 0, n]] and area[0, 0, 0] == area[0, 0, 1] > 0
    pos, mask, group, rad = dev(base, 'pos', 'mask', 'group', 'radius')
    for g_, p_, m_ in ((group[:0], pos[:0], mask[:0]),):
        got = hip.sasa_grouped(p_, m_, g_, rad)
        assert got['pts'].shape == (0, 4) and got['area'].shape == (0, L, 2)
    ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
    out = torch.full((4,), 77, dtype=torch.int32, device=DEV)
    ar = torch.full((L * 2,), 77.0, device=DEV)
    d = hip.sphere_points(n, DEV)
    for G_, S_ in ((0, 3), (3, 0)):
        assert hip.lib().abopt_sasa_grouped(hip.ptr(pos), hip.ptr(mask), 0, hip.ptr(group), hip.ptr(rad.expand(1, L, A).contiguous()), hip.ptr(d), n, G_, S_, L, A,
                                            1.4, float(k_of(n)), hip.ptr(out), hip.ptr(ar), hip.ptr(ws), 64, hip.stream()) == 0
    torch.cuda.synchronize()
    assert (out == 77).all() and (ar == 77).all()


@pytest.mark.gpu
def test_grouped_call_equals_per_group_calls():
    G, S, L, A, n = 3, 2, 63, 5, 63
    c = case(G, S, L, A, n)
    pos, mask, group, rad = dev(c, 'pos', 'mask', 'group', 'radius')
    harness.grouped_equals_per_group(lambda **t: _bits(hip.sasa_grouped(radius=rad, points=n, **t)), [('sasa', G, S, dict(pos=pos, mask=mask, group=group))], {'group'})


@pytest.mark.gpu
def test_shared_mask_equals_expanded_mask():
    G, S, L, A, n = 2, 5, 65, 5, 64
    c = case(G, S, L, A, n)
    pos, mask, group, rad = dev(c, 'pos', 'mask', 'group', 'radius')
    shared = mask[::S].contiguous()                                                     # (G, L, A): the first candidate's mask for the whole group
    a = hip.sasa_grouped(pos, shared, group, rad, points=n)
    b = hip.sasa_grouped(pos, shared.repeat_interleave(S, 0), group, rad, points=n)
    assert torch.equal(a['pts'], b['pts']) and torch.equal(a['area'].view(torch.int32), b['area'].view(torch.int32))
    pts, area = statement(c['pos'], c['mask'][::S], c['group'], c['radius'], S, n)
    _assert_equals_statement(a, pts, area, 'shared mask')


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    """n = 0, n = 1025, A = 16, a negative / NaN / infinite probe, bad dims and G > 65535 through the C entry point: ABOPT_EINVAL with a message, and pts / area
    keep the pattern they were filled with; a short workspace: ABOPT_EWORKSPACE.  The wrapper raises for the same, and for a CPU tensor."""
    L_ = hip.lib()
    G, S, L, A, n = 2, 5, 65, 5, 64
    c = case(G, S, L, A, n)
    pos, mask, group = dev(c, 'pos', 'mask', 'group')
    rad = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(c['radius'], (G, L, A)))).to(DEV)
    dirs = hip.sphere_points(n, DEV)
    pts = torch.full((G * S, 4), 77, dtype=torch.int32, device=DEV)
    area = torch.full((G * S, L, 2), 77.0, device=DEV)
    need = L_.abopt_sasa_ws_bytes(G, S, L, A)
    assert need == G * S * L * 16 and L_.abopt_sasa_ws_bytes(0, S, L, A) == 0 and L_.abopt_sasa_ws_bytes(G, 0, L, A) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def call(G=G, S=S, L=L, A=A, n=n, probe=1.4, ws_bytes=need):
        return L_.abopt_sasa_grouped(hip.ptr(pos), hip.ptr(mask), 0, hip.ptr(group), hip.ptr(rad), hip.ptr(dirs), n, G, S, L, A, probe, float(k_of(max(n, 1))),
                                     hip.ptr(pts), hip.ptr(area), hip.ptr(ws), ws_bytes, hip.stream())
    for bad in (-1.0, float('nan'), float('inf')):
        assert call(probe=bad) == 1 and 'probe' in L_.abopt_last_error().decode()
    assert call(n=0) == 1 and 'n_points' in L_.abopt_last_error().decode()
    assert call(n=1025) == 1 and '1024' in L_.abopt_last_error().decode()
    assert call(A=16) == 1 and '16' in L_.abopt_last_error().decode()
    assert call(A=0) == 1 and call(L=0) == 1 and call(G=-1) == 1 and call(S=-1) == 1
    assert call(G=65536, S=1) == 1 and '65535' in L_.abopt_last_error().decode()
    assert call(ws_bytes=need - 1) == 4 and 'workspace too small' in L_.abopt_last_error().decode()
    assert call(G=0) == 0 and call(S=0) == 0                          # no-ops
    torch.cuda.synchronize()
    assert (pts == 77).all() and (area == 77).all()
    assert call() == 0                                                # ... and the same buffers are filled by a good call
    torch.cuda.synchronize()
    _assert_equals_statement(dict(pts=pts, area=area), c['pts'], c['area'], 'C entry')
    for bad in (-2.0, float('nan')):
        with pytest.raises(ValueError, match='probe'):
            hip.sasa_grouped(pos, mask, group, rad, probe=bad)
    for bad in (0, 1025):
        with pytest.raises(ValueError, match='1 .. 1024'):
            hip.sasa_grouped(pos, mask, group, rad, points=bad)
    with pytest.raises(ValueError, match='1 .. 15'):
        hip.sasa_grouped(torch.zeros(2, 5, 16, 3, device=DEV), torch.ones(2, 5, 16, dtype=torch.bool, device=DEV), group[:, :5], torch.ones(16, device=DEV))
    with pytest.raises(ValueError, match='whole groups'):
        hip.sasa_grouped(pos[:9], mask[:9], group, rad)
    with pytest.raises(RuntimeError, match='HIP device only'):
        hip.sasa_grouped(pos.cpu(), mask.cpu(), group.cpu(), rad.cpu())


@pytest.mark.gpu
def test_call_is_capturable():
    """One call recorded with torch.cuda.graph (two launches on one stream: a single chain, no parallel branch, no memset node) and replayed on OTHER inputs copied
    into the static tensors gives what the eager call gives on them."""
    G, S, L, A, n = 2, 5, 65, 5, 64
    a = case(G, S, L, A, n)
    other = _raw(G, S, L, A, 4242)
    pos, mask, group = dev(a, 'pos', 'mask', 'group')
    rad = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a['radius'], (G, L, A)))).to(DEV)
    first, held = harness.capture_replays_on_other_inputs(lambda **t: _bits(hip.sasa_grouped(radius=rad, points=n, **t)), dict(pos=pos, mask=mask, group=group),
                                                          {k: torch.from_numpy(src).to(DEV) for k, src in zip(('pos', 'mask', 'group'), other)})
    _assert_equals_statement(dict(pts=first['pts'], area=first['area'].view(torch.float32)), a['pts'], a['area'], 'replay on the captured inputs')
    assert not np.array_equal(held['pts'].cpu().numpy(), a['pts']), 'the other inputs give other counts'


@pytest.mark.gpu
def test_repeat_calls_are_bit_identical():
    G, S, L, A, n = 1, 1, 130, 5, 128                                                   # one candidate over many slices: the integer atomics meet on pts
    c = case(G, S, L, A, n)
    first = _run(c, n)
    for _ in range(5):
        again = _run(c, n)
        assert torch.equal(first['pts'], again['pts']) and torch.equal(first['area'].view(torch.int32), again['area'].view(torch.int32))


@pytest.mark.gpu
def test_buried_surface_summary():
    """sampler.buried_surface on the screen's complex: groups resolved as sampler.interface_geometry resolves them, bsa_res = free - complex >= 0, bsa / sasa the
    float64 sums rounded once, default radii = slot_radii."""
    one = screen_workers.complex_(DEV)
    L, A = one['pos_heavyatom'].shape[1:3]
    got = sampler.buried_surface(one, one['pos_heavyatom'], one['mask_heavyatom'], points=96)
    raw = hip.sasa_grouped(one['pos_heavyatom'], one['mask_heavyatom'], screen.chain_groups(one['fragment_type']), sampler.slot_radii(A), points=96)
    assert torch.equal(got['pts'], raw['pts']) and torch.equal(got['sasa_res'], raw['area'][..., 1])
    assert torch.equal(got['bsa_res'], raw['area'][..., 0] - raw['area'][..., 1]) and (got['bsa_res'] >= 0).all()
    assert torch.equal(got['bsa'], got['bsa_res'].double().sum(-1).float()) and torch.equal(got['sasa'], got['sasa_res'].double().sum(-1).float())
    assert got['sasa_res'].shape == (1, L) and got['bsa'].shape == (1,) and got['sasa'].item() > 0
    gen = sampler.buried_surface(one, one['pos_heavyatom'], one['mask_heavyatom'], groups='generated', points=96)
    side = torch.where(one['generate_flag'].bool(), 1, torch.where(one['fragment_type'] > 0, 2, 0))
    want = hip.sasa_grouped(one['pos_heavyatom'], one['mask_heavyatom'], side, sampler.slot_radii(A), points=96)
    assert torch.equal(gen['pts'], want['pts']) and gen['bsa'].item() > 0              # the generated loop is buried among its neighbours
