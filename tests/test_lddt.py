"""lDDT-CA: abopt_lddt_ca_grouped / abopt_lddt_ca_ensemble, hip.lddt_ca_grouped / hip.lddt_ca_ensemble, sampler.lddt_scores /
sampler.lddt_consistency and the screen's redock_lddt, redock_lddt_res, lddt_mean, lddt_std, lddt_res_mean, redock_consistency
(screen.optimize_antibody(lddt_cutoff=...), screen.screen_filter(min_lddt=...)).

The definition (include/abopt.h) is restated below in numpy / float64 (`pair_counts`).  Every result of the kernels is an integer count, so the device call has to
EQUAL the statement; fp32 and float64 may disagree only on a pair whose reference distance sits on the cutoff or whose distance error sits on one of the four
thresholds, so no test input has one.  The acceptance condition: in float64, no pair of residues (masks ignored: the condition then covers every mask a test puts
on the inputs), in any structure of a group as the reference and any other as the model, has dt within 1e-3 A of the cutoff or, with dt or dp below the cutoff,
e = |dt - dp| within 1e-3 A of 0.5, 1, 2 or 4.  fp32 subtraction of two fp32 coordinates errs by at most half an ulp of the DIFFERENCE, whatever the magnitude of the
coordinates, so every distance below 64 A is good to a few 1e-5 A and 1e-3 A leaves more than a factor of 20.  It is a condition on the inputs, not a tolerance
on the code.  A seed alone cannot meet it: a group of five candidates of 130 residues has 2.5e5 scored pairs, each within 1e-3 A of some threshold with probability
~2e-3.  So `case` generates the structures from a fixed seed and then `repair`, a deterministic pass on the CPU, moves the later residue of every offending pair by
about 0.05 A (trying displacements from the same fixed stream until that residue's pairs all keep the margin); the condition is asserted on the inputs used."""
import functools
import os

import numpy as np
import pytest
import torch

import lddt_workers
import screen_workers
from ab_opt_amd import screen

DEV = torch.device('cuda:0')
CUTOFF = 15.0                                             # the reference's
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
MARGIN = 1e-3
GS = [(1, 1), (3, 2), (2, 5)]
LS = [1, 2, 7, 63, 64, 65, 130]                           # the 64-residue tiles of rows and of j, and the smallest sizes
AS = [2, 4, 15]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lddt_small.npz')
FAR = (900.0, -700.0, 500.0)


# ------------------------------------------------------------------------------------------ the statement
def ca_dist(ca, dtype=np.float64):
    """CA (L, 3) -> (L, L) distances.  float64: the plain formula.  float32: the operation order of csrc/lddt.hip -- the coordinate differences rounded once,
    d2 = fma(dz, dz, fma(dy, dy, dx dx)) with each step rounded once (a product of two fp32 numbers is exact in float64, so rounding the float64 sum to fp32
    is the fused operation up to a double rounding that the margin covers a thousandfold), then the fp32 root."""
    if dtype == np.float64:
        x = np.asarray(ca, dtype=np.float64)
        d = x[:, None, :] - x[None, :, :]
        with np.errstate(invalid='ignore'):
            return np.sqrt((d * d).sum(-1))
    x = np.asarray(ca, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        d = x[:, None, :] - x[None, :, :]
        dx, dy, dz = (d[..., k].astype(np.float64) for k in range(3))
        f32 = lambda v: v.astype(np.float32).astype(np.float64)
        t = f32(dz * dz + f32(dy * dy + f32(dx * dx)))
        return np.sqrt(t.astype(np.float32))


def pair_counts(ref_ca, ref_ok, mod_ca, mod_ok, rows=None, group=None, cutoff=CUTOFF, dtype=np.float64):
    """The definition for ONE model against ONE reference: CA (L, 3), validity (L,) -> (num (L,), den (L,)) int64.  Comparisons with a NaN are false."""
    L = len(ref_ca)
    dt, dp = ca_dist(ref_ca, dtype), ca_dist(mod_ca, dtype)
    ok = np.asarray(ref_ok).astype(bool) & np.asarray(mod_ok).astype(bool)
    pair = ok[:, None] & ok[None, :] & ~np.eye(L, dtype=bool)
    if rows is not None:
        pair = pair & np.asarray(rows).astype(bool)[:, None]
    if group is not None:
        g = np.asarray(group)
        pair = pair & (((g[:, None] == 1) & (g[None, :] == 2)) | ((g[:, None] == 2) & (g[None, :] == 1)))
    with np.errstate(invalid='ignore'):
        scored = pair & (dt < dtype(cutoff))
        e = np.abs(dt - dp)
        hits = sum((e < dtype(t)).astype(np.int64) for t in THRESHOLDS)
    return (hits * scored).sum(1), scored.sum(1).astype(np.int64)


def grouped_statement(pos, mask, ref_pos, ref_mask, S, rows=None, group=None, cutoff=CUTOFF, dtype=np.float64):
    """pos (G*S, L, A, 3), mask (G*S, L, A) or (G, L, A), ref_pos (G, L, A, 3), ref_mask (G, L, A), rows / group (G, L) -> num, den (G*S, L) int64."""
    N, L = pos.shape[:2]
    num, den = np.zeros((N, L), dtype=np.int64), np.zeros((N, L), dtype=np.int64)
    for c in range(N):
        g = c // S
        m = mask[c] if mask.shape[0] == N else mask[g]
        num[c], den[c] = pair_counts(ref_pos[g, :, 1], ref_mask[g, :, 1], pos[c, :, 1], m[:, 1], None if rows is None else rows[g],
                                     None if group is None else group[g], cutoff, dtype)
    return num, den


def ensemble_statement(pos, mask, S, rows=None, group=None, cutoff=CUTOFF, dtype=np.float64):
    """-> num, den (G, S, S) int64: entry (g, a, b) = candidate a of the group as the reference, b as the model, summed over the residues."""
    N = pos.shape[0]
    G = N // S
    num, den = np.zeros((G, S, S), dtype=np.int64), np.zeros((G, S, S), dtype=np.int64)
    m = lambda c: (mask[c] if mask.shape[0] == N else mask[c // S])[:, 1]
    for g in range(G):
        for a in range(S):
            for b in range(S):
                n, d = pair_counts(pos[g * S + a, :, 1], m(g * S + a), pos[g * S + b, :, 1], m(g * S + b), None if rows is None else rows[g],
                                   None if group is None else group[g], cutoff, dtype)
                num[g, a, b], den[g, a, b] = n.sum(), d.sum()
    return num, den


def ratio_f64(num, den):
    """num / (4 den) in float64, -1 where den == 0."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.where(den > 0, num / (4.0 * np.maximum(den, 1.0)), -1.0)


def consistency_f64(num, den):
    """(G, S, S) -> (G, S): for model b the mean of num / (4 den) over the references a != b with den > 0; -1 if there is none."""
    S = num.shape[1]
    peer = (den > 0) & ~np.eye(S, dtype=bool)
    r = np.where(peer, ratio_f64(num, den), 0.0)
    cnt = peer.sum(1)
    return np.where(cnt > 0, r.sum(1) / np.maximum(cnt, 1), -1.0)


def lddt_torch(pos, mask, ref_pos, ref_mask, S, cutoff=CUTOFF, chunk=1000):
    """The plain torch statement of the grouped form on the device (fp32 cdist, about ten (chunk, L, L) temporaries), `chunk` candidates at a time: what the
    kernel's time is compared with in DESIGN.md section 6.5.  No rows, no group.  -> num, den (G*S, L) int64."""
    N, L = pos.shape[:2]
    eye = torch.eye(L, dtype=torch.bool, device=pos.device)
    nums, dens = [], []
    for lo in range(0, N, chunk):
        hi = min(lo + chunk, N)
        g = torch.arange(lo, hi, device=pos.device) // S
        m = mask[lo:hi] if mask.shape[0] == N else mask[g]
        ok = m[:, :, 1].bool() & ref_mask[g, :, 1].bool()
        rca, ca = ref_pos[g, :, 1], pos[lo:hi, :, 1]
        dt = torch.cdist(rca, rca, compute_mode='donot_use_mm_for_euclid_dist')
        dp = torch.cdist(ca, ca, compute_mode='donot_use_mm_for_euclid_dist')
        scored = ok[:, :, None] & ok[:, None, :] & ~eye & (dt < cutoff)
        e = (dt - dp).abs()
        hits = sum((e < t).long() for t in THRESHOLDS)
        nums.append((hits * scored).sum(2))
        dens.append(scored.sum(2))
    return torch.cat(nums), torch.cat(dens)


def ensemble_torch(pos, mask, S, cutoff=CUTOFF):
    """The same for the ensemble form: per group the S distance matrices, then one pass per reference a over the group's S models.  -> num, den (G, S, S) int64."""
    N, L = pos.shape[:2]
    G = N // S
    eye = torch.eye(L, dtype=torch.bool, device=pos.device)
    num, den = (torch.zeros(G, S, S, dtype=torch.int64, device=pos.device) for _ in range(2))
    for g in range(G):
        sl = slice(g * S, (g + 1) * S)
        ok = (mask[sl] if mask.shape[0] == N else mask[g:g + 1].expand(S, -1, -1))[:, :, 1].bool()
        D = torch.cdist(pos[sl, :, 1], pos[sl, :, 1], compute_mode='donot_use_mm_for_euclid_dist')
        for a in range(S):
            both = ok & ok[a]
            scored = both[:, :, None] & both[:, None, :] & ~eye & (D[a] < cutoff)
            e = (D[a] - D).abs()
            hits = sum((e < t).long() for t in THRESHOLDS)
            num[g, a], den[g, a] = (hits * scored).sum((1, 2)), scored.sum((1, 2))
    return num, den


# ------------------------------------------------------------------------------------------ the inputs
def _near(v, targets):
    out = np.zeros(v.shape, dtype=bool)
    with np.errstate(invalid='ignore'):
        for t in targets:
            out |= np.abs(v - t) <= MARGIN
    return out


def violations(X, cutoff=CUTOFF):
    """X (T, L, 3) fp32: the CA of the T structures of a group (the reference, if any, first).  -> (bad (T, L) bool: residue j of structure t is the later end of a
    pair that breaks the acceptance condition of the module docstring, D (T, L, L) float64 distances)."""
    T, L = X.shape[:2]
    D = np.stack([ca_dist(x) for x in X])
    upper = np.triu(np.ones((L, L), dtype=bool), 1)
    bad = np.zeros((T, L), dtype=bool)
    for a in range(T):
        bad[a] |= (upper & _near(D[a], (cutoff,))).any(0)
        for b in range(a + 1, T):
            with np.errstate(invalid='ignore'):
                live = upper & (np.minimum(D[a], D[b]) < cutoff + MARGIN)
                bad[b] |= (live & _near(np.abs(D[a] - D[b]), THRESHOLDS)).any(0)
    return bad, D


def _row_ok(t, j, d, D, cutoff):
    """Would residue j of structure t, with distances d (L,) to the residues of its structure, keep every pair it is in off the cutoff and the thresholds?"""
    others = np.ones(len(d), dtype=bool)
    others[j] = False
    if _near(d, (cutoff,))[others].any():
        return False
    for s in range(D.shape[0]):
        if s != t:
            live = others & (np.minimum(d, D[s, j]) < cutoff + MARGIN)
            if (live & _near(np.abs(d - D[s, j]), THRESHOLDS)).any():
                return False
    return True


def repair(X, rng, cutoff=CUTOFF):
    """X (T, L, 3) fp32 -> a copy in which the later residue of every offending pair has been moved by normal(0.05 A) per coordinate (rounded to fp32 again), the
    first displacement of the stream after which all pairs of that residue keep the margin: an accepted move creates no new offence, so one pass suffices."""
    X = X.copy()
    bad, D = violations(X, cutoff)
    for t, j in zip(*np.nonzero(bad)):
        for _ in range(500):
            p = (X[t, j].astype(np.float64) + rng.normal(size=3) * 0.05).astype(np.float32)
            d = np.sqrt(((X[t].astype(np.float64) - p.astype(np.float64)) ** 2).sum(-1))
            d[j] = 0.0
            if _row_ok(t, j, d, D, cutoff):
                X[t, j] = p
                D[t, j, :] = d
                D[t, :, j] = d
                break
        else:
            raise AssertionError(f'no displacement of residue {j} of structure {t} keeps the margin')
    return X


def walk(rng, L):
    step = rng.normal(size=(L, 3))
    step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
    return np.cumsum(step, 0)


def _raw(G, S, L, A, seed):
    """Per group a CA random walk of 3.8 A steps as the reference; candidate c is the reference with its CA perturbed by normal(sigma), sigma = 0.3, 1, 3 A in turn;
    the other atoms normal(1.2 A) around their CA.  Atom masks with probability 0.8; the CA byte is set except, from L = 7 on, at one residue of every candidate and
    one of every reference.  rows: half the residues (residue 0 always).  group: the first third side 1, the rest side 2, from L = 7 on two residues 0 and, in odd
    groups, two residues of each side swapped."""
    rng = np.random.default_rng(seed)
    N = G * S
    ref_pos, pos = np.zeros((G, L, A, 3)), np.zeros((N, L, A, 3))
    for g in range(G):
        ca = walk(rng, L)
        ref_pos[g] = ca[:, None] + rng.normal(size=(L, A, 3)) * 1.2
        ref_pos[g, :, 1] = ca
        for s in range(S):
            c = g * S + s
            mca = ca + rng.normal(size=(L, 3)) * (0.3, 1.0, 3.0)[c % 3]
            pos[c] = mca[:, None] + rng.normal(size=(L, A, 3)) * 1.2
            pos[c, :, 1] = mca
    ref_mask, mask = rng.random((G, L, A)) < 0.8, rng.random((N, L, A)) < 0.8
    ref_mask[:, :, 1] = True
    mask[:, :, 1] = True
    rows = rng.random((G, L)) < 0.5
    rows[:, 0] = True
    n1 = max(1, L // 3)
    group = np.full((G, L), 2, dtype=np.int32)
    group[:, :n1] = 1
    if L >= 7:
        for g in range(G):
            ref_mask[g, rng.integers(L), 1] = False
            if g % 2:
                group[g, rng.permutation(n1)[:2]] = 2
                group[g, n1 + rng.permutation(L - n1)[:2]] = 1
            group[g, rng.permutation(L)[:2]] = 0
        for c in range(N):
            mask[c, rng.integers(L), 1] = False
    return dict(pos=pos.astype(np.float32), mask=mask, ref_pos=ref_pos.astype(np.float32), ref_mask=ref_mask, rows=rows, group=group)


def _moved(x, shift):
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(1.1) * K + (1 - np.cos(1.1)) * K @ K
    return (x.astype(np.float64) @ R.T + np.array(shift)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(G, S, L, A, far=False):
    """Inputs that meet the acceptance condition, built once per shape and shared by the tests (read-only).  far: rotated about a fixed axis and moved by FAR,
    rounded to fp32 again, before the repair.  The seed is a fixed function of the shape."""
    seed = 1000 + 31 * L + 7 * A + 3 * G + S
    c = _raw(G, S, L, A, seed)
    if far:
        c['pos'], c['ref_pos'] = _moved(c['pos'], FAR), _moved(c['ref_pos'], FAR)
    rng = np.random.default_rng(seed + 1)
    for g in range(G):
        X = repair(np.concatenate([c['ref_pos'][g:g + 1, :, 1], c['pos'][g * S:(g + 1) * S, :, 1]]), rng)
        assert not violations(X)[0].any(), (G, S, L, A, far, g)            # a condition on the inputs, not on the code
        c['ref_pos'][g, :, 1], c['pos'][g * S:(g + 1) * S, :, 1] = X[0], X[1:]
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def want(G, S, L, A, far=False, use_rows=False, use_group=False, shared=False, ensemble=False, dtype=np.float64):
    """The statement on case(G, S, L, A, far) -> (num, den), computed once per variant."""
    c = case(G, S, L, A, far)
    mask = c['mask'][::S] if shared else c['mask']
    rows, group = (c['rows'] if use_rows else None), (c['group'] if use_group else None)
    if ensemble:
        return ensemble_statement(c['pos'], mask, S, rows, group, CUTOFF, dtype)
    return grouped_statement(c['pos'], mask, c['ref_pos'], c['ref_mask'], S, rows, group, CUTOFF, dtype)


def _dev(c, *names):
    return [torch.from_numpy(np.array(c[n])).to(DEV) for n in names]


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------ CPU
def test_statement_on_a_hand_worked_example():
    """Four residues on a line, cutoff 15: reference x = 0, 3, 10, 40; model x = 0, 3.6, 11.5, 40.
      dt: (0,1) 3  (0,2) 10  (1,2) 7  every pair with residue 3: 40, 37, 30 -- not scored, so residue 3 has den = 0
      dp: (0,1) 3.6  (0,2) 11.5  (1,2) 7.9        e: (0,1) 0.6 -> 3 hits   (0,2) 1.5 -> 2 hits   (1,2) 0.9 -> 3 hits
    -> den = 2, 2, 2, 0 and num = 5, 6, 5, 0; lddt_res = 0.625, 0.75, 0.625, -1; pooled 16 / 24.  rows, group, a masked residue and NaN coordinates after that."""
    line = lambda xs: np.stack([np.array(xs, dtype=np.float64), np.zeros(len(xs)), np.zeros(len(xs))], 1)
    ref, mod = line([0.0, 3.0, 10.0, 40.0]), line([0.0, 3.6, 11.5, 40.0])
    ok = np.ones(4, dtype=bool)
    num, den = pair_counts(ref, ok, mod, ok)
    assert den.tolist() == [2, 2, 2, 0] and num.tolist() == [5, 6, 5, 0]
    assert ratio_f64(num, den).tolist() == [0.625, 0.75, 0.625, -1.0] and ratio_f64(num.sum(), den.sum()) == 16 / 24
    num, den = pair_counts(ref, ok, mod, ok, rows=[1, 0, 1, 1])                      # rows selects i, not j
    assert den.tolist() == [2, 0, 2, 0] and num.tolist() == [5, 0, 5, 0]
    num, den = pair_counts(ref, ok, mod, ok, group=[1, 2, 2, 0])                     # (1, 2) are on one side
    assert den.tolist() == [2, 1, 1, 0] and num.tolist() == [5, 3, 2, 0]
    num, den = pair_counts(ref, ok, mod, [1, 0, 1, 1])                               # residue 1 invalid in the model: invalid in the pair
    assert den.tolist() == [1, 0, 1, 0] and num.tolist() == [2, 0, 2, 0]
    nan = mod.copy()
    nan[1, 2] = np.nan                                                               # a NaN dp: no hit, the pair still counts
    num, den = pair_counts(ref, ok, nan, ok)
    assert den.tolist() == [2, 2, 2, 0] and num.tolist() == [2, 0, 2, 0]
    num, den = pair_counts(nan, ok, mod, ok)                                         # a NaN dt is never scored; the pair (0, 2) is left: dt = dp = 11.5
    assert den.tolist() == [1, 0, 1, 0] and num.tolist() == [4, 0, 4, 0]
    num, den = pair_counts(ref, ok, ref, ok, cutoff=7.0)                             # strict: dt = 7 is not scored; identical structures: num = 4 den
    assert den.tolist() == [1, 1, 0, 0] and num.tolist() == [4, 4, 0, 0]
    n3, d3 = ensemble_statement(np.stack([ref, mod])[:, :, None, :].repeat(2, 2), np.ones((2, 4, 2), dtype=bool), 2)
    assert d3.tolist() == [[[6, 6], [6, 6]]] and n3.tolist() == [[[24, 16], [16, 24]]]
    assert consistency_f64(n3, d3).tolist() == [[16 / 24, 16 / 24]]
    assert consistency_f64(np.zeros((1, 1, 1)), np.zeros((1, 1, 1))).tolist() == [[-1.0]]


def _grid():
    return [(G, S, L, A) for G, S in GS for L in LS for A in AS]


def test_fp32_statement_equals_the_float64_statement_on_every_test_input():
    """The numpy-float32 restatement of the kernel's operation order gives the counts of the float64 statement on every input of the GPU grid, near the origin and
    moved by FAR (the L = 65 cases), grouped and ensemble, with rows and group: the acceptance condition does its job.  The CA does not depend on A beyond the seed,
    so one A per (G, S, L) is walked with all variants and the others plainly."""
    checked = 0
    for G, S, L, A in _grid():
        variants = [(False, False), (True, True)] if A == 4 else [(False, False)]
        for far in ((False, True) if L == 65 else (False,)):
            for use_rows, use_group in variants:
                for ens in (False, True):
                    a = want(G, S, L, A, far, use_rows, use_group, False, ens)
                    b = want(G, S, L, A, far, use_rows, use_group, False, ens, np.float32)
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (G, S, L, A, far, use_rows, use_group, ens)
                    checked += int(a[1].sum())
    assert checked > 10 ** 6                                                         # scored pairs that were compared
    spread = ratio_f64(*(x.sum(1) for x in want(2, 5, 130, 4)))
    assert spread.min() < 0.5 < 0.8 < spread.max(), spread                           # sigma = 0.3 / 1 / 3 A spread the scores over (0, 1)


def test_matches_the_reference_fixture_statement():
    """pair_counts against lddt() of the reference (AbDock/src/modules/common/plddt.py) on the fixture's inputs: per residue and pooled within 1e-6 wherever
    den > 0 (the reference works in fp32 with eps = 1e-10 inside the root and around the ratio: three roundings of a number <= 1, 1.8e-7, times five), and the
    documented divergence where den == 0: the reference returns eps / eps = 1.0, this library -1.  The fixture's inputs meet the acceptance condition."""
    z = np.load(GOLDEN)
    far_seen = 0
    for L in (7, 65):
        ref, mod, mask = z[f'ref_{L}'], z[f'model_{L}'], z[f'mask_{L}'][..., 0] > 0
        assert ref.shape == (4, L, 3) and ref.dtype == np.float32 and float(z['cutoff']) == CUTOFF and not mask.all()
        for b in range(4):
            assert not violations(np.stack([ref[b], mod[b]]))[0].any(), (L, b)
            num, den = pair_counts(ref[b], mask[b], mod[b], mask[b])
            res = ratio_f64(num, den)
            scored = den > 0
            assert np.abs(res[scored] - z[f'per_residue_{L}'][b][scored]).max(initial=0.0) <= 1e-6, (L, b)
            assert (res[~scored] == -1.0).all() and (z[f'per_residue_{L}'][b][~scored] == 1.0).all(), (L, b)
            far_seen += int((~scored & mask[b]).sum())
            assert den.sum() > 0 and abs(ratio_f64(num.sum(), den.sum()) - z[f'pooled_{L}'][b]) <= 1e-6, (L, b)
    assert far_seen >= 2                                                             # valid residues farther than the cutoff from everything


def test_cutoff_is_validated_without_a_device():
    """hip.check_lddt_cutoff, the two hip calls, the two sampler calls and optimize_antibody refuse a non-positive or non-finite cutoff and malformed shapes with
    ValueError before anything touches a device: the tensors live on the CPU and the models are None.  Valid arguments reach the binding, which has no CPU path."""
    from ab_opt_amd import hip, sampler
    from ab_opt_amd.utils import synth
    assert hip.check_lddt_cutoff('x', 15) == 15.0
    pos, mask = torch.zeros(4, 6, 4, 3), torch.ones(4, 6, 4, dtype=torch.bool)
    rpos, rmask = torch.zeros(2, 6, 4, 3), torch.ones(2, 6, 4, dtype=torch.bool)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='finite and > 0'):
            hip.check_lddt_cutoff('x', bad)
        with pytest.raises(ValueError, match='cutoff'):
            hip.lddt_ca_grouped(pos, mask, rpos, rmask, cutoff=bad)
        with pytest.raises(ValueError, match='cutoff'):
            hip.lddt_ca_ensemble(pos, mask, 2, cutoff=bad)
        with pytest.raises(ValueError, match='cutoff'):
            sampler.lddt_scores(pos, mask, rpos, rmask, cutoff=bad)
        with pytest.raises(ValueError, match='cutoff'):
            sampler.lddt_consistency(pos, mask, 2, cutoff=bad)
    with pytest.raises(ValueError, match='whole groups'):
        hip.lddt_ca_grouped(pos[:3], mask[:3], rpos, rmask)
    with pytest.raises(ValueError, match='whole groups'):
        hip.lddt_ca_ensemble(pos, mask, 3)
    with pytest.raises(ValueError, match='neither per candidate nor per group'):
        hip.lddt_ca_grouped(pos, mask[:3], rpos, rmask)
    with pytest.raises(ValueError, match='2 .. 15'):
        hip.lddt_ca_grouped(pos[:, :, :1], mask[:, :, :1], rpos[:, :, :1], rmask[:, :, :1])
    with pytest.raises(ValueError, match='2 .. 15'):
        hip.lddt_ca_ensemble(torch.zeros(4, 6, 16, 3), torch.ones(4, 6, 16, dtype=torch.bool), 2)
    with pytest.raises(ValueError, match='do not match'):
        hip.lddt_ca_grouped(pos, mask, rpos[:, :5], rmask[:, :5])
    with pytest.raises(ValueError, match='rows'):
        hip.lddt_ca_grouped(pos, mask, rpos, rmask, rows=torch.ones(2, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match='group'):
        hip.lddt_ca_ensemble(pos, mask, 2, group=torch.ones(4, 6, dtype=torch.int32))
    with pytest.raises(ValueError, match='fragment_type'):
        sampler.lddt_scores(pos, mask, rpos, rmask, interface=True)
    with pytest.raises(RuntimeError, match='HIP device only'):
        hip.lddt_ca_grouped(pos, mask, rpos, rmask)
    with pytest.raises(RuntimeError, match='HIP device only'):
        hip.lddt_ca_ensemble(pos, mask, 2)
    one = synth.make_batch(1, synth.LAYOUT_128, seed=21)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='lddt_cutoff'):
            screen.optimize_antibody(None, None, one, 4, 2, 2, lddt_cutoff=bad)


def test_screen_filter_min_lddt():
    """screen_filter on a hand-made result: without min_lddt what the median rule alone returns; with it, additionally the MEDIAN over the D re-docks of redock_lddt
    >= min_lddt (the mean of the two middle values for an even D; a -1 enters as it is)."""
    flat = torch.zeros(3, 2)                                         # every design sits on every median: the median rule keeps all
    ld = torch.tensor([[[0.9, 0.2, 0.7], [0.1, 0.2, 0.9]], [[-1.0, 0.8, 0.6], [-1.0, -1.0, 0.9]], [[0.5, 0.5, 0.5], [0.49, 0.6, 0.3]]])    # medians .7 .2 | .6 -1 | .5 .49
    res = dict(dockq_std=flat, prmsd_std=flat.clone(), prmsd_mean=flat.clone(), redock_lddt=ld)
    assert screen.screen_filter(res).all() and screen.screen_filter(res, min_lddt=None).all()
    assert screen.screen_filter(res, min_lddt=0.5).tolist() == [[True, False], [True, False], [True, False]]
    assert screen.screen_filter(res, min_lddt=0.65).tolist() == [[True, False], [False, False], [False, False]]
    assert screen.screen_filter(res, min_lddt=-1.0).all()
    even = dict(res, redock_lddt=torch.tensor([[[0.2, 0.4, 0.8, 1.0]]]).expand(3, 2, 4))                 # median 0.6
    assert screen.screen_filter(even, min_lddt=0.6).all() and not screen.screen_filter(even, min_lddt=0.61).any()
    with pytest.raises(ValueError, match='redock_lddt'):
        screen.screen_filter(dict(dockq_std=flat, prmsd_std=flat, prmsd_mean=flat), min_lddt=0.5)
    m, s = screen._scored_mean_std(ld, -1)
    assert torch.allclose(m, torch.tensor([[0.6, 0.4], [0.7, 0.9], [0.5, 1.39 / 3]]), atol=1e-6) and abs(float(s[1, 0]) - 0.1) < 1e-6 and float(s[1, 1]) == 0.0
    assert screen._scored_mean_std(torch.full((2, 3), -1.0), -1)[0].tolist() == [-1.0, -1.0]


# ------------------------------------------------------------------------------------------ GPU: the kernels
def _check_grouped(got, num, den, tag):
    assert all(got[k].is_cuda for k in ('num', 'den', 'lddt_res', 'lddt')) and got['num'].dtype == torch.int32 and got['den'].dtype == torch.int32, tag
    assert np.array_equal(_np(got['den']), den), (tag, 'den')
    assert np.array_equal(_np(got['num']), num), (tag, 'num')
    assert got['lddt_res'].dtype == torch.float32 and np.abs(_np(got['lddt_res']) - ratio_f64(num, den)).max(initial=0.0) <= 1e-7, tag
    assert got['lddt'].dtype == torch.float32 and np.abs(_np(got['lddt']) - ratio_f64(num.sum(1), den.sum(1))).max(initial=0.0) <= 1e-7, tag


def _check_ensemble(got, num, den, tag):
    assert all(got[k].is_cuda for k in ('num', 'den', 'lddt', 'consistency')) and got['num'].dtype == torch.int32 and got['den'].dtype == torch.int32, tag
    assert np.array_equal(_np(got['den']), den), (tag, 'den')
    assert np.array_equal(_np(got['num']), num), (tag, 'num')
    assert np.abs(_np(got['lddt']) - ratio_f64(num, den)).max(initial=0.0) <= 1e-7, tag
    assert got['consistency'].shape == num.shape[:2] and np.abs(_np(got['consistency']) - consistency_f64(num, den)).max(initial=0.0) <= 1e-7, tag
    diag = np.diagonal(den, axis1=1, axis2=2)
    assert np.array_equal(np.diagonal(num, axis1=1, axis2=2), 4 * diag), tag


def _run_variants(G, S, L, A, far):
    from ab_opt_amd import hip
    c = case(G, S, L, A, far)
    pos, mask, ref_pos, ref_mask, rows, group = _dev(c, 'pos', 'mask', 'ref_pos', 'ref_mask', 'rows', 'group')
    for use_rows in (False, True):
        for use_group in (False, True):
            kw = dict(rows=rows if use_rows else None, group=group if use_group else None, cutoff=CUTOFF)
            tag = (G, S, L, A, far, use_rows, use_group)
            num, den = want(G, S, L, A, far, use_rows, use_group)
            _check_grouped(hip.lddt_ca_grouped(pos, mask, ref_pos, ref_mask, **kw), num, den, tag)
            enum, eden = want(G, S, L, A, far, use_rows, use_group, False, True)
            _check_ensemble(hip.lddt_ca_ensemble(pos, mask, S, **kw), enum, eden, tag)
    shared = mask[::S].contiguous()
    num, den = want(G, S, L, A, far, False, False, True)
    _check_grouped(hip.lddt_ca_grouped(pos, shared, ref_pos, ref_mask), num, den, (G, S, L, A, far, 'shared'))
    enum, eden = want(G, S, L, A, far, False, False, True, True)
    _check_ensemble(hip.lddt_ca_ensemble(pos, shared, S), enum, eden, (G, S, L, A, far, 'shared'))
    return num, den


@pytest.mark.gpu
@pytest.mark.parametrize('A', AS)
@pytest.mark.parametrize('L', LS)
@pytest.mark.parametrize('G,S', GS)
def test_counts_equal_the_float64_statement(G, S, L, A):
    """num and den of both entry points are exactly those of the numpy / float64 statement: with and without rows, with and without group, with per-candidate
    masks and with a mask shared by the group; the floats derived from them are the statement's ratios."""
    num, den = _run_variants(G, S, L, A, False)
    print(f'(G, S, L, A) = {(G, S, L, A)}: pooled lDDT {np.round(ratio_f64(num.sum(1), den.sum(1)), 3).tolist()}')
    if L >= 63:
        assert den.sum() > 0 and (den == 0).any()                   # an invalid residue holds 0, and something is scored


@pytest.mark.gpu
def test_torch_statement_equals_the_float64_statement():
    """lddt_torch / ensemble_torch (the statements the kernels' times are compared with in DESIGN.md section 6.5) give the float64 counts on a case with a margin."""
    G, S, L, A = 2, 5, 65, 4
    c = case(G, S, L, A)
    pos, mask, ref_pos, ref_mask = _dev(c, 'pos', 'mask', 'ref_pos', 'ref_mask')
    num, den = lddt_torch(pos, mask, ref_pos, ref_mask, S, chunk=3)
    assert np.array_equal(_np(num), want(G, S, L, A)[0]) and np.array_equal(_np(den), want(G, S, L, A)[1])
    num, den = ensemble_torch(pos, mask, S)
    e = want(G, S, L, A, False, False, False, False, True)
    assert np.array_equal(_np(num), e[0]) and np.array_equal(_np(den), e[1])


@pytest.mark.gpu
def test_matches_the_reference_fixture():
    """hip.lddt_ca_grouped on the fixture's inputs (A = 2, CA in slot 1, one group per structure) against the recorded lddt() of the reference: lddt_res and lddt
    within 1e-6 wherever den > 0 (three fp32 roundings of a number <= 1 give <= 1.8e-7; a factor of five on top), -1 where den == 0 -- there the reference holds 1.0."""
    from ab_opt_amd import hip
    z = np.load(GOLDEN)
    for L in (7, 65):
        ref, mod, m = z[f'ref_{L}'], z[f'model_{L}'], z[f'mask_{L}'][..., 0] > 0
        lift = lambda ca: torch.from_numpy(np.stack([ca + 1.0, ca], 2)).to(DEV)                  # slot 0 holds something else
        mask = torch.from_numpy(np.stack([m, m], 2)).to(DEV)
        got = hip.lddt_ca_grouped(lift(mod), mask, lift(ref), mask, cutoff=float(z['cutoff']))
        den = _np(got['den'])
        res, pooled = _np(got['lddt_res']), _np(got['lddt'])
        assert np.abs(res - z[f'per_residue_{L}'])[den > 0].max() <= 1e-6, L
        assert (res[den == 0] == -1.0).all() and (z[f'per_residue_{L}'][den == 0] == 1.0).all() and (den == 0).any(), L
        assert (den.sum(1) > 0).all() and np.abs(pooled - z[f'pooled_{L}']).max() <= 1e-6, L


@pytest.mark.gpu
def test_ensemble_entry_equals_the_grouped_call_with_that_peer_as_reference():
    """Entry (g, a, :) of the ensemble call equals, bit for bit, the sum over L of a grouped call handed candidate a of every group as ref_pos / ref_mask."""
    from ab_opt_amd import hip
    for (G, S, L, A), use in (((2, 5, 65, 4), False), ((3, 2, 130, 15), True), ((2, 5, 7, 2), True)):
        c = case(G, S, L, A)
        pos, mask, rows, group = _dev(c, 'pos', 'mask', 'rows', 'group')
        kw = dict(rows=rows if use else None, group=group if use else None)
        ens = hip.lddt_ca_ensemble(pos, mask, S, **kw)
        for a in range(S):
            one = hip.lddt_ca_grouped(pos, mask, pos[a::S].contiguous(), mask[a::S].contiguous(), **kw)
            for k in ('num', 'den'):
                assert torch.equal(ens[k][:, a, :], one[k].view(G, S, L).sum(2, dtype=torch.int32)), (G, S, L, A, a, k)


@pytest.mark.gpu
@pytest.mark.parametrize('A', AS)
@pytest.mark.parametrize('G,S', GS)
def test_far_from_the_origin(G, S, A):
    """The grid's L = 65 cases rotated and moved by (900, -700, 500) A (one ulp of a coordinate: 6e-5 A), the acceptance condition asserted on the moved fp32
    inputs: the counts still equal the float64 statement -- the differences of coordinates are what is rounded, not the coordinates."""
    _run_variants(G, S, 65, A, True)


@pytest.mark.gpu
def test_grouped_call_equals_per_group_calls():
    """G groups in one call against G single-group calls, both entry points: torch.equal on num and den."""
    from ab_opt_amd import hip
    for G, S in ((3, 2), (2, 5)):
        for L, A in ((7, 4), (65, 15), (130, 2)):
            c = case(G, S, L, A)
            pos, mask, ref_pos, ref_mask, rows, group = _dev(c, 'pos', 'mask', 'ref_pos', 'ref_mask', 'rows', 'group')
            got = hip.lddt_ca_grouped(pos, mask, ref_pos, ref_mask, rows=rows, group=group)
            ens = hip.lddt_ca_ensemble(pos, mask, S, rows=rows, group=group)
            for g in range(G):
                sl, gg = slice(g * S, (g + 1) * S), slice(g, g + 1)
                one = hip.lddt_ca_grouped(pos[sl], mask[sl], ref_pos[gg], ref_mask[gg], rows=rows[gg], group=group[gg])
                eone = hip.lddt_ca_ensemble(pos[sl], mask[sl], S, rows=rows[gg], group=group[gg])
                for k in ('num', 'den'):
                    assert torch.equal(got[k][sl], one[k]) and torch.equal(ens[k][gg], eone[k]), (G, S, L, A, g, k)


@pytest.mark.gpu
def test_shared_mask_equals_expanded_mask():
    """mask (G, L, A) shared by the S candidates of a group against the same mask repeated per candidate: torch.equal, both entry points."""
    from ab_opt_amd import hip
    for G, S, L, A in ((3, 2, 65, 15), (2, 5, 63, 4)):
        c = case(G, S, L, A)
        pos, mask, ref_pos, ref_mask, rows = _dev(c, 'pos', 'mask', 'ref_pos', 'ref_mask', 'rows')
        shared = mask[::S].contiguous()
        exp = shared.repeat_interleave(S, 0)
        a, b = hip.lddt_ca_grouped(pos, shared, ref_pos, ref_mask, rows=rows), hip.lddt_ca_grouped(pos, exp, ref_pos, ref_mask, rows=rows)
        ea, eb = hip.lddt_ca_ensemble(pos, shared, S, rows=rows), hip.lddt_ca_ensemble(pos, exp, S, rows=rows)
        for k in ('num', 'den'):
            assert torch.equal(a[k], b[k]) and torch.equal(ea[k], eb[k]), (G, S, L, A, k)
        assert not torch.equal(a['den'], hip.lddt_ca_grouped(pos, mask, ref_pos, ref_mask, rows=rows)['den'])     # the masks do differ


@pytest.mark.gpu
def test_candidate_split_over_workgroups_and_whole_tiles():
    """Few candidates: the j-tiles of a unit are split over several workgroups (case(1, 1, 130, 4): three grouped units and one ensemble unit on a whole chip; the
    grid covers it and this names it).  Many candidates: every unit walks all its tiles in one wave -- the ten candidates of case(2, 5, 130, 15) repeated into
    G = 8 groups of S >= 176 (S such that the grouped call has sixteen waves per CU without a split).  Group g repeats the candidates of base group g % 2, so the
    grouped counts are the base's rows and ensemble entry (g, a, b) is base entry (g % 2, a % 5, b % 5)."""
    from ab_opt_amd import hip
    c = case(1, 1, 130, 4)
    pos, mask, ref_pos, ref_mask = _dev(c, 'pos', 'mask', 'ref_pos', 'ref_mask')
    _check_grouped(hip.lddt_ca_grouped(pos, mask, ref_pos, ref_mask), *want(1, 1, 130, 4), 'few')
    _check_ensemble(hip.lddt_ca_ensemble(pos, mask, 1), *want(1, 1, 130, 4, False, False, False, False, True), 'few')
    c = case(2, 5, 130, 15)
    G = 8
    S = max(176, -(-16 * hip.device_info()['cu_count'] // (3 * G)))
    pick = np.array([(g % 2) * 5 + s % 5 for g in range(G) for s in range(S)])
    base = [g % 2 for g in range(G)]
    pos, mask = torch.from_numpy(c['pos'][pick]).to(DEV), torch.from_numpy(c['mask'][pick]).to(DEV)
    ref_pos, ref_mask = torch.from_numpy(c['ref_pos'][base]).to(DEV), torch.from_numpy(c['ref_mask'][base]).to(DEV)
    rows, group = torch.from_numpy(c['rows'][base]).to(DEV), torch.from_numpy(c['group'][base]).to(DEV)
    num, den = want(2, 5, 130, 15, False, True, True)
    got = hip.lddt_ca_grouped(pos, mask, ref_pos, ref_mask, rows=rows, group=group)
    assert np.array_equal(_np(got['num']), num[pick]) and np.array_equal(_np(got['den']), den[pick])
    enum, eden = want(2, 5, 130, 15, False, True, True, False, True)
    s5 = np.arange(S) % 5
    ens = hip.lddt_ca_ensemble(pos, mask, S, rows=rows, group=group)
    for g in range(G):
        assert np.array_equal(_np(ens['num'][g]), enum[g % 2][np.ix_(s5, s5)]) and np.array_equal(_np(ens['den'][g]), eden[g % 2][np.ix_(s5, s5)]), g


@pytest.mark.gpu
def test_degenerate_inputs():
    """G = 0 and S = 0: empty results, nothing launched.  Every CA masked out: all zeros and -1.  NaN coordinates in a model residue: no hit, the pairs still count;
    in a reference residue: its pairs are not scored -- both as the statement says, both entry points."""
    from ab_opt_amd import hip
    G, S, L, A = 2, 5, 65, 4
    c = case(G, S, L, A)
    pos, mask, ref_pos, ref_mask, rows, group = _dev(c, 'pos', 'mask', 'ref_pos', 'ref_mask', 'rows', 'group')
    got = hip.lddt_ca_grouped(pos[:0], mask[:0], ref_pos[:0], ref_mask[:0], rows=rows[:0], group=group[:0])
    assert got['num'].shape == (0, L) and got['lddt'].shape == (0,) and got['lddt_res'].shape == (0, L)
    got = hip.lddt_ca_grouped(pos[:0], mask[:0], ref_pos, ref_mask)                               # S = 0
    assert got['den'].shape == (0, L)
    got = hip.lddt_ca_ensemble(pos[:0], mask[:0], S)
    assert got['num'].shape == (0, S, S) and got['consistency'].shape == (0, S)
    none = torch.zeros_like(mask)
    got = hip.lddt_ca_grouped(pos, none, ref_pos, ref_mask)
    assert (got['num'] == 0).all() and (got['den'] == 0).all() and (got['lddt_res'] == -1).all() and (got['lddt'] == -1).all()
    got = hip.lddt_ca_grouped(pos, mask, ref_pos, torch.zeros_like(ref_mask))
    assert (got['den'] == 0).all() and (got['lddt'] == -1).all()
    got = hip.lddt_ca_ensemble(pos, none, S)
    assert (got['den'] == 0).all() and (got['lddt'] == -1).all() and (got['consistency'] == -1).all()
    valid = np.nonzero(c['mask'][:, :, 1].all(0) & c['ref_mask'][:, :, 1].all(0))[0]
    r = int(valid[len(valid) // 2])                                                              # a residue whose CA is valid everywhere
    bad = c['pos'].copy()
    bad[:, r, 1, 1] = np.nan                                                                      # the model side, every candidate
    num, den = grouped_statement(bad, c['mask'], c['ref_pos'], c['ref_mask'], S)
    plain = want(G, S, L, A)
    assert np.array_equal(den, plain[1]) and (num[:, r] == 0).all() and (den[:, r] > 0).all() and num.sum() < plain[0].sum()
    _check_grouped(hip.lddt_ca_grouped(torch.from_numpy(bad).to(DEV), mask, ref_pos, ref_mask), num, den, 'NaN in the model')
    enum, eden = ensemble_statement(bad, c['mask'], S)
    ens = hip.lddt_ca_ensemble(torch.from_numpy(bad).to(DEV), mask, S)
    assert np.array_equal(_np(ens['num']), enum) and np.array_equal(_np(ens['den']), eden)        # every structure is a reference here: residue r is never scored
    badref = c['ref_pos'].copy()
    badref[:, r, 1, 2] = np.nan
    num, den = grouped_statement(c['pos'], c['mask'], badref, c['ref_mask'], S)
    assert (den[:, r] == 0).all() and den.sum() < plain[1].sum()
    _check_grouped(hip.lddt_ca_grouped(pos, mask, torch.from_numpy(badref).to(DEV), ref_mask), num, den, 'NaN in the reference')


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    """Through the C entry points: a non-positive / NaN / infinite cutoff, A = 1 and 16, L = 0, negative G and S, G > 65535 and G S S > 2^31 - 1: ABOPT_EINVAL;
    L > 16384 and, for the ensemble form, S > 16384: ABOPT_EUNSUPPORTED; a short workspace: ABOPT_EWORKSPACE -- each with a message, and num / den keep the
    pattern they were filled with.  G = 0 and S = 0 are no-ops.  Then the same buffers are filled by a good call.  The Python wrappers raise for the same."""
    from ab_opt_amd import hip
    L_ = hip.lib()
    G, S, L, A = 2, 5, 65, 4
    c = case(G, S, L, A)
    pos, mask, ref_pos, ref_mask, rows, group = _dev(c, 'pos', 'mask', 'ref_pos', 'ref_mask', 'rows', 'group')
    num, den = torch.full((G * S, L), 77, dtype=torch.int32, device=DEV), torch.full((G * S, L), 77, dtype=torch.int32, device=DEV)
    enum, eden = torch.full((G, S, S), 77, dtype=torch.int32, device=DEV), torch.full((G, S, S), 77, dtype=torch.int32, device=DEV)
    need = L_.abopt_lddt_ws_bytes(G, S, L)
    assert need == (G * S + G) * L * 16 + G * L * 4 + G * 4 and L_.abopt_lddt_ws_bytes(0, S, L) == 0 and L_.abopt_lddt_ws_bytes(G, 0, L) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p = hip.ptr

    def grouped(G=G, S=S, L=L, A=A, cutoff=CUTOFF, ws_bytes=need):
        return L_.abopt_lddt_ca_grouped(p(pos), p(mask), 0, p(ref_pos), p(ref_mask), p(rows), p(group), G, S, L, A, cutoff, p(num), p(den), p(ws), ws_bytes, hip.stream())

    def ensemble(G=G, S=S, L=L, A=A, cutoff=CUTOFF, ws_bytes=need):
        return L_.abopt_lddt_ca_ensemble(p(pos), p(mask), 0, p(rows), p(group), G, S, L, A, cutoff, p(enum), p(eden), p(ws), ws_bytes, hip.stream())
    err = lambda: L_.abopt_last_error().decode()
    for call in (grouped, ensemble):
        for bad in (0.0, -1.0, float('nan'), float('inf')):
            assert call(cutoff=bad) == 1 and 'cutoff' in err()
        assert call(A=1) == 1 and call(A=16) == 1 and '16' in err()
        assert call(L=0) == 1 and call(G=-1) == 1 and call(S=-1) == 1
        assert call(G=65536, S=1) == 1 and '65535' in err()
        assert call(L=16385) == 3 and '16384' in err()
        assert call(ws_bytes=need - 1) == 4 and 'workspace too small' in err()
        assert call(G=0) == 0 and call(S=0) == 0
    assert ensemble(G=1, S=16385) == 3 and '16384' in err() and ensemble(G=9, S=16384) == 1 and '2^31' in err()
    torch.cuda.synchronize()
    assert (num == 77).all() and (den == 77).all() and (enum == 77).all() and (eden == 77).all()
    assert grouped() == 0 and ensemble() == 0
    torch.cuda.synchronize()
    want_g, want_e = want(G, S, L, A, False, True, True), want(G, S, L, A, False, True, True, False, True)
    assert np.array_equal(_np(num), want_g[0]) and np.array_equal(_np(den), want_g[1])
    assert np.array_equal(_np(enum), want_e[0]) and np.array_equal(_np(eden), want_e[1])
    for bad in (0.0, float('nan')):
        with pytest.raises(ValueError, match='cutoff'):
            hip.lddt_ca_grouped(pos, mask, ref_pos, ref_mask, cutoff=bad)
        with pytest.raises(ValueError, match='cutoff'):
            hip.lddt_ca_ensemble(pos, mask, S, cutoff=bad)
    with pytest.raises(ValueError, match='whole groups'):
        hip.lddt_ca_grouped(pos[:9], mask[:9], ref_pos, ref_mask)
    with pytest.raises(ValueError, match='whole groups'):
        hip.lddt_ca_ensemble(pos, mask, 3)
    with pytest.raises(RuntimeError, match='HIP device only'):
        hip.lddt_ca_grouped(pos.cpu(), mask.cpu(), ref_pos.cpu(), ref_mask.cpu())
    with pytest.raises(RuntimeError, match='HIP device only'):
        hip.lddt_ca_ensemble(pos.cpu(), mask.cpu(), S)


@pytest.mark.gpu
def test_call_is_capturable():
    """Both calls recorded with torch.cuda.graph (two launches each on one stream: a single chain, no memset node) and replayed on OTHER inputs copied into the
    static tensors, without a synchronisation between the copy and the replay, give what the eager calls give on them."""
    from ab_opt_amd import hip
    G, S, L, A = 2, 5, 65, 4
    a, b = case(G, S, L, A), case(G, S, L, 15)                                       # other structures of the same (G, S, L); their first four atoms serve
    names = ('pos', 'mask', 'ref_pos', 'ref_mask', 'rows', 'group')
    pos, mask, ref_pos, ref_mask, rows, group = _dev(a, *names)
    other = [torch.from_numpy(np.array(b[n][:, :, :A] if n in names[:4] else b[n])).to(DEV) for n in names]
    run = lambda: (hip.lddt_ca_grouped(pos, mask, ref_pos, ref_mask, rows=rows, group=group), hip.lddt_ca_ensemble(pos, mask, S, rows=rows, group=group))
    run()                                                                            # library load, device queries, workspace
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = run()
    graph.replay()
    torch.cuda.synchronize()
    num, den = want(G, S, L, A, False, True, True)
    assert np.array_equal(_np(held[0]['num']), num) and np.array_equal(_np(held[0]['den']), den)
    enum, eden = want(G, S, L, A, False, True, True, False, True)
    assert np.array_equal(_np(held[1]['num']), enum) and np.array_equal(_np(held[1]['den']), eden)
    for dst, src in zip((pos, mask, ref_pos, ref_mask, rows, group), other):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    eager = run()
    for h, e in zip(held, eager):
        for k in h:
            assert torch.equal(h[k], e[k]), k
    assert not np.array_equal(_np(held[0]['num']), num), 'the other inputs give other counts'


# ------------------------------------------------------------------------------------------ GPU: the screen
LDDT = dict(lddt_workers.LDDT)
NEW = {'redock_lddt', 'redock_lddt_res', 'lddt_mean', 'lddt_std', 'lddt_res_mean', 'redock_consistency'}


@pytest.fixture
def screen_models():
    """(dock, design) of screen_workers with no captured denoising loop before or after the test (tests/test_interface_geometry.py: the graph key does not hold the
    ABOPT_PAIR_TERMS / ABOPT_CORE_NO_SPLIT switches)."""
    pair = screen_workers.models(DEV)
    for m in pair:
        m.diffusion.clear_graphs()
    yield pair
    for m in pair:
        m.diffusion.clear_graphs()


def _shapes(res, lead, k, D, n):
    assert res['redock_lddt'].shape == (lead, k, D) and res['redock_lddt_res'].shape == (lead, k, D, n) and res['redock_consistency'].shape == (lead, k, D)
    assert res['lddt_mean'].shape == (lead, k) and res['lddt_std'].shape == (lead, k) and res['lddt_res_mean'].shape == (lead, k, n)
    for name in NEW:
        t = res[name]
        assert t.dtype == torch.float32 and bool((((t >= 0) & (t <= 1)) | (t == -1)).all()), name


@pytest.mark.gpu
def test_screen_fields_do_not_change_with_lddt_on(screen_models):
    """lDDT draws nothing and steers nothing: every field the screen returns without lddt_cutoff is torch.equal in a run with it, which adds exactly the six new
    fields, fp32 in [0, 1] or -1; the statistics are those of `screen._scored_mean_std` on the per-re-dock fields."""
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    kw = dict(screen_workers.SCREEN)
    P, k, D, n = kw['num_poses'], kw['screened_per_pose'], kw['redocks_per_design'], int(one['generate_flag'].sum())
    plain = screen.optimize_antibody(dock, design, one, poses_per_launch=2, **kw)
    on = screen.optimize_antibody(dock, design, one, poses_per_launch=2, **kw, **LDDT)
    assert set(on) == set(plain) | NEW and not set(plain) & NEW
    for name, v in plain.items():
        assert torch.equal(on[name], v), name
    _shapes(on, P, k, D, n)
    assert (on['redock_lddt'] >= 0).all() and (on['redock_consistency'] >= 0).all()               # 12 re-docked residues in a 128-residue complex: pairs everywhere
    m, s = screen._scored_mean_std(on['redock_lddt'], -1)
    assert torch.equal(on['lddt_mean'], m) and torch.equal(on['lddt_std'], s)
    assert torch.equal(on['lddt_res_mean'], screen._scored_mean_std(on['redock_lddt_res'], 2)[0])
    assert screen.screen_filter(on, min_lddt=0.0).equal(screen.screen_filter(plain)) and not screen.screen_filter(on, min_lddt=1.01).any()


@pytest.mark.gpu
def test_screen_lddt_equals_the_public_calls(screen_models):
    """The new fields of a screen with all poses in one launch against the same stages written out with the public calls (tests/scorer_harness.py:
    stages) and scored by sampler.lddt_scores / sampler.lddt_consistency with rows = the re-docked residues, and design by design by single-group hip calls."""
    from ab_opt_amd import geometry, hip, sampler
    from scorer_harness import stages as _stages
    P, S, k, D, contig, seed = 4, 3, 2, 3, '33-39', 5
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    L = one['aa'].shape[1]
    gen = one['generate_flag'][0].bool()
    n = int(gen.sum())
    res = screen.optimize_antibody(dock, design, one, P, S, D, contig=contig, screened_per_pose=k, seed=seed, poses_per_launch=P, screen_by='ppl', **LDDT)
    _, _, rpos, rmask = _stages(dock, design, one, P, S, k, D, contig, seed)
    # the design complexes: stage 2 of _stages once more, as far as the chosen designs' coordinates
    rep = lambda t, m: t.expand(m, *t.shape[1:]).contiguous()
    t1 = sampler.sample_replicated(dock, one, P, dict(sample_structure=True, sample_sequence=False, seed=screen.stage_seed(seed, 'dock'), rng_offset=0))[0]
    g1 = rep(gen[None], P)
    pose_pos, pose_mask = geometry.reconstruct_backbone_partially(rep(one['pos_heavyatom'], P), hip.so3_exp(t1[0]), t1[1], torch.where(g1, t1[2], rep(one['aa'], P)),
                                                                  rep(one['chain_nb'], P), rep(one['res_nb'], P), rep(one['mask_heavyatom'], P), g1)
    from ab_opt_amd.model import generate_mask_from_str
    dflag = gen & generate_mask_from_str(contig, gen)
    cx = [dict(one, pos_heavyatom=pose_pos[i:i + 1], mask_heavyatom=pose_mask[i:i + 1], generate_flag=dflag[None]) for i in range(P)]
    t2 = sampler.sample_grouped(design, cx, S, dict(sample_structure=False, sample_sequence=True, seed=screen.stage_seed(seed, 'design'), rng_offset=0))[0]
    g2 = rep(dflag[None], P * S)
    des_pos, des_mask = geometry.reconstruct_backbone_partially(pose_pos.repeat_interleave(S, 0), hip.so3_exp(t2[0]), t2[1], torch.where(g2, t2[2], rep(one['aa'], P * S)),
                                                                rep(one['chain_nb'], P * S), rep(one['res_nb'], P * S), pose_mask.repeat_interleave(S, 0), g2)
    pick = (torch.arange(P, device=DEV)[:, None] * S + res['chosen']).reshape(-1)
    npos, nmask = des_pos[pick], des_mask[pick]
    sc = sampler.lddt_scores(rpos, rmask, npos, nmask, rows=gen, cutoff=LDDT['lddt_cutoff'])
    assert torch.equal(res['redock_lddt'], sc['lddt'].view(P, k, D))
    assert torch.equal(res['redock_lddt_res'], sc['lddt_res'][:, gen].view(P, k, D, n))
    assert (sc['den'][:, ~gen] == 0).all() and (sc['den'][:, gen] > 0).all()
    co = sampler.lddt_consistency(rpos, rmask, D, rows=gen, cutoff=LDDT['lddt_cutoff'])
    assert torch.equal(res['redock_consistency'], co['consistency'].view(P, k, D))
    rows = gen[None]
    for i in range(P * k):
        sl = slice(i * D, (i + 1) * D)
        alone = hip.lddt_ca_grouped(rpos[sl], rmask[sl], npos[i:i + 1], nmask[i:i + 1], rows=rows, cutoff=LDDT['lddt_cutoff'])
        assert torch.equal(res['redock_lddt'].view(P * k, D)[i], alone['lddt']), i
        ens = hip.lddt_ca_ensemble(rpos[sl], rmask[sl], D, rows=rows, cutoff=LDDT['lddt_cutoff'])
        assert torch.equal(res['redock_consistency'].view(P * k, D)[i], ens['consistency'][0]), i
    # the interface form of the public call: only pairs across antibody / antigen
    iface = sampler.lddt_scores(rpos, rmask, npos, nmask, rows=gen, fragment_type=one['fragment_type'][0], interface=True)
    grp = screen.chain_groups(one['fragment_type']).expand(P * k, L)
    direct = hip.lddt_ca_grouped(rpos, rmask, npos, nmask, rows=gen[None].expand(P * k, L), group=grp)
    assert torch.equal(iface['num'], direct['num']) and torch.equal(iface['den'], direct['den']) and (iface['den'] <= sc['den']).all()


@pytest.mark.gpu
def test_screen_lddt_does_not_depend_on_poses_per_launch(monkeypatch, screen_models):
    """The screen with lDDT on, with all, 1 and 2 poses per launch: every field, the six new ones included, bit for bit -- ABOPT_PAIR_TERMS=0 /
    ABOPT_CORE_NO_SPLIT=1 pin one arithmetic form of the denoiser, as DESIGN.md section 6.1 prescribes and tests/test_screen.py does."""
    monkeypatch.setenv('ABOPT_PAIR_TERMS', '0')
    monkeypatch.setenv('ABOPT_CORE_NO_SPLIT', '1')
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    kw = dict(screen_workers.SCREEN)
    runs = [screen.optimize_antibody(dock, design, one, poses_per_launch=n, **kw, **LDDT) for n in (kw['num_poses'], 1, 2)]
    assert NEW <= set(runs[0])
    for r in runs[1:]:
        assert set(r) == set(runs[0])
        for name, v in runs[0].items():
            assert torch.equal(r[name], v), name


@pytest.mark.gpu
def test_screen_lddt_with_share_redocks_and_with_cluster_cutoff(monkeypatch, screen_models):
    """cluster_cutoff: the new fields have the C cluster centres as their leading dimension, like dockq.  share_redocks (with allowed types that leave duplicates
    among the chosen designs): the shapes stay; redock_consistency is per unit -- every owner of a unit holds the unit's row, like redock_score; every other
    field is what the run without lddt_cutoff returns; and the whole result, the per-owner versus-design fields included, is that of a run with another
    poses_per_launch (other launches, the same owners)."""
    monkeypatch.setenv('ABOPT_PAIR_TERMS', '0')
    monkeypatch.setenv('ABOPT_CORE_NO_SPLIT', '1')
    from sequence_cluster_workers import allowed
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    kw = dict(screen_workers.SCREEN)
    P, k, D, n = kw['num_poses'], kw['screened_per_pose'], kw['redocks_per_design'], int(one['generate_flag'].sum())
    res = screen.optimize_antibody(dock, design, one, poses_per_launch=2, cluster_cutoff=0.0, max_clusters=3, **kw, **LDDT)
    C = int(res['cluster_centre'].numel())
    assert C == 3 and res['dockq'].shape[0] == C
    _shapes(res, C, k, D, n)
    extra = dict(seq_mismatch=0, share_redocks=True, allowed_aa=allowed(DEV))
    shared = screen.optimize_antibody(dock, design, one, poses_per_launch=P * k, **kw, **extra, **LDDT)
    _shapes(shared, P, k, D, n)
    unit = shared['design_unit'].reshape(-1)
    U = int(shared['unit_owner'].numel())
    assert U < P * k, 'the allowed types leave duplicates: some unit has several owners'
    cons, score = shared['redock_consistency'].view(P * k, D), shared['redock_score'].view(P * k, D)
    for u in range(U):
        own = (unit == u).nonzero().flatten()
        assert (cons[own] == cons[own[0]]).all() and (score[own] == score[own[0]]).all(), u
    without = screen.optimize_antibody(dock, design, one, poses_per_launch=P * k, **kw, **extra)
    for name, v in without.items():
        assert torch.equal(shared[name], v), name
    again = screen.optimize_antibody(dock, design, one, poses_per_launch=2, **kw, **extra, **LDDT)
    for name, v in shared.items():
        assert torch.equal(again[name], v), name


@pytest.mark.gpu
def test_two_rank_screen_gathers_the_lddt_fields(tmp_path, monkeypatch, screen_models):
    """Two gloo ranks sharing cuda:0 (5 poses split 3 + 2, two per launch) return what one process returns, the six new fields included, bit for bit -- plainly and
    with share_redocks, where the versus-design fields travel per owner and redock_consistency per unit."""
    from scorer_harness import spawn2 as _spawn2
    monkeypatch.setenv('ABOPT_PAIR_TERMS', '0')
    monkeypatch.setenv('ABOPT_CORE_NO_SPLIT', '1')
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    kw = dict(screen_workers.SCREEN)
    ref = {tag: screen.optimize_antibody(dock, design, one, poses_per_launch=kw['num_poses'], **kw, **LDDT, **extra(DEV)) for tag, extra in lddt_workers.RUNS.items()}
    _spawn2(lddt_workers.lddt_screen_worker, tmp_path)
    for tag, want_ in ref.items():
        assert NEW <= set(want_)
        for r in range(2):
            got = torch.load(tmp_path / f'lddt_{tag}_{r}.pt')
            assert set(got) == set(want_), (tag, r)
            for name, v in want_.items():
                assert torch.equal(got[name], v.cpu()), (tag, r, name)
