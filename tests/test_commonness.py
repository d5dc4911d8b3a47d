"""Commonness (abopt_commonness_score / abopt_commonness_score_grouped, csrc/denoise.hip: commonness_kernel) against its statement in numpy / float64 on the fp32
inputs:

    score[b] = sum over b' of sqrt(mean_n |x_b - x_b'|^2) / (B - 1)

at the wave edges of the kernel: B below, at and one past the four waves of a workgroup (a wave takes b' = wave, wave + 4, ...), 3 n below, around and above the
64 lanes of a wave (a lane takes k = lane, lane + 64, ... of the 3 n coordinates).

The bound (u = 2^-24; `bound`).  The kernel is fp32 throughout.  For one pair: every difference d is rounded once, which counts twice after squaring; a lane
adds its ceil(3 n / 64) squares with one fma each, so a square passes through at most that many roundings; wave_sum (csrc/abopt_common.h) adds across the wave in
six steps (permlane32 swap, permlane16 swap, four row rotations), one rounding each.  That is (8 + ceil(3 n / 64)) u relative on the sum of squares.  The division
by n and the square root are correctly rounded: the root halves what came before and the two add u / 2 + u.  A wave then adds its ceil(B / 4) distances (a term
passes through at most that many roundings), the four waves' sums take three more adds and the division by B - 1 one.  All terms are >= 0, so relative errors
carry through the sums:

    |score - score64| <= ((8 + ceil(3 n / 64)) / 2 + 1.5 + ceil(B / 4) + 4) u x 1.001 x score64        (1.001: the second-order terms)

about 4.5e-6 at B = 257, n = 50."""
import functools
import math

import numpy as np
import pytest
import torch

import scorer_harness as harness

DEV = torch.device('cuda:0')
U = 2.0 ** -24
FAR = np.array([900.0, -700.0, 1100.0])
SHAPES = [(B, n) for B in (2, 3, 4, 5, 7, 64, 65, 257) for n in (1, 21, 22, 50)] + [(5, 300)]           # 3 n = 63 and 66 straddle a wave
GROUPED = [(G, S, n) for G in (1, 3) for S in (2, 5, 65) for n in (1, 21, 22, 50)]


# ------------------------------------------------------------------------------------------ the statement, the bound and the inputs
def commonness_f64(x):
    x = np.asarray(x, dtype=np.float64)
    d = x[:, None] - x[None]
    return np.sqrt((d * d).sum((2, 3)) / x.shape[1]).sum(1) / (x.shape[0] - 1)


def bound(B, n):
    """the relative bound of the module docstring"""
    return ((8 + math.ceil(3 * n / 64)) / 2 + 1.5 + math.ceil(B / 4) + 4) * U * 1.001


def _raw_structures(B, n, seed, far=True):
    """Clustered structures (5 centres, normal x 8 A; jitter with sigma from {0.3, 1.0, 2.5} A) as fp32.  With `far`, from B = 5 on, structure B - 2 is
    structure 1 translated by (900, -700, 1100) A; from B = 64 on, structure B - 1 is an exact duplicate of structure 0.  The far copy puts a term of about
    1600 / (B - 1) A into every score, next to which the ordinary distances (about 10 A) weigh little under a relative bound: every shape is therefore
    evaluated a second time without it (far=False), where the bound bears on the ordinary distances alone."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(5, n, 3)) * 8.0
    which = rng.integers(0, 5, size=B)
    sigma = rng.choice([0.3, 1.0, 2.5], size=B)
    x = (centres[which] + rng.normal(size=(B, n, 3)) * sigma[:, None, None]).astype(np.float32)
    if far and B >= 5:
        x[B - 2] = (x[1].astype(np.float64) + FAR).astype(np.float32)
    if B >= 64:
        x[B - 1] = x[0]
    return x


def separated_pairs(ref, B, n):
    """ref sorted -> (order, flags): adjacent entries of the float64 order whose scores are further apart than twice the bound (of the larger one)"""
    order = np.argsort(ref, kind='stable')
    s = ref[order]
    return order, np.diff(s) > 2 * bound(B, n) * s[1:]


@functools.lru_cache(maxsize=None)
def case(B, n, far=True):
    """(x [B, n, 3] fp32 numpy, float64 scores), built once per shape and left unchanged: the first seed whose float64 scores leave at least 90 % of the adjacent
    pairs of their order further apart than twice the bound (B >= 3; the two scores of B = 2 are one number).  A condition on the inputs, not on the code."""
    for seed in range(100):
        x = _raw_structures(B, n, 1000 * seed + 7 * B + n, far)
        ref = commonness_f64(x)
        if B == 2 or separated_pairs(ref, B, n)[1].mean() >= 0.9:
            break
    assert B == 2 or separated_pairs(ref, B, n)[1].mean() >= 0.9, (B, n, far)
    return x, ref


def grouped_case(G, S, n):
    x = np.concatenate([_raw_structures(S, n, 5000 + 100 * g + 7 * S + n) for g in range(G)])
    return x, np.concatenate([commonness_f64(x[g * S:(g + 1) * S]) for g in range(G)])


def _assert_within_bound(got, ref, B, n, tag):
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    ratio = (err / (bound(B, n) * ref)).max()
    print('commonness', tag, 'worst error / bound: %.3f' % ratio)
    assert (err <= bound(B, n) * ref).all(), (tag, ratio)
    return ratio


# ------------------------------------------------------------------------------------------ CPU
def test_statement_on_a_hand_worked_example_and_the_input_conditions():
    """Three points on a line (n = 1): distances 1, 3, 2 -> scores (1 + 3) / 2, (1 + 2) / 2, (3 + 2) / 2.  Every shape's inputs leave 90 % of the adjacent pairs of
    the float64 order separated, hold the far copy and the duplicate, and the bound is the docstring's number at the largest shape."""
    x = np.array([0.0, 1.0, 3.0]).reshape(3, 1, 1) * np.array([1.0, 0.0, 0.0])
    assert commonness_f64(x).tolist() == [2.0, 1.5, 2.5]
    assert abs(bound(257, 50) - 4.5e-6) < 0.1e-6
    for B, n in SHAPES:
        x, ref = case(B, n)
        near, ref_near = case(B, n, False)
        assert x.dtype == np.float32 and x.shape == (B, n, 3) and np.isfinite(ref).all() and (ref > 0).all()
        assert near.dtype == np.float32 and near.shape == (B, n, 3) and np.abs(near).max() < 100.0 and (ref_near > 0).all()
        if B >= 5:
            assert np.abs(x[B - 2] - x[1] - FAR).max() < 1e-3 and ref.min() > 1000.0 / (B - 1)
        if B >= 64:
            assert np.array_equal(x[B - 1], x[0]) and ref[B - 1] == ref[0]


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_scores_match_the_float64_statement_within_the_derived_bound():
    """Every score of every shape, with and without the far copy, within the bound of the module docstring, and the order of the scores equal to the float64 order over the adjacent pairs that
    are further apart than twice the bound (at least 90 % of them, by the choice of the inputs).  B = 2: the two scores are the same bits (one distance)."""
    from ab_opt_amd import hip
    worst = 0.0
    for B, n, far in [(B, n, far) for B, n in SHAPES for far in (True, False)]:
        x, ref = case(B, n, far)
        got = hip.commonness_score(torch.from_numpy(x).to(DEV))
        assert got.shape == (B,) and got.dtype == torch.float32
        worst = max(worst, _assert_within_bound(got, ref, B, n, (B, n, 'far' if far else 'near')))
        g = got.cpu().numpy()
        if B == 2:
            assert g[0] == g[1]
            continue
        order, sep = separated_pairs(ref, B, n)
        assert sep.mean() >= 0.9, (B, n, far)
        assert (g[order[1:]][sep] > g[order[:-1]][sep]).all(), (B, n, far)
        if B >= 64:
            assert g[0] == g[B - 1], (B, n)                            # the duplicate: the same distances in the same order
    print('commonness: worst error / bound over all shapes: %.3f' % worst)


@pytest.mark.gpu
def test_duplicates_have_a_pair_distance_of_exactly_zero():
    """B = 2 duplicates score exactly 0.  B = 3 with structures 0 and 1 equal and structure 2 at distance d: the scores are d / 2, d / 2 and (d + d) / 2 = d, so
    score[2] is exactly twice score[0] only if the duplicates' distance is exactly 0.  The same through the grouped entry."""
    from ab_opt_amd import hip
    for n in (1, 21, 22, 50):
        x, _ = case(3, n)
        x = x.copy()
        x[1] = x[0]
        xd = torch.from_numpy(x).to(DEV)
        assert hip.commonness_score(xd[:2]).tolist() == [0.0, 0.0]
        s = hip.commonness_score(xd)
        assert s[0] == s[1] and s[2] == 2 * s[0] and s[0] > 0, (n, s)
        assert hip.commonness_score_grouped(xd[:2], 2).tolist() == [0.0, 0.0]
        assert torch.equal(hip.commonness_score_grouped(xd, 3), s)


@pytest.mark.gpu
def test_grouped_scores_match_the_statement_and_the_per_group_calls():
    """G in {1, 3} groups of S in {2, 5, 65}: every score within the bound of its group's statement (B = S), and the grouped call equal to the per-group calls of
    abopt_commonness_score bit for bit."""
    from ab_opt_amd import hip
    for G, S, n in GROUPED:
        x, ref = grouped_case(G, S, n)
        xd = torch.from_numpy(x).to(DEV)
        got = hip.commonness_score_grouped(xd, S)
        assert got.shape == (G * S,)
        _assert_within_bound(got, ref, S, n, ('grouped', G, S, n))
        harness.grouped_equals_per_group(lambda structs: dict(score=hip.commonness_score_grouped(structs, S)), [((G, S, n), G, S, dict(structs=xd))], set())
        for g in range(G):
            assert torch.equal(got[g * S:(g + 1) * S], hip.commonness_score(xd[g * S:(g + 1) * S])), (G, S, n, g)


@pytest.mark.gpu
def test_a_nan_coordinate_sits_where_the_statement_has_it():
    """One NaN coordinate in one structure: the call returns, every score of that structure's group is NaN (each one sums a distance to it) and, in the grouped
    call, the other groups keep their bits."""
    from ab_opt_amd import hip
    for B, n in ((3, 1), (5, 22), (65, 50)):
        x, _ = case(B, n)
        x = x.copy()
        x[B // 2, n - 1, 1] = np.nan
        ref = commonness_f64(x)
        got = hip.commonness_score(torch.from_numpy(x).to(DEV)).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).all(), (B, n)
    G, S, n = 3, 5, 22
    x, _ = grouped_case(G, S, n)
    clean = hip.commonness_score_grouped(torch.from_numpy(x).to(DEV), S)
    x = x.copy()
    x[S + 2, 0, 2] = np.nan
    ref = np.concatenate([commonness_f64(x[g * S:(g + 1) * S]) for g in range(G)])
    got = hip.commonness_score_grouped(torch.from_numpy(x).to(DEV), S)
    assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(ref)) and np.isnan(ref).sum() == S
    assert torch.equal(got[:S], clean[:S]) and torch.equal(got[2 * S:], clean[2 * S:])


@pytest.mark.gpu
def test_calls_are_capturable_and_repeatable():
    """Each entry recorded with torch.cuda.graph (one launch) and replayed on OTHER structures copied into the static input gives what the eager call gives on
    them; five repeat calls are bit-identical."""
    from ab_opt_amd import hip
    B, n = 65, 22
    a, ref = case(B, n)
    b = _raw_structures(B, n, 4242)
    for call in (lambda structs: dict(score=hip.commonness_score(structs)), lambda structs: dict(score=hip.commonness_score_grouped(structs, 5))):
        first, held = harness.capture_replays_on_other_inputs(call, dict(structs=torch.from_numpy(a).to(DEV)), dict(structs=torch.from_numpy(b).to(DEV)))
        assert torch.equal(first['score'], call(torch.from_numpy(a).to(DEV))['score'])
        assert not torch.equal(first['score'], held['score'])
    xd = torch.from_numpy(a).to(DEV)
    runs = [hip.commonness_score(xd) for _ in range(5)] + [hip.commonness_score_grouped(xd, 13) for _ in range(5)]
    assert all(torch.equal(r, runs[0]) for r in runs[1:5]) and all(torch.equal(r, runs[5]) for r in runs[6:])
    _assert_within_bound(runs[0], ref, B, n, 'repeat')


@pytest.mark.gpu
def test_one_structure_is_refused_before_any_launch():
    """B = 1 and S = 1 (a mean over no peers), n = 0 and a NULL pointer through the C entries: ABOPT_EINVAL, and `score` keeps the pattern it was filled with.
    hip.commonness_score_grouped raises for S = 1 without a device call."""
    from ab_opt_amd import hip
    L_ = hip.lib()
    x = torch.from_numpy(case(5, 21)[0]).to(DEV)
    score = torch.full((5,), 77.0, device=DEV)
    assert L_.abopt_commonness_score(hip.ptr(x), hip.ptr(score), 1, 21, hip.stream()) == 1 and 'B=1' in L_.abopt_last_error().decode()
    assert L_.abopt_commonness_score(hip.ptr(x), hip.ptr(score), 5, 0, hip.stream()) == 1
    assert L_.abopt_commonness_score(None, hip.ptr(score), 5, 21, hip.stream()) == 1
    assert L_.abopt_commonness_score(hip.ptr(x), None, 5, 21, hip.stream()) == 1
    assert L_.abopt_commonness_score_grouped(hip.ptr(x), hip.ptr(score), 5, 1, 21, hip.stream()) == 1 and 'S=1' in L_.abopt_last_error().decode()
    assert L_.abopt_commonness_score_grouped(hip.ptr(x), hip.ptr(score), -1, 5, 21, hip.stream()) == 1
    assert L_.abopt_commonness_score_grouped(hip.ptr(x), hip.ptr(score), 1, 5, 0, hip.stream()) == 1
    assert L_.abopt_commonness_score_grouped(hip.ptr(x), hip.ptr(score), 0, 5, 21, hip.stream()) == 0         # no groups: a no-op
    torch.cuda.synchronize()
    assert (score == 77.0).all()
    with pytest.raises(ValueError, match='whole groups'):
        hip.commonness_score_grouped(x, 1)
    with pytest.raises(RuntimeError, match='abopt error 1'):
        hip.commonness_score(x[:1])
    assert L_.abopt_commonness_score(hip.ptr(x), hip.ptr(score), 5, 21, hip.stream()) == 0                     # ... and a good call fills the same buffer
    torch.cuda.synchronize()
    assert (score != 77.0).all()
