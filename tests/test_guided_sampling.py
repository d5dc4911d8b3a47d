"""Guided sampling (include/abopt.h: abopt_guide_positions, ABI 56): after every reverse step the generated residues are pulled towards
the hotspot residues and pushed out of the repellers' radius.

The float64 statement of the definition and the kernel cases live in tests/guide_statement.py.  The CPU tests cover the statement on hand cases, the validation,
the C entry's refusals, the way the knobs reach the loop's spec and the roles reach the batch; the GPU tests hold the kernel to the statement and to its contract
(bits outside the moved rows, p_norm, the cap, shared roles, capture), and whole guided loops to the step entry driven by hand, to their replays, and through the
model, the samplers and the screen.

Tolerance of the kernel against the statement, in units of 2^-23 max |coordinate| of the case: four times the worst error measured on one MI355X (MEASURED below;
DESIGN.md section 3.12 lists the values), separately for the cases at the origin and for the same cases moved by (900, -700, 500) A."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

import guide_statement as gs
import screen_workers
import step_harness
from conftest import build_model
from ab_opt_amd import hip, model as model_, sampler, screen
from ab_opt_amd.dpm import FullDPM, _LoopSpec, _graph_key
from ab_opt_amd.utils import synth

DEV = torch.device('cuda:0')
MEAN, SCALE = (1.5, -2.0, 0.5), 10.0
# worst |device - float64 statement| / (2^-23 max |coordinate|) over the cases, measured on one MI355X: at the origin 0.288 (max |coordinate| 2.9 .. 117 A; worst
# absolute error 4.0e-6 A, at L = 1100) and moved by (900, -700, 500) A 0.544 (max |coordinate| 902 .. 991 A; worst absolute error 6.1e-5 A, at (5, 130)): below one
# ulp of the coordinates either way, most of it the rounding of the stored sum p + shift
MEASURED = {'origin': 0.2884, 'moved': 0.5440}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
PLACES = {'origin': (0.0, 0.0, 0.0), 'moved': gs.OFFSET}
GUIDE = dict(guide_attract=0.5, guide_attract_radius=2.0, guide_repel=0.5, guide_repel_radius=6.0, guide_max_shift=2.0)


@functools.lru_cache(maxsize=None)
def _case(N, L, place):
    """(inputs, float64 statement) of a kernel case: computed once, shared, never changed"""
    c = gs.case(N, L, PLACES[place])
    return c, gs.statement(c['p'], c['gen'], c['res'], c['role'], c['w_att'], c['r_att'], c['w_rep'], c['r_rep'], c['max_shift'])


# ------------------------------------------------------------------------------------------ CPU: the statement
def _one(p, gen, role, res=None, **kw):
    p = np.asarray(p, dtype=np.float64)[None]
    gen, role = np.asarray(gen, bool)[None], np.asarray(role, np.int32)[None]
    res = np.ones_like(gen) if res is None else np.asarray(res, bool)[None]
    args = dict(w_att=0.0, r_att=8.0, w_rep=0.0, r_rep=3.0, max_shift=1e9)
    args.update(kw)
    return gs.statement(p, gen, res, role, **args)


def test_statement_on_hand_cases():
    # one moved row, one repeller at d < r_rep, w_rep = 1: the row ends at distance r_rep from it, along the line that joins them
    st = _one([[1.0, 2.0, 2.0], [0.0, 0.0, 0.0]], [True, False], [0, gs.REP], w_rep=1.0, r_rep=5.0)
    assert abs(np.linalg.norm(st['p'][0, 0]) - 5.0) < 1e-12 and np.allclose(st['p'][0, 0], np.array([1.0, 2.0, 2.0]) * 5.0 / 3.0)
    assert np.array_equal(st['p'][0, 1], [0.0, 0.0, 0.0])
    # ... and one beyond r_rep is left alone
    st = _one([[3.0, 4.0, 0.0], [0.0, 0.0, 0.0]], [True, False], [0, gs.REP], w_rep=1.0, r_rep=5.0)
    assert not st['written'].any()
    # w_att = 1, no repulsion, a huge cap: the new centroid distance is min(D, r_att)
    rng = np.random.default_rng(4)
    p = rng.normal(size=(12, 3)) * 4.0
    p[8:] += np.array([7.0, -3.0, 2.0])
    gen = np.arange(12) < 5
    role = np.where(np.arange(12) >= 8, gs.HOT, 0)
    D = np.linalg.norm(p[role == gs.HOT].mean(0) - p[gen].mean(0))
    for r_att in (5.0, D + 1.0):
        st = _one(p, gen, role, w_att=1.0, r_att=r_att)
        new = np.linalg.norm(st['p'][0, role == gs.HOT].mean(0) - st['p'][0, gen].mean(0))
        print(f'centroid distance {D:.4f} -> {new:.4f} at r_att {r_att:.4f}')
        assert abs(new - min(D, r_att)) < 1e-12 and np.array_equal(st['p'][0, ~gen], p[~gen])
    assert D > 5.0
    # the pull is rigid: every moved row gets the same shift
    st = _one(p, gen, role, w_att=0.3, r_att=1.0)
    assert np.allclose(st['shift'][0, gen], st['shift'][0, 0]) and np.abs(st['shift'][0, 0]).max() > 0
    # an empty H, R or M: no shift; bits on generated or absent rows are ignored; a coincident pair contributes 0
    both = gs.HOT | gs.REP
    assert not _one(p, gen, np.zeros(12), w_att=1.0, w_rep=1.0, r_rep=50.0)['written'].any()
    assert not _one(p, np.zeros(12, bool), np.full(12, both), w_att=1.0, w_rep=1.0, r_rep=50.0)['written'].any()
    assert not _one(p, gen, np.where(gen, both, 0), w_att=1.0, w_rep=1.0, r_rep=50.0)['written'].any()
    assert not _one(p, gen, np.where(gen, 0, both), res=gen, w_att=1.0, w_rep=1.0, r_rep=50.0)['written'].any()
    assert not _one([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]], [True, False], [0, gs.REP], w_rep=1.0, r_rep=5.0)['written'].any()
    # the cap: direction kept, length max_shift
    free = _one(p, gen, np.where(gen, 0, both), w_att=0.9, r_att=0.5, w_rep=1.0, r_rep=6.0)
    capped = _one(p, gen, np.where(gen, 0, both), w_att=0.9, r_att=0.5, w_rep=1.0, r_rep=6.0, max_shift=0.25)
    n_free, n_cap = np.linalg.norm(free['shift'][0, gen], axis=1), np.linalg.norm(capped['shift'][0, gen], axis=1)
    assert (n_free > 0.25).all() and np.allclose(n_cap, 0.25) and np.allclose(capped['shift'][0, gen] * n_free[:, None], free['shift'][0, gen] * 0.25)


def test_the_kernel_cases_exercise_what_they_claim():
    """The conditions of the GPU comparison, on the statement alone: no moved row within 0.1 A of a repeller; in every case with L >= 63 at least 5 % of the moved
    rows capped, 20 % moving below the cap and 40 % repelled; pooled over those cases 40 % attracted; a sample without hotspots per case with N >= 2, a case without
    repellers, a sample without generated rows, a generated mask that is not a prefix, an absent row from L = 7 on, and more than one repeller tile at L = 1100."""
    pooled = [0, 0.0]
    for N, L in gs.CASES:
        c, st = _case(N, L, 'origin')
        sh = gs.shares(c, st)
        print((N, L), {k: round(v, 3) for k, v in sh.items()}, f'closest pair {st["dmin"]:.3f} A')
        assert st['dmin'] >= 0.1
        if L >= 63:
            assert sh['capped'] >= 0.05 and sh['free'] >= 0.20 and sh['repelled'] >= 0.40, (N, L, sh)
            pooled[0] += sh['moved']
            pooled[1] += sh['attracted'] * sh['moved']
        ctx = c['res'] & ~c['gen']
        if N >= 2:
            assert not (ctx[N - 1] & ((c['role'][N - 1] & gs.HOT) != 0)).any()
        if L >= 7:
            assert (~c['res']).sum(1).min() == 1 and not c['gen'][:, 0].any()
        if L >= 63:
            assert c['gen'][[n for n in range(N) if (N, L, n) != (5, 130, 3)], 10].all()
            assert (c['role'][c['gen']] != 0).any() and (c['role'][~c['res']] != 0).any()       # bits that must be ignored are there
    assert pooled[1] / pooled[0] >= 0.40
    assert not (_case(*gs.R_EMPTY_CASE, 'origin')[0]['role'] & gs.REP).any() and not _case(5, 130, 'origin')[0]['gen'][3].any()
    big = _case(1, 1100, 'origin')[0]
    rep = big['res'][0] & ~big['gen'][0] & ((big['role'][0] & gs.REP) != 0)
    assert rep[:1024].any() and rep[1024:].any()


# ------------------------------------------------------------------------------------------ CPU: validation, the spec, the roles
def test_guidance_knobs_are_validated_without_a_device():
    kn = hip.check_guidance()
    assert kn == dict(guide_attract=0.0, guide_attract_radius=8.0, guide_repel=0.0, guide_repel_radius=3.0, guide_max_shift=2.0, guide_decay=0)
    assert hip.check_guidance(guide_attract=1, guide_decay='quadratic')['guide_decay'] == 2 and hip.check_guidance(guide_decay='linear')['guide_decay'] == 1
    assert all(isinstance(v, float) for k, v in hip.check_guidance(guide_attract=1, guide_repel=3).items() if k != 'guide_decay')
    for name in ('guide_attract', 'guide_attract_radius', 'guide_repel', 'guide_repel_radius', 'guide_max_shift'):
        for bad in (-0.5, -1e-9, float('nan'), float('inf'), -float('inf')):
            with pytest.raises(ValueError, match=f'{name} must be finite and >= 0'):
                hip.check_guidance(**{name: bad})
    with pytest.raises(ValueError, match='guide_attract must be <= 1'):
        hip.check_guidance(guide_attract=1.0 + 1e-9)
    with pytest.raises(ValueError, match='guide_max_shift must be > 0'):
        hip.check_guidance(guide_max_shift=0)
    for bad in ('cubic', '', 3, -1, True, 1.5):
        with pytest.raises(ValueError, match='guide_decay'):
            hip.check_guidance(guide_decay=bad)
    assert hip.guide_weight(0, 100, 1) == 0.0 and hip.guide_weight(50, 100, 2) == 0.25 and hip.guide_weight(0, 100, 0) == 1.0 and hip.guide_weight(100, 100, 2) == 1.0
    with pytest.raises(RuntimeError, match='HIP device only'):                  # a CPU tensor is refused before anything else (the knobs here are bad too)
        hip.guide_positions(torch.zeros(1, 4, 3), None, torch.zeros(1, 4, dtype=torch.bool), torch.ones(1, 4, dtype=torch.bool), torch.zeros(1, 4, dtype=torch.int32), w_att=7)


def test_entry_refuses_bad_arguments_before_any_launch():
    """ABOPT_EINVAL (1) with a message for a NULL pointer, N % S != 0, a negative or non-finite scalar, w_att > 1, max_shift == 0; the 16-byte dummies are never
    touched by a launch (no device is needed); N = 0 and L = 0 are no-ops; p_norm may be NULL."""
    L_ = hip.lib()
    dummy = (ctypes.c_char * 16)()
    a = ctypes.c_void_p(ctypes.addressof(dummy))
    good = dict(p=a, p_norm=a, gen=a, res=a, role=a, S=0, N=0, L=8, w_att=0.5, r_att=8.0, w_rep=0.5, r_rep=3.0, max_shift=2.0, scale=10.0, mean=a)

    def call(**kw):
        g = dict(good, **kw)
        return L_.abopt_guide_positions(g['p'], g['p_norm'], g['gen'], g['res'], g['role'], g['S'], g['N'], g['L'], g['w_att'], g['r_att'], g['w_rep'], g['r_rep'],
                                        g['max_shift'], g['scale'], g['mean'], None)
    assert call() == 0 and call(p_norm=None) == 0 and call(N=4, L=0) == 0 and call(N=0, S=3) == 0
    for kw, word in ((dict(p=None), 'NULL'), (dict(gen=None), 'NULL'), (dict(res=None), 'NULL'), (dict(role=None), 'NULL'), (dict(mean=None), 'NULL'),
                     (dict(N=4, S=3), 'role_shared'), (dict(S=-1), 'role_shared'), (dict(N=-1), 'bad dims'),
                     (dict(w_att=-0.1), 'w_att'), (dict(w_att=1.5), 'w_att must be <= 1'), (dict(w_att=float('nan')), 'w_att'), (dict(r_att=float('inf')), 'r_att'),
                     (dict(w_rep=-1.0), 'w_rep'), (dict(r_rep=float('nan')), 'r_rep'), (dict(max_shift=0.0), 'max_shift must be > 0'),
                     (dict(max_shift=-2.0), 'max_shift'), (dict(scale=0.0), 'position_scale')):
        assert call(**dict(dict(N=4), **kw)) == 1, kw                                            # ABOPT_EINVAL, with N > 0: the launch is what the check precedes
        assert word in L_.abopt_last_error().decode(), (kw, L_.abopt_last_error().decode())


class _Stop(Exception):
    pass


@pytest.fixture
def spec_of(monkeypatch):
    """spec_of(lambda d: d.sample(...)) -> (the _LoopSpec, the inputs) that call hands to FullDPM._denoise; every device call before it is a fake (the style of
    tests/test_loop_spec.py)"""
    d = build_model(10, 3).diffusion
    seen, touched = [], []

    def denoise(self, spec, state, inputs, *args, **kw):
        seen.append((spec, inputs))
        raise _Stop

    def state(*a, **kw):
        touched.append(1)
        return torch.zeros(2, 8, 3), torch.zeros(2, 8, 3), torch.zeros(2, 8, dtype=torch.long)
    monkeypatch.setattr(FullDPM, '_denoise', denoise)
    for name, fake in (('lib', lambda: touched.append(1)), ('sample_init', state), ('add_noise', state), ('nonfinite_flag_reset', lambda: None)):
        monkeypatch.setattr(hip, name, fake)

    def run(call):
        with pytest.raises(_Stop):
            call(d)
        return seen.pop()
    run.d, run.touched = d, touched
    return run


def _cpu_args():
    rf, pf = torch.zeros(2, 8, 128), torch.zeros(2, 8, 8, 64)
    gen = torch.zeros(2, 8, dtype=torch.bool)
    gen[:, 2:5] = True
    return (torch.zeros(2, 8, 3), torch.zeros(2, 8, 3), torch.zeros(2, 8, dtype=torch.long)), (rf, pf, gen, torch.ones(2, 8, dtype=torch.bool))


def test_the_spec_carries_the_knobs_and_the_defaults_keep_the_graph_key(spec_of):
    state, feats = _cpu_args()
    role = torch.tensor([0, 1, 0, 0, 0, 2, 3, 1], dtype=torch.int64)
    plain, plain_in = spec_of(lambda d: d.sample(*state, *feats, seed=1))
    assert plain == _LoopSpec(10, ppl_masked=True) and not plain.guided and len(plain_in) == 4
    for kw in (dict(guide_role=role), dict(guide_role=role, guide_attract=0.0, guide_repel=0.0, guide_max_shift=5.0, guide_decay='linear'),
               dict(guide_attract=0.5, guide_repel=1.0)):
        spec, inputs = spec_of(lambda d: d.sample(*state, *feats, seed=1, **kw))
        assert spec == plain and len(inputs) == 4, kw                               # no role or no weight: today's loop, today's key
        assert _graph_key(spec, inputs, None) == _graph_key(plain, plain_in, None)
    spec, inputs = spec_of(lambda d: d.sample(*state, *feats, seed=1, guide_role=role, guide_attract=0.25, guide_repel=1.5, guide_decay='quadratic'))
    assert spec == dataclasses.replace(plain, guided=True, guide_attract=0.25, guide_attract_radius=8.0, guide_repel=1.5, guide_repel_radius=3.0,
                                       guide_max_shift=2.0, guide_decay=2)
    assert len(inputs) == 5 and inputs[4].dtype == torch.int32 and inputs[4].shape == (2, 8) and inputs[4].is_contiguous()
    assert torch.equal(inputs[4], role.to(torch.int32).expand(2, 8))
    assert _graph_key(spec, inputs, None) != _graph_key(plain, plain_in, None)
    # behind aa_allowed when both are present; optimize() the same way
    allowed = torch.full((8,), (1 << 20) - 1, dtype=torch.int32)
    spec, inputs = spec_of(lambda d: d.optimize(*state, 4, *feats, seed=1, aa_allowed=allowed, guide_role=role[None], guide_repel=0.5))
    assert spec.guided and spec.constrained and spec.optimize_mode and spec.guide_repel == 0.5 and spec.guide_attract == 0.0 and len(inputs) == 6
    assert torch.equal(inputs[5], role.to(torch.int32).expand(2, 8)) and torch.equal(inputs[4], allowed.expand(2, 8))
    # the role's contents are data, not key
    other, inputs2 = spec_of(lambda d: d.optimize(*state, 4, *feats, seed=1, aa_allowed=allowed, guide_role=role.flip(0), guide_repel=0.5))
    assert other == spec and _graph_key(other, inputs2, None) == _graph_key(spec, inputs, None)
    for bad, err in ((torch.zeros(8), TypeError), (torch.zeros(7, dtype=torch.int32), ValueError), (torch.zeros(3, 8, dtype=torch.int32), ValueError)):
        with pytest.raises(err, match='guide_role'):
            run = spec_of.d.sample(*state, *feats, seed=1, guide_role=bad, guide_attract=0.5)
    every = [f.name for f in dataclasses.fields(_LoopSpec)]
    assert every[every.index('noise_scale') + 1:] == ['guided', 'guide_attract', 'guide_attract_radius', 'guide_repel', 'guide_repel_radius', 'guide_max_shift',
                                                      'guide_decay']
    assert all(type(f.default) in (bool, int, float) for f in dataclasses.fields(_LoopSpec) if f.name.startswith('guide'))


def test_sample_and_optimize_refuse_guidance_of_a_fixed_structure_before_any_device_call(spec_of):
    state, feats = _cpu_args()
    role = torch.ones(8, dtype=torch.int32)
    d = spec_of.d
    for call in (lambda **kw: d.sample(*state, *feats, seed=1, **kw), lambda **kw: d.optimize(*state, 4, *feats, seed=1, **kw)):
        with pytest.raises(ValueError, match='sample_structure=True'):
            call(sample_structure=False, guide_role=role, guide_attract=0.5)
        with pytest.raises(ValueError, match='guide_attract must be <= 1'):
            call(guide_role=role, guide_attract=2)
        with pytest.raises(ValueError, match='guide_decay'):
            call(guide_decay='cubic')                                               # checked even where nothing is guided
    assert not spec_of.touched                                                      # neither the library nor a kernel was asked for anything
    # ... and a role without a weight on a fixed structure is no guidance: the design stage of the screen passes one along
    spec, inputs = spec_of(lambda d_: d_.sample(*state, *feats, seed=1, sample_structure=False, guide_role=role))
    assert not spec.guided and len(inputs) == 4
    with pytest.raises(ValueError, match='never guided'):
        d._run_eager(_LoopSpec(3, sample_structure=False, guided=True, use_bias_cache=False), state, feats + (role.expand(2, 8).contiguous(),), None, 0, 0, False)


def test_guide_roles_and_pad_complex_carry_the_role():
    r = model_.guide_roles(10, hotspots=[2, 9])
    assert r.dtype == torch.int32 and r.tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 1, 0]
    mask = torch.arange(10) >= 6
    assert model_.guide_roles(10, hotspots=mask, repel=~mask).tolist() == [2] * 6 + [1] * 4
    assert model_.guide_roles(10, hotspots=torch.tensor([7]), repel=mask).tolist() == [0] * 6 + [3] + [2] * 3
    for bad in ([0], [11], [2.5]):
        with pytest.raises(ValueError, match='outside 1..10'):
            model_.guide_roles(10, hotspots=bad)
    with pytest.raises(ValueError, match='need a batch'):
        model_.guide_roles(10, repel='context')
    with pytest.raises(ValueError, match='bool mask'):
        model_.guide_roles(10, repel=torch.zeros(9, dtype=torch.bool))
    batch = synth.make_batch(2, synth.LAYOUT_128, seed=1, lengths=[32, 27])
    ctx = model_.guide_roles(batch, hotspots=[30, 31], repel='context')
    assert ctx.shape == batch['aa'].shape and ctx.dtype == torch.int32
    assert torch.equal((ctx & 2) != 0, batch['mask'] & ~batch['generate_flag']) and torch.equal((ctx & 1) != 0, ((torch.arange(32) == 29) | (torch.arange(32) == 30)).expand(2, 32))
    whole = synth.make_batch(1, synth.LAYOUT_128, seed=1)
    ant = model_.guide_roles(whole, repel='antigen')
    assert torch.equal(ant != 0, whole['fragment_type'] == 3) and int(ant.max()) == 2
    one = {k: v[:1] for k, v in batch.items()}
    one['guide_role'] = ctx[:1]
    padded = sampler.pad_complex(one, 40)
    assert padded['guide_role'].shape == (1, 40) and padded['guide_role'].dtype == torch.int32
    assert torch.equal(padded['guide_role'][:, :32], ctx[:1]) and not padded['guide_role'][:, 32:].any()


# ------------------------------------------------------------------------------------------ GPU: the kernel
def _normalised(p):
    """(p - mean) / scale as FullDPM._run_eager forms it in torch fp32: a subtraction and a true division by a tensor (a Python scalar divisor would be turned into a
    multiplication by its reciprocal)"""
    return (p - torch.tensor(MEAN, device=DEV)) / torch.tensor(SCALE, device=DEV)


def _t(c):
    """the device tensors of a case: p, its normalised copy, the masks, the role"""
    p = torch.tensor(c['p'], dtype=torch.float32, device=DEV)
    pn = _normalised(p)
    return p, pn, torch.tensor(c['gen'], device=DEV), torch.tensor(c['res'], device=DEV), torch.tensor(c['role'], dtype=torch.int32, device=DEV)


def _guide(c, p, pn, gen, res, role, **kw):
    args = dict(w_att=c['w_att'], r_att=c['r_att'], w_rep=c['w_rep'], r_rep=c['r_rep'], max_shift=c['max_shift'], position_scale=SCALE, position_mean=MEAN)
    args.update(kw)
    return hip.guide_positions(p, pn, gen, res, role, **args)


@pytest.mark.gpu
@pytest.mark.parametrize('place', ['origin', 'moved'])
@pytest.mark.parametrize('N,L', gs.CASES)
def test_kernel_against_the_float64_statement(N, L, place):
    """Every case at both placements: the moved rows within TOL of the statement on the same fp32 inputs; every element of p and p_norm outside the rows the
    statement moves keeps its bits; p_norm == (p - mean) / scale in torch fp32, bit for bit; no shift longer than max_shift (1 + 2^-22) -- measured on the stored
    p_out - p_in, whose components carry the rounding of the sum p + shift, half an ulp of p_out each, on top; a second call on a fresh copy gives the same bits."""
    c, st = _case(N, L, place)
    p, pn, gen, res, role = _t(c)
    p0, pn0 = p.clone(), pn.clone()
    assert _guide(c, p, pn, gen, res, role) is p
    torch.cuda.synchronize()
    got, moved = p.cpu().double().numpy(), st['written']
    unit = 2.0 ** -23 * np.abs(c['p']).max()
    err = float(np.abs(got - st['p']).max())
    print(f'case {(N, L)} {place}: worst error {err:.3e} A = {err / unit:.3f} units of 2^-23 x {np.abs(c["p"]).max():.1f} A; {int(moved.sum())} rows moved')
    assert err <= TOL[place] * unit
    keep = torch.tensor(~moved, device=DEV)
    assert torch.equal(p[keep], p0[keep]) and torch.equal(pn[keep], pn0[keep])
    assert torch.equal(pn, _normalised(p))
    if moved.any():
        assert not torch.equal(p, p0)
    shift = got - c['p']
    slack = 0.5 * np.linalg.norm(np.spacing(np.abs(got).astype(np.float32)).astype(np.float64), axis=-1)
    assert (np.linalg.norm(shift, axis=-1) <= c['max_shift'] * (1.0 + 2.0 ** -22) + slack).all()
    again, pn2 = p0.clone(), pn0.clone()
    _guide(c, again, pn2, gen, res, role)
    assert torch.equal(again, p) and torch.equal(pn2, pn)


@pytest.mark.gpu
def test_kernel_contract_zero_weights_null_p_norm_shared_roles_and_capture():
    """(5, 130) and (6, 65): both weights 0 leave every bit; p_norm = NULL and p_norm given agree on p; role_shared = S equals the call on the expanded role; the call
    is capturable -- captured once, replayed twice on refreshed inputs, equal to the eager result."""
    c, st = _case(5, 130, 'origin')
    p, pn, gen, res, role = _t(c)
    p0, pn0 = p.clone(), pn.clone()
    _guide(c, p, pn, gen, res, role, w_att=0.0, w_rep=0.0)
    assert torch.equal(p, p0) and torch.equal(pn, pn0)
    _guide(c, p, pn, gen, res, role)
    bare = p0.clone()
    _guide(c, bare, None, gen, res, role)
    assert torch.equal(bare, p) and not torch.equal(p, p0)
    # shared roles: 6 samples, 3 role rows, S = 2
    c6 = gs.case(6, 65)
    p6, pn6, gen6, res6, _ = _t(c6)
    role3 = torch.tensor(gs.case(3, 65)['role'], dtype=torch.int32, device=DEV)
    full, shared = p6.clone(), p6.clone()
    _guide(c6, full, None, gen6, res6, role3.repeat_interleave(2, dim=0).contiguous())
    _guide(c6, shared, None, gen6, res6, role3, role_shared=2)
    assert torch.equal(full, shared) and not torch.equal(full, p6)
    want = gs.statement(c6['p'], c6['gen'], c6['res'], role3.cpu().numpy(), c6['w_att'], c6['r_att'], c6['w_rep'], c6['r_rep'], c6['max_shift'])['p']
    assert np.abs(shared.cpu().double().numpy() - want).max() <= TOL['origin'] * 2.0 ** -23 * np.abs(c6['p']).max()
    with pytest.raises(ValueError, match='role'):
        _guide(c6, shared, None, gen6, res6, role3, role_shared=4)
    # capture
    sp, spn = p0.clone(), pn0.clone()
    _guide(c, sp, spn, gen, res, role)                                                 # warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    sp.copy_(p0), spn.copy_(pn0)
    with torch.cuda.graph(g):
        _guide(c, sp, spn, gen, res, role)
    for _ in range(2):
        sp.copy_(p0), spn.copy_(pn0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(sp, p) and torch.equal(spn, pn)
    del g


# ------------------------------------------------------------------------------------------ GPU: the loop
def _loop_case(flavour):
    """(FullDPM, state, features) at N = 3, L = 40: the three-block AbDesign model of tests/step_harness.py (T = 3, the fused tail) or the AbDock model of
    conftest.build_model (T = 10, the unfused one), and a role word per residue"""
    d = step_harness.model() if flavour == 'abdesign' else build_model(10, 3, device=DEV).diffusion
    T = d.num_steps
    v, p, s, rf, pf, _, gen, mres = [a.to(DEV) for a in synth.eps_inputs(3, 40, [40, 33, 40], [(4, 19), (25, 31)], salt=300, num_steps=T, t=1)]
    role = torch.randint(0, 4, (3, 40), generator=torch.Generator().manual_seed(9), dtype=torch.int32).to(DEV)
    return d, (v, p * 10.0, s), (rf, pf, gen, mres), role


def _nudge(d, p, gen, mres, role, weight=1.0):
    h = d._sched_host()
    return hip.guide_positions(p.clone(), None, gen, mres, role, GUIDE['guide_attract'] * weight, GUIDE['guide_attract_radius'], GUIDE['guide_repel'] * weight,
                               GUIDE['guide_repel_radius'], GUIDE['guide_max_shift'], h['scale'], h['mean'])


@pytest.mark.gpu
@pytest.mark.parametrize('flavour', ['abdesign', 'abdock'])
def test_one_guided_step_is_the_plain_step_and_one_nudge(flavour):
    """sample(steps=1, seed=s, guide...) gives the v, s (prmsd, ppl) of the unguided call and, at t = 0, the p that hip.guide_positions makes of the unguided p, bit for
    bit; optimize(opt_step, steps=1) the same way; both weights 0, or no role, is the plain call with its last_run_info; decay 'linear' lands on u = 0 with weight 0."""
    d, state, feats, role = _loop_case(flavour)
    gen, mres = feats[2], feats[3]
    d.clear_graphs()
    for run in (lambda **kw: d.sample(*state, *feats, seed=7, steps=1, graph=False, **kw), lambda **kw: d.optimize(*state, 2, *feats, seed=7, steps=1, graph=False, **kw)):
        plain = run()
        info = dict(d.last_run_info)
        guided = run(guide_role=role, **GUIDE)
        assert d.last_run_info == dict(info, guided=True)
        assert sorted(guided) == sorted(plain) and len(plain) == 2
        top = max(plain)
        assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(plain[top], guided[top]))
        for k, (a, b) in enumerate(zip(plain[0], guided[0])):
            if k != 1:
                assert torch.equal(a.cpu(), b.cpu()), k
        assert torch.equal(guided[0][1], _nudge(d, plain[0][1], gen, mres, role)) and not torch.equal(guided[0][1], plain[0][1])
        assert torch.equal(guided[0][1][~gen], plain[0][1][~gen])
        for kw in (dict(guide_role=role), dict(guide_role=role, guide_attract=0.0, guide_repel=0.0), dict(GUIDE), dict(guide_role=role, guide_decay='linear', **GUIDE)):
            same = run(**kw)
            assert all(torch.equal(a.cpu(), b.cpu()) for t in plain for a, b in zip(plain[t], same[t])), kw
            if 'guide_decay' not in kw:
                assert d.last_run_info == info, kw


def _chain(d, state, feats, role, spec):
    """The loop `spec` by hand: one hip.eps_net_step per step with the arguments FullDPM._run_eager gives it (the chain of step_harness.steps, mixer carried from call to
    call), and hip.guide_positions on what the step stored in between.  -> [(v, p, s)] after every step."""
    rf, pf, gen, mres = feats
    N, L = mres.shape
    f32 = dict(dtype=torch.float32, device=DEV)
    pairs = d._loop_steps(spec)
    X, cdf = d._loop_tables(pairs)
    pbc = hip.pair_bias_cache(d.eps_net.encoder.packed_array(), len(d.eps_net.encoder.blocks), pf)
    pterms = hip.pair_terms(pf) if d._pair_terms_wanted(N, L, N, DEV) else None
    tiles = d._query_row_tiles(spec, gen, True)
    qrows = (*hip.query_row_list(gen), tiles) if tiles > 0 else None
    h = d._sched_host()
    v, p, s = state
    p_norm = ((p - d.position_mean) / d.position_scale).contiguous()
    net = dict(v_next=torch.empty(N, L, 3, **f32), R_next=torch.empty(N, L, 3, 3, **f32), eps_pos=torch.empty(N, L, 3, **f32), c=torch.empty(N, L, 20, **f32),
               prmsd_logits=torch.empty(N, d.num_bins, **f32) if d.abdock else None)
    res = []
    for j, (t, u) in enumerate(pairs):
        out = dict(v=torch.empty(N, L, 3, **f32), p=torch.empty(N, L, 3, **f32), s=torch.empty(N, L, dtype=torch.int64, device=DEV), p_norm=p_norm)
        if d.abdock:
            out.update(prmsd=torch.zeros(N, **f32), ppl=torch.zeros(N, **f32))
        beta = d.trans_pos.var_sched.betas[t].expand(N).contiguous()
        hip.eps_net_step(d.eps_net.packed(), v, p_norm, s, rf, pf, beta, gen, mres, d.num_bins, net, d._step_params(t, True, True, True, False, u), None, 11, 4096, p,
                         X[j], cdf[j], out, pair_bias_cache=pbc, pair_terms=pterms, carry_in=j > 0, carry_out=j + 1 < len(pairs), context_outputs_unused=True, query_rows=qrows)
        g = hip.guide_weight(u, d.num_steps, spec.guide_decay)
        hip.guide_positions(out['p'], p_norm, gen, mres, role, spec.guide_attract * g, spec.guide_attract_radius, spec.guide_repel * g, spec.guide_repel_radius,
                            spec.guide_max_shift, h['scale'], h['mean'])
        v, p, s = out['v'], out['p'], out['s']
        res.append((v, p, s))
    torch.cuda.synchronize()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize('flavour', ['abdesign', 'abdock'])
def test_guided_loop_equals_the_steps_by_hand_and_its_replays(flavour, monkeypatch):
    """Three guided steps (the whole loop of the AbDesign model, the last three of the AbDock one): the loop equals the step entry driven one step at a time with
    hip.guide_positions between the steps, bit for bit in every slot, carry included; eager, captured and replayed loops agree; a second replay with another role
    follows the new role; with decay 'linear' the last step is the unguided step of the same previous state."""
    monkeypatch.delenv('ABOPT_STEP_COMPACT', raising=False)
    d, state, feats, role = _loop_case(flavour)
    kn = hip.check_guidance(**GUIDE)
    spec = _LoopSpec(3, use_bias_cache=True, guided=True, **kn)
    d.clear_graphs()
    try:
        want = _chain(d, state, feats, role, spec)
        run = lambda sp, r, graph: [a.clone() for a in d._denoise(sp, state, feats + (r,), None, 11, 4096, False, graph)[:3]]
        tv, tp, ts = run(spec, role, False)
        assert d.last_run_info['steps'] == 3 and d.last_run_info['graph'] is False and d.last_run_info['guided'] is True
        for j, (v, p, s) in enumerate(want):
            assert torch.equal(tv[2 - j], v) and torch.equal(tp[2 - j], p) and torch.equal(ts[2 - j], s), j
        plain = [a.clone() for a in d._denoise(_LoopSpec(3, use_bias_cache=True), state, feats, None, 11, 4096, False, False)[:3]]
        assert not torch.equal(plain[1][2], tp[2]) and not torch.equal(plain[1][0], tp[0])
        captured = run(spec, role, True)
        assert d.last_run_info['graph'] is True and len(d._graphs) == 1
        replayed = run(spec, role, True)
        assert len(d._graphs) == 1
        for a, b, c_ in zip((tv, tp, ts), captured, replayed):
            assert torch.equal(a, b) and torch.equal(a, c_)
        other = role.flip(1).contiguous()
        moved = run(spec, other, True)
        assert len(d._graphs) == 1
        fresh = _chain(d, state, feats, other, spec)
        assert torch.equal(moved[1][0], fresh[2][1]) and torch.equal(moved[0][0], fresh[2][0]) and not torch.equal(moved[1][0], tp[0])
        # decay 'linear': the step that lands on u = 0 carries weight 0
        lin = dataclasses.replace(spec, guide_decay=1)
        lv, lp, ls = run(lin, role, False)
        assert not torch.equal(lp[1], plain[1][1])
        last = d._denoise(_LoopSpec(1, use_bias_cache=True), (lv[1], lp[1], ls[1]), feats, None, 11, 4096, False, False)
        assert torch.equal(last[1][0], lp[0]) and torch.equal(last[0][0], lv[0]) and torch.equal(last[2][0], ls[0])
    finally:
        d.clear_graphs()


@pytest.mark.gpu
def test_plain_and_unguided_calls_share_one_graph():
    """sample(graph=True) without the keywords, with a role but no weight and with weights but no role: one captured loop serves all three, bit for bit."""
    d, state, feats, role = _loop_case('abdock')
    d.clear_graphs()
    try:
        run = lambda **kw: d.sample(*state, *feats, seed=3, graph=True, **kw)
        plain = run()
        info = dict(d.last_run_info)
        assert info['graph'] is True and len(d._graphs) == 1
        for kw in (dict(guide_role=role), dict(GUIDE), dict(guide_role=role, guide_attract=0.0, guide_repel=0.0, guide_decay='quadratic')):
            same = run(**kw)
            assert len(d._graphs) == 1 and d.last_run_info == info
            assert all(torch.equal(a.cpu(), b.cpu()) for t in plain for a, b in zip(plain[t], same[t])), kw
        guided = run(guide_role=role, **GUIDE)
        assert len(d._graphs) == 2 and not torch.equal(guided[0][1], plain[0][1])
    finally:
        d.clear_graphs()


@pytest.mark.gpu
def test_model_samplers_and_screen_carry_the_guidance():
    """batch['guide_role'] and the knobs in sample_opt reach the loop through model.sample / optimize; sample_replicated equals model.sample on the replicated batch;
    sample_grouped with a role per complex (one complex without) equals the per-complex calls at the launch's Philox offsets; the screen with (None, None) equals the
    call without the arguments in every field, and with hotspots and dock_guide it returns the same fields with other poses."""
    from test_aa_allowed import _design_batch, _same_traj
    m = build_model(10, 3, device=DEV)
    batch = _design_batch()
    N, L = batch['aa'].shape
    opt = dict(sample_structure=True, sample_sequence=True, seed=11, graph=False)
    roles = model_.guide_roles(batch, hotspots=[28, 29, 30], repel='context')
    free = m.sample(dict(batch), dict(opt, contig=''))
    assert _same_traj(free, m.sample(dict(batch, guide_role=roles), dict(opt, contig='')))                 # a role without a weight
    assert _same_traj(free, m.sample(dict(batch), dict(opt, contig='', **GUIDE)))                           # weights without a role
    led = m.sample(dict(batch, guide_role=roles), dict(opt, contig='', **GUIDE))
    gen = batch['generate_flag']
    assert sorted(led) == sorted(free) and not torch.equal(led[0][1], free[0][1]) and torch.equal(led[0][1][~gen], free[0][1][~gen])
    assert torch.equal(led[10][1].cpu(), free[10][1].cpu())                                                 # the initial state is not touched
    o_free, o_led = m.optimize(dict(batch), 4, dict(opt)), m.optimize(dict(batch, guide_role=roles), 4, dict(opt, **GUIDE))
    assert sorted(o_led) == sorted(o_free) and not torch.equal(o_led[0][1], o_free[0][1])
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(o_free[4][:3], o_led[4][:3]))
    with pytest.raises(ValueError, match='sample_structure=True'):
        m.sample(dict(batch, guide_role=roles), dict(opt, contig='', sample_structure=False, **GUIDE))
    c0 = dict({k: v[:1] for k, v in batch.items()}, guide_role=roles[:1])
    c1 = {k: v[1:2] for k, v in batch.items()}                                                              # no role: nothing moves there
    repl = {k: v.expand(4, *v.shape[1:]).contiguous() for k, v in c0.items()}
    rep = sampler.sample_replicated(m, dict(c0), 4, dict(opt, **GUIDE))
    assert _same_traj(rep, m.sample(repl, dict(opt, contig='', **GUIDE)))
    assert not _same_traj(rep, sampler.sample_replicated(m, dict(c0), 4, dict(opt)))
    grouped = sampler.sample_grouped(m, [dict(c0), dict(c1)], 2, dict(opt, rng_offset=0, **GUIDE))
    for gidx, c in enumerate((c0, c1)):
        single = sampler.sample_replicated(m, dict(c), 2, dict(opt, rng_offset=gidx * 2 * L, **GUIDE))
        for step in single:
            for a, b in zip(single[step], grouped[step]):
                assert torch.equal(a.cpu(), b[2 * gidx:2 * gidx + 2].cpu()), (gidx, step)
    # the screen
    P, S, k, D, contig, seed = 4, 3, 2, 3, '33-39', 5
    dock, design = screen_workers.models(DEV)
    one = screen_workers.complex_(DEV)
    kw = dict(contig=contig, screened_per_pose=k, seed=seed, poses_per_launch=P, screen_by='ppl')
    base = screen.optimize_antibody(dock, design, one, P, S, D, **kw)
    none = screen.optimize_antibody(dock, design, one, P, S, D, hotspots=None, dock_guide=None, **kw)
    assert sorted(base) == sorted(none)
    for name, v in base.items():
        assert torch.equal(none[name], v), name
    antigen = (one['fragment_type'][0] == 3).nonzero().flatten()
    hot = (antigen[:4] + 1).tolist()
    led = screen.optimize_antibody(dock, design, one, P, S, D, hotspots=hot, dock_guide=dict(guide_attract=0.5, guide_repel=0.5, repel='context'), **kw)
    assert sorted(led) == sorted(base) and all(led[n].shape == base[n].shape for n in base)
    assert not torch.equal(led['pose_ca'], base['pose_ca']) and bool(torch.isfinite(led['pose_ca']).all()) and bool(torch.isfinite(led['prmsd']).all())
    target = one['pos_heavyatom'][0, antigen[:4], 1].mean(0)
    dist = lambda r: [round(x, 2) for x in (r['pose_ca'].mean(1) - target).norm(dim=-1).tolist()]
    print('centroid of the docked residues to the hotspots, per pose: unguided', dist(base), 'guided', dist(led))       # hash-filled weights: a figure, not a gate
    with pytest.raises(ValueError, match='dock_guide'):
        screen.optimize_antibody(dock, design, one, P, S, D, hotspots=hot, **kw)
    with pytest.raises(ValueError, match='guide_attract must be <= 1'):
        screen.optimize_antibody(dock, design, one, P, S, D, hotspots=hot, dock_guide=dict(guide_attract=3), **kw)
