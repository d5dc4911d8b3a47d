"""Respaced sampling: sample(steps=K) / optimize(opt_step, steps=K) over a sub-sequence of the trained steps.

The definition is restated here in float64: `definition_scalars` (the scalars of a step t -> u), `restated_step` (the three transitions with those scalars) and
`igso3_truth` (the IGSO(3) series of ApproxAngularDistribution).  The CPU tests cover the sub-sequence, the scalars, the way the options reach the loop's spec, and the
conditioning of the injected draws the GPU tests replay; the GPU tests the loop itself (bit-identity with the plain loop at K = T, every respaced step against the
restatement, the device-built tables, the captured graph, the constrained sampler and the screen)."""
import ctypes
import dataclasses
import functools
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import screen_workers
from conftest import build_model, max_abs
from ab_opt_amd import hip, modules, sampler, screen
from ab_opt_amd.dpm import FullDPM, _LoopSpec, _graph_key, respaced_steps
from ab_opt_amd.utils import synth
from oracle import dpm as odpm, geometry as G
from test_hip_parity import rot_close

DEV = torch.device('cuda:0')
T, N, L = 100, 2, 24
SEED = 2                                    # the hash-filled T = 100 models the other tests of the session build too
GEN = [(4, 14)]
KS = (1, 7, 20)
# test_denoising_steps_teacher_forced_vs_reference checks at least 230 of its 256 residues per step (rot_close skips the others: the reference's own log map is noise
# there); the same share of the N L = 48 residues here
MAX_SKIPPED = (256 - 230) * N * L // 256


def f32(x):
    return ctypes.c_float(x).value


# ------------------------------------------------------------------------------------------ the definition, restated in float64
def definition_scalars(d, t, u):
    """The scalars of the step t -> u from the fp32 schedule buffers of FullDPM `d` (CPU), as python floats that hold fp32 values: a unit stride reads the buffers, a
    longer one computes alpha' = abar_t / abar_u and sigma = sqrt((1 - abar_u) / (1 - abar_t) (1 - alpha')) in float64 and rounds once."""
    vs, inv = d.trans_pos.var_sched, d.trans_rot.angular_distrib_inv
    ab = vs.alpha_bars.double().numpy()
    floor = float(vs.alphas[-2])
    out = dict(t=t, t_prev=u, alpha_bar=float(vs.alpha_bars[t]), sqrt_recip_abar=float(vs.sqrt_recip_alphas_cumprod[t]),
               sqrt_recipm1_abar=float(vs.sqrt_recipm1_alphas_cumprod[t]))
    if u == t - 1:
        out.update(alpha_clamped=max(float(vs.alphas[t]), floor), sigma=float(vs.sigmas[t]), igso3_std=float(inv.stddevs[t]), igso3_gaussian=int(inv.approx_flag[t]))
    else:
        a = ab[t] / ab[u]
        sig = float(np.float32(np.sqrt((1.0 - ab[u]) / (1.0 - ab[t]) * (1.0 - a))))
        out.update(alpha_clamped=float(np.float32(max(a, floor))), sigma=sig, igso3_std=sig, igso3_gaussian=int(np.float32(sig) <= np.float32(inv.std_threshold)))
    return out


def restated_init(v, p, s, gen, init):
    """FullDPM.sample's initial state (dpm_full.py:255-269) from the injected draws, float64; positions in Angstrom (position_mean 0, position_scale 10)."""
    gen3 = gen[..., None].expand(-1, -1, 3)
    v_i = torch.where(gen3, G.so3_log(G.quat_to_rot(init['q4'].double())), v.double())
    p_i = torch.where(gen3, init['p'].double() * 10.0, p.double())
    return v_i, p_i, torch.where(gen, init['s'], s)


def restated_step(sc, state, net, draws, gen, X, abdock, pred_x0, dist=(0.5, 19.5)):
    """One step t -> u of the loop in float64: state = (v, p in Angstrom, s), net = the network's outputs on that state (v_next, R_next, eps_pos, c[, prmsd_logits]),
    sc = definition_scalars, X = the bin starts linspace(0, pi, bins).  -> (v, p, s), (prmsd, ppl) or None, R_pre (what the transition's log map was fed)."""
    v, p, s = state
    gen3 = gen[..., None].expand(-1, -1, 3)
    noisy = sc['t_prev'] > 0                                                          # no noise on the step that lands on 0
    # rotation (transition.py:146-160; so3.py:111-146)
    sd = sc['igso3_std']
    b = draws['bin']
    hist = X[b] + draws['ubin'].double() * (X[b + 1] - X[b])
    gau = (sd * 2 + draws['gauss'].double() * sd).abs() % math.pi
    th = gau if sc['igso3_gaussian'] else hist
    e = torch.nn.functional.normalize(draws['axis'].double(), dim=-1) * th[..., None]
    if not noisy:
        e = torch.zeros_like(e)
    R_pre = G.so3_exp(e) @ G.so3_exp(net['v_next'].double())
    v_new = torch.where(gen3, G.so3_log(R_pre), v)
    # position (transition.py:42-50, 80-101), normalised coordinates
    pt = p / 10.0
    pnet = net['eps_pos'].double()
    eps = (sc['sqrt_recip_abar'] * pt - pnet) / sc['sqrt_recipm1_abar'] if pred_x0 else pnet
    c0 = 1.0 / math.sqrt(sc['alpha_clamped'] + 1e-8)
    c1 = (1.0 - sc['alpha_clamped']) / math.sqrt(1.0 - sc['alpha_bar'] + 1e-8)
    z = draws['z'].double() if noisy else torch.zeros_like(pt)
    p_new = torch.where(gen3, c0 * (pt - c1 * eps) + sc['sigma'] * z, pt) * 10.0
    # sequence (transition.py:202-245): alpha_bar_t on both factors whatever the stride; the injected sample is taken as it is
    ab = sc['alpha_bar']
    c_t = odpm.one_hot20(s).double()
    th_ = ((ab * c_t) + (1 - ab) / 20) * ((ab * net['c'].double()) + (1 - ab) / 20)
    post = torch.where(gen[..., None], th_ / (th_.sum(-1, keepdim=True) + 1e-8), c_t)
    extras = None
    if abdock:
        extras = (odpm.prmsd_score(net['prmsd_logits'].double(), *dist), odpm.perplexity(post, gen))
    return (v_new, p_new, draws['s_next']), extras, R_pre


def igso3_series(sigma, x, iters=1024):
    """Y of ApproxAngularDistribution._histograms_impl at the bin starts x (float64 numpy): sum over l < iters of c a b, nan_to_num, clamp_min(0)."""
    x = np.asarray(x, dtype=np.float64)[:, None]
    l = np.arange(iters, dtype=np.float64)[None, :]
    a = (2 * l + 1) * np.exp(-l * (l + 1) * np.float64(sigma) ** 2)
    Y = np.empty(x.shape[0])
    for lo in range(0, x.shape[0], 2048):
        xx = x[lo:lo + 2048]
        c = (1 - np.cos(xx)) / math.pi
        b = (np.sin((l + 0.5) * xx) + 1e-6) / (np.sin(xx / 2) + 1e-6)
        Y[lo:lo + 2048] = np.clip(np.nan_to_num((c * a * b).sum(1)), 0, None)
    return Y


def cdf_of(Y):
    """ApproxAngularDistribution.cdf(): the normalised prefix sum over the first bins - 1 cells."""
    y = Y[:-1]
    tot = y.sum()
    return np.cumsum(y) / (tot if tot > 0 else 1.0)


def igso3_truth(sigmas, X):
    """cdf rows (len(sigmas), bins - 1) of the series in float64, at the fp32 bin starts X the tables are built on."""
    x = X.double().numpy()
    with ThreadPoolExecutor(8) as pool:
        return np.stack(list(pool.map(lambda s: cdf_of(igso3_series(s, x)), sigmas)))


def loop_sigmas(d, K):
    """The IGSO(3) widths of the K-step loop's strides (fp32 values), in loop order."""
    ts = respaced_steps(T, K)
    return [definition_scalars(d, t, u)['igso3_std'] for t, u in zip(ts, ts[1:] + (0,))]


# ------------------------------------------------------------------------------------------ shared inputs and injected draws
@functools.lru_cache(None)
def inputs():
    """v, p (Angstrom), s, res_feat, pair_feat, mask_generate, mask_res on the CPU: N = 2 samples of L = 24 (21 in the second), residues 4..13 generated."""
    v, p, s, rf, pf, _, gen, mres = synth.eps_inputs(N, L, [L, L - 3], GEN, num_steps=T)
    return v, p * 10, s, rf, pf, gen, mres


@functools.lru_cache(None)
def coarse_cdf(sigma):
    """The series at every 64th bin start: enough to draw histogram bins the way multinomial(Y) would, cheaply."""
    x = torch.linspace(0, math.pi, 8192)[::64]
    return cdf_of(np.append(igso3_series(sigma, x.double().numpy()), 0.0))


@functools.lru_cache(None)
def draws_for(K):
    """Injected draws of sample(steps=K) in the layout sample(noise=...) takes: 'init' and one entry per visited step.  Axis, Gaussian and position draws are standard
    normal; a histogram bin is drawn from the stride's own IGSO(3) density (coarse_cdf, then uniformly inside the 64 bins); s_next is uniform over the twenty types on
    generated residues and the input type elsewhere."""
    d = build_model(T, SEED).diffusion
    v, p, s, rf, pf, gen, mres = inputs()
    g = torch.Generator().manual_seed(1000 + K)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    types = lambda: torch.where(gen, torch.randint(0, 20, (N, L), generator=g), s)
    nz = {'init': dict(q4=rn(N, L, 4), p=rn(N, L, 3), s=types())}
    ts = respaced_steps(T, K)
    for t, u in zip(ts, ts[1:] + (0,)):
        sig = definition_scalars(d, t, u)['igso3_std']
        cell = torch.from_numpy(np.searchsorted(coarse_cdf(sig), torch.rand(N, L, generator=g).numpy(), side='right')).clamp(0, 127) if sig > 0 else torch.zeros(N, L, dtype=torch.long)
        nz[t] = dict(axis=rn(N, L, 3), bin=(cell * 64 + torch.randint(0, 64, (N, L), generator=g)).clamp(0, 8190), ubin=torch.rand(N, L, generator=g), gauss=rn(N, L),
                     z=rn(N, L, 3), s_next=types())
    return nz


def walk(d_cpu, K, net_of, step_of=None):
    """The restated K-step loop from the injected draws of draws_for(K): every state is the restatement's own, the network outputs come from net_of(state32, t).
    step_of(state32, t, u) (optional): the code under test run for that one step from the same state; its result is compared in place.
    -> the restated states {tau: (v, p, s)} and the number of residues rot_close would check at each step."""
    v, p, s, rf, pf, gen, mres = inputs()
    nz = draws_for(K)
    X = torch.linspace(0, math.pi, 8192).double()
    abdock = d_cpu.abdock
    state = restated_init(v, p, s, gen, nz['init'])
    ts = respaced_steps(T, K)
    states, checked = {T: state}, {}
    for t, u in zip(ts, ts[1:] + (0,)):
        s32 = (state[0].float(), state[1].float(), state[2])
        net = net_of(s32, t)
        new, extras, R_pre = restated_step(definition_scalars(d_cpu, t, u), state, net, nz[t], gen, X, abdock, abdock and d_cpu.obj == 'pred_x0')
        checked[t] = rot_close(new[0], new[0], R_pre, R_upstream=net['R_next'].double())[0]
        if step_of is not None:
            got_v, got_p, got_s, got_pr, got_pp = step_of(s32, t, u)
            n, worst = rot_close(got_v, new[0], R_pre, R_upstream=net['R_next'].double())
            dp = max_abs(got_p, new[1])
            print(f'K={K} step {t}->{u}: rotations checked {n}/{N * L} worst err/tol {worst:.3f}; position {dp:.2e} A')
            assert n >= N * L - MAX_SKIPPED and worst < 1.0, (t, u, n, worst)
            assert dp < 1e-4, (t, u, dp)
            assert torch.equal(got_s, new[2]), (t, u)
            if abdock:
                assert max_abs(got_pr, extras[0]) < 1e-4 and max_abs(got_pp, extras[1]) < 1e-5, (t, u)
        state = new
        states[u] = state
    return states, checked


def cpu_net(m_cpu):
    """The oracle's EpsilonNet on the model's weights: stands in for the device's network where no device is there."""
    sd = m_cpu.state_dict()
    v, p, s, rf, pf, gen, mres = inputs()
    abdock = m_cpu.diffusion.abdock

    def net_of(state, t):
        beta = m_cpu.diffusion.trans_pos.var_sched.betas[t].expand([N])
        o = odpm.eps_net(sd, 'diffusion.eps_net.', state[0], state[1] / 10.0, state[2], rf, pf, beta, gen, mres, 6, prmsd_head=abdock, mode='mm')
        return dict(v_next=o[0], R_next=o[1], eps_pos=o[2], c=o[3], prmsd_logits=o[4] if abdock else None)
    return net_of


# ------------------------------------------------------------------------------------------ CPU: the sub-sequence
def test_respaced_steps_is_the_evenly_spaced_subsequence():
    assert respaced_steps(T, T) == respaced_steps(T) == tuple(range(T, 0, -1))
    assert respaced_steps(T, 1) == (T,)
    assert respaced_steps(10, 4) == (10, 8, 5, 3)                                    # tau_i = (10 i + 2) // 4
    for K in (7, 20, 33):
        ts = respaced_steps(T, K)
        assert len(ts) == K and ts[0] == T and ts[-1] >= 1 and all(a > b for a, b in zip(ts, ts[1:]))
        assert ts == tuple((i * T + K // 2) // K for i in range(K, 0, -1))
        assert respaced_steps(T, timesteps=ts) == ts and respaced_steps(T, timesteps=list(ts)) == ts
    for t0 in (1, 2, 10, 37):
        for K in range(1, t0 + 1):
            ts = respaced_steps(t0, K) + (0,)
            assert len(ts) == K + 1 and ts[0] == t0 and all(a > b for a, b in zip(ts, ts[1:]))
    assert respaced_steps(T, timesteps=range(T, 0, -1)) == tuple(range(T, 0, -1))
    assert respaced_steps(T, timesteps=[T, 50, 3]) == (T, 50, 3)
    for bad in (dict(steps=0), dict(steps=T + 1), dict(steps=-3), dict(timesteps=[T, 50, 50]), dict(timesteps=[T, 40, 60]), dict(timesteps=[T - 1, 5]),
                dict(timesteps=[T, 5, 0]), dict(timesteps=[]), dict(steps=20, timesteps=list(respaced_steps(T, 20)))):
        with pytest.raises(ValueError):
            respaced_steps(T, **bad)


# ------------------------------------------------------------------------------------------ CPU: the scalars of a step
FIELDS = ('alpha_clamped', 'alpha_bar', 'sigma', 'sqrt_recip_abar', 'sqrt_recipm1_abar', 'igso3_std')


def test_unit_strides_read_the_buffers_and_longer_ones_are_the_float64_formula():
    d = build_model(T, SEED).diffusion
    vs, inv = d.trans_pos.var_sched, d.trans_rot.angular_distrib_inv
    floor = float(vs.alphas[T - 1])
    bits = lambda x: np.float32(x).tobytes()
    for t in range(1, T + 1):                                                          # every unit stride: what _step_params(t) gave before there were strides
        for sp in (d._step_params(t, True, True, True), d._step_params(t, True, True, True, t_prev=t - 1)):
            assert (sp.t, sp.t_prev) == (t, t - 1)
            want = dict(alpha_clamped=max(vs.alphas[t], vs.alphas[T - 1]), alpha_bar=vs.alpha_bars[t], sigma=vs.sigmas[t], sqrt_recip_abar=vs.sqrt_recip_alphas_cumprod[t],
                        sqrt_recipm1_abar=vs.sqrt_recipm1_alphas_cumprod[t], igso3_std=inv.stddevs[t])
            for name in FIELDS:
                assert bits(getattr(sp, name)) == bits(float(want[name])), (t, name)
            assert sp.igso3_gaussian == int(inv.approx_flag[t])
    strides = 0
    for K in (1, 7, 20, 33, T):
        ts = respaced_steps(T, K)
        for j, (t, u) in enumerate(zip(ts, ts[1:] + (0,))):
            sp = d._step_params(t, True, True, False, True, t_prev=u)
            sc = definition_scalars(d, t, u)
            assert (sp.t, sp.t_prev) == (t, u) and (sp.t_prev == 0) == (j == K - 1)
            for name in FIELDS:
                assert bits(getattr(sp, name)) == bits(sc[name]), (K, t, u, name)
            assert sp.igso3_gaussian == sc['igso3_gaussian']
            assert sp.alpha_clamped >= floor
            assert (sp.pred_x0, sp.ppl_masked, sp.sample_structure, sp.sample_sequence) == (0, 0, 1, 1)
            if u != t - 1:                                                              # the float64 recomputation, spelled out once more here
                ab = vs.alpha_bars.double().numpy()
                a = ab[t] / ab[u]
                assert bits(sp.sigma) == bits(np.sqrt((1 - ab[u]) / (1 - ab[t]) * (1 - a))) and bits(sp.alpha_clamped) == bits(max(a, floor))
                assert sp.igso3_gaussian == int(np.float32(sp.sigma) <= np.float32(0.1))
                strides += 1
    assert strides == 1 + 7 + 20 + 33
    # both sides of the threshold occur among the strides of K = 20 and K = 33
    flags = {d._step_params(t, True, True, True, t_prev=u).igso3_gaussian for K in (20, 33) for t, u in zip(respaced_steps(T, K), respaced_steps(T, K)[1:] + (0,))}
    assert flags == {0, 1}


# ------------------------------------------------------------------------------------------ CPU: the options reach the loop's spec
class _Stop(Exception):
    pass


@pytest.fixture
def spec_of(monkeypatch):
    """spec_of(lambda d: d.sample(...)) -> the _LoopSpec that call hands to FullDPM._denoise (the device work before it is faked, the loop never starts)."""
    d = build_model(10, 3).diffusion
    seen = []

    def denoise(self, spec, state, inputs, *args, **kw):
        seen.append(spec)
        raise _Stop
    state = lambda *a, **kw: (torch.zeros(2, 8, 3), torch.zeros(2, 8, 3), torch.zeros(2, 8, dtype=torch.long))
    monkeypatch.setattr(FullDPM, '_denoise', denoise)
    for name, fake in (('lib', lambda: None), ('sample_init', state), ('add_noise', state), ('nonfinite_flag_reset', lambda: None)):
        monkeypatch.setattr(hip, name, fake)

    def run(call):
        with pytest.raises(_Stop):
            call(d)
        return seen.pop()
    return run


def test_steps_and_timesteps_reach_the_spec_in_one_spelling(spec_of):
    z, s = torch.zeros(2, 8, 3), torch.zeros(2, 8, dtype=torch.long)
    tail = (torch.zeros(2, 8, 128), torch.zeros(2, 8, 8, 64), torch.zeros(2, 8, dtype=torch.bool), torch.ones(2, 8, dtype=torch.bool))
    plain = spec_of(lambda d: d.sample(z, z, s, *tail, seed=1))
    assert plain.timesteps == 0 and FullDPM._loop_steps(plain) == [(t, t - 1) for t in range(10, 0, -1)]
    for kw in (dict(steps=10), dict(timesteps=range(10, 0, -1)), dict(steps=None, timesteps=None)):
        assert spec_of(lambda d: d.sample(z, z, s, *tail, seed=1, **kw)) == plain, kw            # the plain loop itself: same spec, same captured graph
    four = spec_of(lambda d: d.sample(z, z, s, *tail, seed=1, steps=4))
    assert four == dataclasses.replace(plain, timesteps=4) and FullDPM._loop_steps(four) == [(10, 8), (8, 5), (5, 3), (3, 0)]
    assert spec_of(lambda d: d.sample(z, z, s, *tail, seed=1, timesteps=[10, 8, 5, 3])) == four
    odd = spec_of(lambda d: d.sample(z, z, s, *tail, seed=1, timesteps=[10, 9, 2]))
    assert odd.timesteps == (10, 9, 2) and FullDPM._loop_steps(odd) == [(10, 9), (9, 2), (2, 0)]
    inputs_, token = tail, object()
    assert len({_graph_key(x, inputs_, token) for x in (plain, four, odd)}) == 3
    opt = spec_of(lambda d: d.optimize(z, z, s, 6, *tail, seed=1, steps=3))
    assert opt.t_start == 6 and opt.timesteps == 3 and FullDPM._loop_steps(opt) == [(6, 4), (4, 2), (2, 0)]
    assert spec_of(lambda d: d.optimize(z, z, s, 6, *tail, seed=1, steps=6)).timesteps == 0
    for call in (lambda d: d.sample(z, z, s, *tail, steps=11), lambda d: d.sample(z, z, s, *tail, steps=0), lambda d: d.optimize(z, z, s, 6, *tail, steps=7),
                 lambda d: d.sample(z, z, s, *tail, steps=4, timesteps=[10, 8, 5, 3]), lambda d: d.sample(z, z, s, *tail, timesteps=[9, 3]),
                 lambda d: d.optimize(z, z, s, 6, *tail, timesteps=[10, 3])):
        with pytest.raises(ValueError):
            call(build_model(10, 3).diffusion)


def test_model_samplers_and_screen_pass_the_options_on(monkeypatch):
    """model.sample / model.optimize hand sample_opt['steps'] / ['timesteps'] to the diffusion; the replicated and grouped samplers pass sample_opt through unchanged;
    the screen gives dock_steps to the dock and re-dock stages and design_steps to the design stage."""
    import inspect
    for fn in (FullDPM.sample, FullDPM.optimize):
        assert {'steps', 'timesteps'} <= set(inspect.signature(fn).parameters)          # named: sample() swallows unknown keywords
    assert {'dock_steps', 'design_steps'} <= set(inspect.signature(screen.optimize_antibody).parameters)
    seen = []

    class Diffusion(torch.nn.Module):
        def sample(self, *a, **kw):
            seen.append(('sample', kw))
            raise _Stop

        def optimize(self, *a, **kw):
            seen.append(('optimize', kw))
            raise _Stop
    m = synth.fresh_model(10, 3)
    m.diffusion = Diffusion()
    z = torch.zeros(1, 8, 3)
    monkeypatch.setattr(type(m), 'encode', lambda self, batch, **kw: (None, None, torch.eye(3).expand(1, 8, 3, 3), z))
    monkeypatch.setattr(hip, 'so3_log', lambda R, grad_mode=False: z)
    batch = dict(generate_flag=torch.ones(1, 8, dtype=torch.bool), mask=torch.ones(1, 8, dtype=torch.bool), aa=torch.zeros(1, 8, dtype=torch.long))
    calls = [lambda: m.sample(dict(batch), dict(sample_structure=True, sample_sequence=True, contig='', steps=4)),
             lambda: m.optimize(dict(batch), 6, dict(sample_structure=True, sample_sequence=True, timesteps=[6, 2])),
             lambda: sampler.sample_replicated(m, dict(batch), 3, dict(sample_structure=True, sample_sequence=True, steps=4)),
             lambda: sampler.sample_grouped(m, [dict(batch), dict(batch)], 3, dict(sample_structure=True, sample_sequence=True, timesteps=[6, 2]), optimize_step=6),
             lambda: sampler.sample_sharded(m, dict(batch, pos_heavyatom=torch.zeros(1, 8, 15, 3)), dict(sample_structure=True, sample_sequence=True, contig='', steps=4))]
    want = [('sample', 'steps', 4), ('optimize', 'timesteps', [6, 2]), ('sample', 'steps', 4), ('optimize', 'timesteps', [6, 2]), ('sample', 'steps', 4)]
    for call, (which, key, value) in zip(calls, want):
        with pytest.raises(_Stop):
            call()
        got, kw = seen.pop()
        assert got == which and kw[key] == value and ('steps' in kw) != ('timesteps' in kw)
    # the screen: which depth each stage asks its sampler for
    stages = []
    monkeypatch.setattr(sampler, 'sample_replicated', lambda model, one, n, opt, **kw: stages.append(opt) or (_ for _ in ()).throw(_Stop()))
    one = {k: v for k, v in synth.make_batch(1, synth.LAYOUT_128, seed=21).items()}
    with pytest.raises(_Stop):
        screen.optimize_antibody(None, None, one, 2, 2, 2, dock_steps=5, design_steps=3)
    assert stages.pop()['steps'] == 5
    with pytest.raises(_Stop):
        screen.optimize_antibody(None, None, one, 2, 2, 2)
    assert 'steps' not in stages.pop()


# ------------------------------------------------------------------------------------------ CPU: the injected draws leave the restatement well conditioned
@pytest.mark.parametrize('flavour', ['abdock', 'abdesign'])
def test_injected_draws_keep_the_restated_loop_within_the_skip_cap(flavour):
    """The float64 restatement alone, with the oracle's network in the device's place: at every step of K = 1, 7, 20 rot_close would check all but at most
    MAX_SKIPPED - 1 residues (one to spare: the device's network output differs from the oracle's in the last bits, which can move a residue across the line)."""
    m = build_model(T, SEED, flavour)
    for K in KS:
        states, checked = walk(m.diffusion, K, cpu_net(m))
        assert sorted(states) == sorted(respaced_steps(T, K) + (0,))
        assert min(checked.values()) >= N * L - MAX_SKIPPED + 1, (K, checked)
        assert all(torch.isfinite(st[0]).all() and torch.isfinite(st[1]).all() for st in states.values())


def test_restated_unit_step_is_the_oracles_step():
    """restated_step with the buffer scalars of a unit stride against oracle.dpm's own transitions (fp32) on the same inputs: the restatement states the loop body."""
    m = build_model(T, SEED)
    d = m.diffusion
    v, p, s, rf, pf, gen, mres = inputs()
    den = odpm.Denoiser(m.state_dict(), num_steps=T, variant='abdock', obj='pred_x0', mode='mm',
                        tables=(None, dict(stddevs=d.trans_rot.angular_distrib_inv.stddevs, approx_flag=d.trans_rot.angular_distrib_inv.approx_flag,
                                           X=d.trans_rot.angular_distrib_inv.X, Y=None)))
    nz = draws_for(20)
    X = torch.linspace(0, math.pi, 8192).double()
    for t, draws in ((60, nz[60]), (10, nz[10]), (1, nz[5])):
        v_n, p_n, s_n, ex = den.step(t, v, den.norm(p), s, rf, pf, gen, mres, draws)
        o = ex['eps_out']
        net = dict(v_next=o[0], R_next=o[1], eps_pos=o[2], c=o[3], prmsd_logits=o[4])
        new, extras, R_pre = restated_step(definition_scalars(d, t, t - 1), (v.double(), p.double(), s), net, draws, gen, X, True, True)
        n, worst = rot_close(v_n, new[0], R_pre, R_upstream=o[1])
        assert n >= N * L - MAX_SKIPPED and worst < 1.0
        assert max_abs(den.unnorm(p_n), new[1]) < 1e-4 and torch.equal(s_n, new[2])
        assert max_abs(ex['prmsd'], extras[0]) < 1e-4 and max_abs(ex['ppl'], extras[1]) < 1e-5


# ------------------------------------------------------------------------------------------ GPU
def _dev(x):
    if isinstance(x, dict):
        return {k: _dev(v) for k, v in x.items()}
    return x.to(DEV) if isinstance(x, torch.Tensor) else x


def _same_traj(a, b):
    return list(a) == list(b) and all(len(a[t]) == len(b[t]) and all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a[t], b[t])) for t in a)


@pytest.mark.gpu
@pytest.mark.parametrize('flavour', ['abdock', 'abdesign'])
def test_every_step_asked_for_in_three_ways_is_the_plain_loop_bit_for_bit(flavour):
    """sample(), sample(steps=T) and sample(timesteps=T..1) at one seed: the same trajectory in every slot; likewise optimize(opt_step=10)."""
    d = build_model(T, SEED, flavour, device=DEV).diffusion
    v, p, s, rf, pf, gen, mres = [_dev(a) for a in inputs()]
    plain = d.sample(v, p, s, rf, pf, gen, mres, seed=11, graph=False)
    assert sorted(plain) == list(range(T + 1)) and d.last_run_info['steps'] == T
    for kw in (dict(steps=T), dict(timesteps=range(T, 0, -1))):
        assert _same_traj(d.sample(v, p, s, rf, pf, gen, mres, seed=11, graph=False, **kw), plain), kw
    opt = d.optimize(v, p, s, 10, rf, pf, gen, mres, seed=11, graph=False)
    assert sorted(opt) == list(range(11)) and d.last_run_info['steps'] == 10
    for kw in (dict(steps=10), dict(timesteps=range(10, 0, -1))):
        assert _same_traj(d.optimize(v, p, s, 10, rf, pf, gen, mres, seed=11, graph=False, **kw), opt), kw


@pytest.mark.gpu
@pytest.mark.parametrize('flavour', ['abdock', 'abdesign'])
def test_respaced_steps_teacher_forced_vs_float64_restatement(flavour):
    """K = 1, 7, 20 with injected draws.  Every step t -> u of the respaced loop is run on the device from the restatement's own state and compared with the
    restatement, which is fed the device's network outputs on that state (hip.eps_net_forward): rotations under rot_close's conditioning (at most MAX_SKIPPED residues
    skipped, worst err / tol < 1), positions to 1e-4 Angstrom, the sequence exactly, prmsd to 1e-4 and perplexity to 1e-5 -- the figures of
    test_denoising_steps_teacher_forced_vs_reference.  Then sample(noise=..., steps=K) itself: the visited keys, the initial state, the
    injected sequence at every visited step and, for K = 7, every step of the loop against the single step run from the loop's own state.
    Measured on an MI355X: worst err / tol of the rotations 0.25, 46 or more of 48 residues checked; positions 5e-7 .. 7e-6 A on the AbDock walk; the AbDesign walk
    (noise prediction, hash-filled weights) drifts to |p| = 790 A, where one fp32 ulp is 6e-5 A, and reads up to 9.7e-5 A there."""
    m_cpu = build_model(T, SEED, flavour)
    d = build_model(T, SEED, flavour, device=DEV).diffusion
    v, p, s, rf, pf, gen, mres = [_dev(a) for a in inputs()]
    abdock = d.abdock
    ew = d.eps_net.packed()
    betas = d.trans_pos.var_sched.betas

    def net_of(state, t):
        o = hip.eps_net_forward(ew, _dev(state[0]), _dev(state[1]) / 10.0, _dev(state[2]), rf, pf, betas[t].expand(N).contiguous(), gen, mres, abdock, d.num_bins, False)
        return {k: (a.cpu() if a is not None else None) for k, a in o.items()}

    for K in KS:
        nz = _dev(draws_for(K))
        def step_of(state, t, u):
            spec = _LoopSpec(t, 1, True, True, True, timesteps=(t, u) if u > 0 else (t,))
            tv, tp, ts, tpr, tpp = d._denoise(spec, tuple(_dev(a) for a in state), (rf, pf, gen, mres), {t: nz[t]}, 0, 0, False, graph=False)
            assert d.last_run_info['steps'] == 1
            i = len(spec.timesteps) - 1                                                 # the slot of u
            out = (tv[i].cpu(), tp[i].cpu(), ts[i].cpu(), tpr[i].cpu() if abdock else None, tpp[i].cpu() if abdock else None)
            return out
        states, checked = walk(m_cpu.diffusion, K, net_of, step_of)
        ts = respaced_steps(T, K)
        traj = d.sample(v, p, s, rf, pf, gen, mres, noise=nz, steps=K, graph=False)
        assert list(traj) == list(ts) + [0] and d.last_run_info['steps'] == K
        assert len(traj[T]) == len(traj[0]) == (5 if abdock else 3) and traj[0][0].is_cuda and (K == 1 or not traj[ts[1]][0].is_cuda)
        v0, p0, s0 = states[T]
        assert max_abs(G.so3_exp(traj[T][0].double()), G.so3_exp(v0)) < 1e-4 and max_abs(traj[T][1], p0) < 1e-4 and torch.equal(traj[T][2], s0)
        for t, u in zip(ts, ts[1:] + (0,)):
            assert torch.equal(traj[u][2].cpu(), nz[t]['s_next'].cpu()), (K, t, u)
            assert all(torch.isfinite(a).all() for a in traj[u][:2])
            if K == 7:                                                                  # the loop's step t -> u is the single step above, run from the loop's own state
                one = step_of(tuple(a.cpu() for a in traj[t][:3]), t, u)
                assert max_abs(one[0], traj[u][0].cpu()) < 1e-5 and max_abs(one[1], traj[u][1].cpu()) < 1e-5 and torch.equal(one[2], traj[u][2].cpu()), (t, u)
                if abdock:
                    assert max_abs(one[3], traj[u][3]) < 1e-5 and max_abs(one[4], traj[u][4]) < 1e-5, (t, u)


@pytest.mark.gpu
def test_the_step_that_lands_on_zero_adds_no_noise():
    """K = 7: other rotation and position draws at the last visited step tau_1 leave traj[0] as it was, bit for bit; the same change one step earlier does not."""
    d = build_model(T, SEED, device=DEV).diffusion
    v, p, s, rf, pf, gen, mres = [_dev(a) for a in inputs()]
    nz = _dev(draws_for(7))
    ts = respaced_steps(T, 7)
    run = lambda noise: d.sample(v, p, s, rf, pf, gen, mres, noise=noise, steps=7, graph=False)
    base = run(nz)

    def redrawn(t):
        g = torch.Generator().manual_seed(77)
        other = dict(nz[t], axis=_dev(torch.randn(N, L, 3, generator=g)), gauss=_dev(torch.randn(N, L, generator=g)), z=_dev(torch.randn(N, L, 3, generator=g)),
                     ubin=_dev(torch.rand(N, L, generator=g)), bin=(nz[t]['bin'] + 17) % 8191)
        return {**nz, t: other}
    last = run(redrawn(ts[-1]))
    assert _same_traj(last, base)
    earlier = run(redrawn(ts[-2]))
    assert not torch.equal(earlier[ts[-1]][1], base[ts[-1]][1]) and not torch.equal(earlier[0][1], base[0][1])


@pytest.mark.gpu
def test_device_built_igso3_tables_vs_float64_series():
    """abopt_igso3_tables on the sigmas of the K = 7 and K = 20 loops and on widths at and around std_threshold, against the series in float64 (igso3_truth) at the
    same bin starts.  The bound is the host builder's own error on these rows, times 2 (the device sums in fp64; the factor covers differences of the elementary
    functions).  X is linspace(0, pi, bins) bit for bit; Y is non-negative; every cdf row is non-decreasing and ends at 1."""
    d = build_model(T, SEED).diffusion
    thr = d.trans_rot.angular_distrib_inv.std_threshold
    sigmas = sorted(set(loop_sigmas(d, 7) + loop_sigmas(d, 20) + [f32(x) for x in (0.02, 0.05, thr, thr * 1.001, 0.15, 1.5)]))
    assert sigmas[0] == 0.0 and any(0 < s <= thr for s in sigmas) and sum(s > thr for s in sigmas) >= 20
    X, Y, cdf = hip.igso3_tables(torch.tensor(sigmas, dtype=torch.float32, device=DEV))
    lin = torch.linspace(0, math.pi, 8192)
    assert X.shape == Y.shape == (len(sigmas), 8192) and cdf.shape == (len(sigmas), 8191)
    assert all(torch.equal(row, lin) for row in X.cpu())
    truth = igso3_truth(sigmas, lin)
    host = modules.ApproxAngularDistribution(sigmas).cdf().double().numpy()
    dev_cdf = cdf.cpu().double().numpy()
    err_host, err_dev = np.abs(host - truth).max(1), np.abs(dev_cdf - truth).max(1)
    for sg, eh, ed in zip(sigmas, err_host, err_dev):
        print(f'sigma {sg:.6f}: max |cdf - cdf64| host builder {eh:.3e}  device {ed:.3e}')
    print(f'all rows: host builder {err_host.max():.3e}  device {err_dev.max():.3e}')
    assert bool((err_dev <= 2 * err_host).all()), [(sg, eh, ed) for sg, eh, ed in zip(sigmas, err_host, err_dev) if ed > 2 * eh]       # row by row
    assert bool((Y >= 0).all()) and bool(torch.isfinite(Y).all())
    assert bool((cdf[:, 1:] >= cdf[:, :-1]).all()) and bool((cdf[:, -1] == 1).all())
    # odd sizes: bins that are no multiple of the workgroup, more terms than one staged chunk
    Xs, Ys, cs = hip.igso3_tables(torch.tensor([0.3, 0.7], dtype=torch.float32, device=DEV), bins=333, iters=1500)
    xs = torch.linspace(0, math.pi, 333)
    assert torch.equal(Xs[1].cpu(), xs)
    want = np.stack([cdf_of(igso3_series(f32(sg), xs.double().numpy(), 1500)) for sg in (0.3, 0.7)])
    assert np.abs(cs.cpu().double().numpy() - want).max() < 2e-7                       # two fp32 roundings (Y, then the cdf) of values below 1


@pytest.mark.gpu
def test_inverse_tables_reuse_trained_rows_and_cache_the_others():
    d = build_model(T, SEED, device=DEV).diffusion
    rot, inv = d.trans_rot, d.trans_rot.angular_distrib_inv
    pairs = FullDPM._loop_steps(_LoopSpec(T, timesteps=(T, 99, 60, 59, 7)))
    X, cdf = d._loop_tables(pairs)
    assert len(X) == len(cdf) == 5
    for j in (0, 2):                                                                    # 100 -> 99 and 60 -> 59: the trained rows themselves
        t = pairs[j][0]
        assert X[j].data_ptr() == inv.X[t].data_ptr() and cdf[j].data_ptr() == inv.cdf()[t].data_ptr()
    again = d._loop_tables(pairs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(X + cdf, again[0] + again[1]))
    sig = f32(d._stride(99, 60)[1])
    _, _, want = hip.igso3_tables(torch.tensor([sig], dtype=torch.float32, device=DEV))
    assert torch.equal(cdf[1], want[0])


@pytest.mark.gpu
@pytest.mark.parametrize('flavour', ['abdock', 'abdesign'])
def test_device_rng_respaced_run_is_reproducible_and_survives_capture(flavour):
    d = build_model(T, SEED, flavour, device=DEV).diffusion
    d.clear_graphs()
    v, p, s, rf, pf, gen, mres = [_dev(a) for a in inputs()]
    run = lambda graph, seed=23: d.sample(v, p, s, rf, pf, gen, mres, seed=seed, steps=20, graph=graph)
    try:
        a = run(False)
        assert d.last_run_info['steps'] == 20 and d.last_run_info['graph'] is False
        assert tuple(a) == respaced_steps(T, 20) + (0,)
        assert a[0][0].is_cuda and not a[5][0].is_cuda and len(a[T]) == (5 if d.abdock else 3)
        assert _same_traj(run(False), a)
        c = run(True)
        assert d.last_run_info['steps'] == 20 and d.last_run_info['graph'] is True and len(d._graphs) == 1
        assert _same_traj(c, a)
        assert _same_traj(run(True), a) and len(d._graphs) == 1                       # a replay
        other = run(True, seed=24)
        assert not torch.equal(other[0][1], a[0][1])
        full = d.sample(v, p, s, rf, pf, gen, mres, seed=23, graph=False)
        assert _same_traj({T: full[T]}, {T: a[T]})                                      # the same initial draw: tags and counters do not depend on the stride
        o = d.optimize(v, p, s, 30, rf, pf, gen, mres, seed=23, steps=6, graph=False)
        assert tuple(o) == respaced_steps(30, 6) + (0,) and d.last_run_info['steps'] == 6
        assert all(torch.isfinite(e[1]).all() for e in o.values())
    finally:
        d.clear_graphs()


@pytest.mark.gpu
def test_respaced_constrained_run_never_shows_a_forbidden_type():
    d = build_model(T, SEED, 'abdesign', device=DEV).diffusion
    v, p, s, rf, pf, gen, mres = [_dev(a) for a in inputs()]
    allowed = torch.full((N, L), (1 << 3) | (1 << 16), dtype=torch.int32, device=DEV)      # D or T, nothing else
    traj = d.sample(v, p, s, rf, pf, gen, mres, seed=5, steps=20, aa_allowed=allowed, graph=False)
    assert tuple(traj) == respaced_steps(T, 20) + (0,)
    for t, e in traj.items():
        types = e[2].to(DEV)[gen]
        assert bool(((types == 3) | (types == 16)).all()), t


@pytest.mark.gpu
def test_screen_with_respaced_stages_runs_and_does_not_depend_on_poses_per_launch(monkeypatch):
    """optimize_antibody(dock_steps=5, design_steps=5) at P = S = D = 2 on the T = 10 models: documented shapes, finite, 5 network evaluations per trajectory, and the
    same screen bit for bit with 1 or 2 poses per launch (one arithmetic form, as test_optimize_antibody_does_not_depend_on_poses_per_launch pins it)."""
    monkeypatch.setenv('ABOPT_PAIR_TERMS', '0')
    monkeypatch.setenv('ABOPT_CORE_NO_SPLIT', '1')
    dock, design = screen_workers.models(DEV)
    one = screen_workers.complex_(DEV)
    kw = dict(num_poses=2, designs_per_pose=2, redocks_per_design=2, contig='33-39', seed=17, dock_steps=5, design_steps=5)
    runs = [screen.optimize_antibody(dock, design, one, poses_per_launch=n, **kw) for n in (2, 1)]
    assert dock.diffusion.last_run_info['steps'] == 5 and design.diffusion.last_run_info['steps'] == 5
    res = runs[0]
    n_dock, n_design = int(one['generate_flag'].sum()), 7
    shapes = dict(pose_ca=(2, n_dock, 3), pose_score=(2,), seqs=(2, 2, n_design), aar=(2, 2), ppl=(2, 2), chosen=(2, 1), dockq=(2, 1, 2, 4), prmsd=(2, 1, 2),
                  redock_score=(2, 1, 2), dockq_mean=(2, 1), dockq_std=(2, 1), prmsd_mean=(2, 1), prmsd_std=(2, 1))
    assert set(res) == set(shapes)
    for name, shape in shapes.items():
        assert tuple(res[name].shape) == shape and bool(torch.isfinite(res[name].float()).all()), name
        assert torch.equal(runs[1][name], res[name]), name
    full = screen.optimize_antibody(dock, design, one, poses_per_launch=2, **dict(kw, dock_steps=None, design_steps=None))
    assert dock.diffusion.last_run_info['steps'] == 10 and not torch.equal(full['pose_ca'], res['pose_ca'])
