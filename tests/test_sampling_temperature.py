"""Sampling at a temperature (include/abopt.h: abopt_step_params.tempered / seq_temperature / noise_scale, ABI 55): the residue types of a step
drawn from the posterior of the network's prediction at temperature tau, the structure noise of a step scaled by lambda.

The float64 statement of the tempered prediction (`tempered_prediction`, `tempered_statement`) lives here and is the reference of the posterior test; the posterior
behind it, the perplexity and the masks are the statements of tests/test_aa_allowed.py, imported.  The CPU tests cover the validation, the way the knobs reach the
loop's spec and the step's scalars, and the limits of the statement; the GPU tests the step kernel directly (bit-identity at the defaults, the posterior against the
statement, the draws, the scaled structure noise), a whole tempered loop fused, unfused and replayed, and the way through the model, the samplers and the screen."""
import dataclasses
import math

import pytest
import torch

import screen_workers
import step_harness
from conftest import build_model
from ab_opt_amd import hip, model as model_, sampler, screen
from ab_opt_amd.dpm import FullDPM, _LoopSpec, _graph_key
from ab_opt_amd.utils import synth
from oracle import geometry as G
from test_aa_allowed import (FULL, K, _kernel_case, _design_batch, _same_traj, _traj_obeys, _words, allowed_bits, bits_of, obeys, perplexity_statement,
                             posterior_statement)
from test_hip_parity import rot_close

DEV = torch.device('cuda:0')
TAUS = (0.0, 0.1, 0.5, 2.0)
# Tolerances of test_tempered_posterior_vs_fp64_statement: four times the worst error measured against the float64 statement on one MI355X at that tau (DESIGN.md
# section 3.11 lists the measured values), never below the project's own at tau = 1 (2e-6 on the posterior, 1e-5 on the perplexity: tests/test_aa_allowed.py)
MEASURED_POST = {0.0: 4.64e-7, 0.1: 4.59e-7, 0.5: 2.52e-7, 2.0: 2.84e-7}
MEASURED_PPL = {0.0: 2.03e-8, 0.1: 8.93e-9, 0.5: 1.18e-8, 2.0: 1.39e-8}
TOL_POST = {tau: max(2e-6, 4 * e) for tau, e in MEASURED_POST.items()}
TOL_PPL = {tau: max(1e-5, 4 * e) for tau, e in MEASURED_PPL.items()}


# ------------------------------------------------------------------------------------------ the fp64 statement
def tempered_prediction(c_net, bits, tau):
    """c' of the definition, float64, for every row: over the allowed classes `bits` (..., 20), m = max max(c_k, 0), e_k = exp2((log2 max(c_k, 0) - log2 m) / tau),
    c'_k = e_k / sum e; tau = 0: one-hot at the lowest-index allowed class with max(c_k, 0) == m.  Rows with m == 0 or not finite keep c."""
    c = c_net.double().clamp_min(0)
    m = torch.where(bits, c, torch.zeros_like(c)).amax(-1, keepdim=True)
    if tau == 0:
        hit = bits & (c == m)
        first = hit & (hit.long().cumsum(-1) == 1)
        out = first.double()
    else:
        e = torch.where(bits, torch.exp2((torch.log2(c) - torch.log2(m)) / tau), torch.zeros_like(c))
        out = e / e.sum(-1, keepdim=True)
    return torch.where((m > 0) & torch.isfinite(m), out, c_net.double())


def tempered_statement(c_net, gen, allow, tau):
    """What the posterior is formed from at temperature tau: c' on the rows that draw (generated, a non-empty set) when tau != 1, c_net itself elsewhere."""
    if tau == 1:
        return c_net.double()
    draws = gen & ((allow.long() & FULL) != 0)
    return torch.where(draws[..., None], tempered_prediction(c_net, allowed_bits(allow), tau), c_net.double())


# ------------------------------------------------------------------------------------------ CPU
def test_temperature_and_scale_are_validated_without_a_device():
    assert hip.check_temperature('t', 0) == 0.0 and hip.check_temperature('t', 1e-3) == 1e-3 and hip.check_temperature('t', 2) == 2.0
    assert hip.check_noise_scale('s', 0) == 0.0 and hip.check_noise_scale('s', 1e-9) == 1e-9 and hip.check_noise_scale('s', 3) == 3.0
    for bad in (-0.5, -1e-9, float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError, match='finite and >= 0'):
            hip.check_temperature('seq_temperature', bad)
        with pytest.raises(ValueError, match='finite and >= 0'):
            hip.check_noise_scale('noise_scale', bad)
    for tiny in (1e-30, 1e-6, 9.9e-4):
        with pytest.raises(ValueError, match='at least 1e-3'):
            hip.check_temperature('seq_temperature', tiny)
    # sample() and optimize() refuse before anything touches a device; the screen's two arguments go through the same checks
    d = build_model(10, 3).diffusion
    z = torch.zeros(2, 8, 3)
    gen = torch.zeros(2, 8, dtype=torch.bool)
    gen[:, 2:5] = True
    tail = (torch.zeros(2, 8, 128), torch.zeros(2, 8, 8, 64), gen, torch.ones(2, 8, dtype=torch.bool))
    s = torch.zeros(2, 8, dtype=torch.long)
    for kw, msg in ((dict(seq_temperature=-1), 'seq_temperature must be finite'), (dict(seq_temperature=1e-4), 'at least 1e-3'), (dict(noise_scale=float('nan')), 'noise_scale must be')):
        with pytest.raises(ValueError, match=msg):
            d.sample(z, z, s, *tail, seed=1, **kw)
        with pytest.raises(ValueError, match=msg):
            d.optimize(z, z, s, 4, *tail, seed=1, **kw)


def test_loop_spec_and_step_params_carry_the_knobs():
    d = build_model(10, 3).diffusion
    inputs = (torch.zeros(2, 8, 128), torch.zeros(2, 8, 8, 64), torch.zeros(2, 8, dtype=torch.bool), torch.ones(2, 8, dtype=torch.bool))
    token = object()
    plain = _LoopSpec(10)
    assert (plain.seq_temperature, plain.noise_scale) == (1.0, 1.0)
    assert _graph_key(_LoopSpec(10, seq_temperature=1, noise_scale=1.0), inputs, token) == _graph_key(plain, inputs, token)
    keys = {_graph_key(s, inputs, token) for s in (plain, dataclasses.replace(plain, seq_temperature=0.5), dataclasses.replace(plain, noise_scale=0.5),
                                                   dataclasses.replace(plain, seq_temperature=0.0), dataclasses.replace(plain, seq_temperature=0.5, noise_scale=0.5))}
    assert len(keys) == 5
    sp = d._step_params(7, True, True, True)
    assert (sp.tempered, sp.seq_temperature, sp.noise_scale) == (0, 0.0, 0.0)
    assert bytes(sp) == bytes(d._step_params(7, True, True, True, seq_temperature=1.0, noise_scale=1)) and bytes(sp)[-12:] == bytes(12)
    for tau, lam in ((0.5, 1.0), (1.0, 0.25), (0.0, 2.0)):
        sp = d._step_params(7, True, True, True, seq_temperature=tau, noise_scale=lam)
        assert (sp.tempered, sp.seq_temperature, sp.noise_scale) == (1, tau, lam) and (sp.t, sp.t_prev) == (7, 6)
    with pytest.raises(ValueError, match='at least 1e-3'):
        d._step_params(7, True, True, True, seq_temperature=5e-4)
    # sample() / optimize() put the two values into the spec they hand to _denoise
    seen = []

    class Stop(Exception):
        pass

    def denoise(self, spec, *args, **kw):
        seen.append(spec)
        raise Stop
    z, s = torch.zeros(2, 8, 3), torch.zeros(2, 8, dtype=torch.long)
    state = lambda *args, **kw: (z, z, s)
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(FullDPM, '_denoise', denoise)
        for name, fake in (('lib', lambda: None), ('sample_init', state), ('add_noise', state), ('nonfinite_flag_reset', lambda: None)):
            mp.setattr(hip, name, fake)
        for call in (lambda **kw: d.sample(z, z, s, *inputs, seed=1, **kw), lambda **kw: d.optimize(z, z, s, 4, *inputs, seed=1, **kw)):
            for kw in ({}, dict(seq_temperature=0.5), dict(noise_scale=0), dict(seq_temperature=2, noise_scale=0.5)):
                with pytest.raises(Stop):
                    call(**kw)
                spec = seen.pop()
                assert (spec.seq_temperature, spec.noise_scale) == (float(kw.get('seq_temperature', 1.0)), float(kw.get('noise_scale', 1.0)))
                assert (spec == dataclasses.replace(spec, seq_temperature=1.0, noise_scale=1.0)) is (not kw)
    finally:
        mp.undo()


def test_statement_limits():
    """tau = 1: the tempered prediction of a normalised c_net is c_net (no mask), so the posterior statement is the untempered one; tau = 0: the one-hot limit of the
    formula as tau -> 0, on rows whose two largest allowed classes differ by 5 % or more ((1 / 1.05)^1000 = 6e-22 at tau = 1e-3)."""
    N, L = 3, 300
    c = torch.softmax(synth.hash_tensor((N, L, K), 11, scale=6.0), -1)
    gen = torch.ones(N, L, dtype=torch.bool)
    gen[:, ::5] = False
    s_t = (synth.hash_tensor((N, L), 12) + 0.5).mul(K).long().clamp(0, K - 1)
    full = torch.full((N, L), FULL)
    every = allowed_bits(full)
    assert (tempered_prediction(c, every, 1.0) - c.double()).abs().max().item() < 1e-7          # (c is normalised in fp32: its fp64 sum is 1 to 1e-7)
    want = posterior_statement(c, s_t, gen, full, 0.785)
    assert torch.equal(posterior_statement(tempered_statement(c, gen, full, 1.0), s_t, gen, full, 0.785), want)
    assert (posterior_statement(tempered_prediction(c, every, 1.0), s_t, gen, full, 0.785) - want).abs().max().item() < 1e-7
    rs = torch.Generator().manual_seed(4)
    allow = torch.randint(1, FULL + 1, (N, L), generator=rs)
    bits = allowed_bits(allow)
    top2 = torch.where(bits, c.double(), torch.zeros(())).topk(2, -1)[0]
    clear = top2[..., 1] <= top2[..., 0] / 1.05
    assert int(clear.sum()) > N * L // 2
    greedy, limit = tempered_prediction(c, bits, 0.0), tempered_prediction(c, bits, 1e-3)
    assert (greedy - limit)[clear].abs().max().item() < 1e-12
    assert bool((greedy.sum(-1) == 1).all()) and bool((greedy.max(-1)[0] == 1).all()) and bool((greedy[~bits] == 0).all())
    assert torch.equal(greedy.argmax(-1), torch.where(bits, c.double(), -torch.ones(())).argmax(-1))
    tie = torch.tensor([[0.0, 0.3, 0.1, 0.3, 0.3] + [0.0] * 15])                                 # exact ties: the lowest allowed index takes all
    assert tempered_prediction(tie, allowed_bits(torch.tensor([FULL])), 0.0).argmax(-1).item() == 1
    assert tempered_prediction(tie, allowed_bits(torch.tensor([FULL & ~2])), 0.0).argmax(-1).item() == 3
    zero = torch.zeros(1, K)                                                                     # nothing to sharpen
    assert torch.equal(tempered_prediction(zero, allowed_bits(torch.tensor([FULL])), 0.5), zero.double())


# ------------------------------------------------------------------------------------------ GPU: the step kernel, directly
def _step(d, t, g, allow=None, tau=1.0, lam=1.0, force=None, seed=99, ppl_masked=True, noise=None, c_net=None):
    """One direct abopt_denoise_step call on the inputs of tests/test_aa_allowed.py::_kernel_case.  force = (tempered, tau, lambda): written into the struct as they are."""
    N, L = g['gen'].shape
    sp = d._step_params(t, True, True, ppl_masked, seq_temperature=tau, noise_scale=lam)
    if force is not None:
        sp.tempered, sp.seq_temperature, sp.noise_scale = force
    inv = d.trans_rot.angular_distrib_inv
    out = dict(v=torch.empty(N, L, 3, device=DEV), p=torch.empty(N, L, 3, device=DEV), s=torch.empty(N, L, dtype=torch.int64, device=DEV),
               prmsd=torch.empty(N, device=DEV), ppl=torch.empty(N, device=DEV), p_norm=torch.empty(N, L, 3, device=DEV))
    out['post'] = hip.denoise_step(sp, noise, seed, 0, g['v'], g['p'], g['s'], g['v_net'], g['p_net'], g['c_net'] if c_net is None else c_net,
                                   torch.zeros(N, 40, device=DEV), g['gen'], inv.X[t], None if noise is not None else inv.cdf()[t], 40, out, want_post=True, aa_allowed=allow)
    return out, sp


OUTPUTS = ('v', 'p', 's', 'prmsd', 'ppl', 'p_norm', 'post')


@pytest.mark.gpu
@pytest.mark.parametrize('flavour', ['abdock', 'abdesign'])
def test_defaults_and_unit_values_are_bit_identical(flavour):
    """N = 3, L = 300 (the 256-thread stride loop and a ragged last wave), device RNG, one step on each IGSO(3) branch: no arguments, (1.0, 1.0), and tempered = 1
    forced with (1, 1) through the raw binding give the same bits in every output of the step; a tempered step does not (the comparison can fail)."""
    N, L = 3, 300
    _, _, _, g = _kernel_case(N, L)
    d = build_model(100, 2, flavour, device=DEV).diffusion
    allow = _words(N, L, FULL & ~bits_of('CM'))
    for t in (30, 10):
        assert int(d.trans_rot.angular_distrib_inv.approx_flag[t]) == (1 if t == 10 else 0)
        for a in (None, allow):
            plain, sp0 = _step(d, t, g, a)
            assert sp0.tempered == 0 and sp0.pred_x0 == (1 if flavour == 'abdock' else 0)
            ones, sp1 = _step(d, t, g, a, tau=1.0, lam=1.0)
            forced, sp2 = _step(d, t, g, a, force=(1, 1.0, 1.0))
            assert sp1.tempered == 0 and sp2.tempered == 1
            for k in OUTPUTS:
                assert torch.equal(plain[k], ones[k]) and torch.equal(plain[k], forced[k]), (t, k)
            other, _ = _step(d, t, g, a, tau=0.5, lam=0.5)
            assert not torch.equal(plain['v'], other['v']) and not torch.equal(plain['p'], other['p']) and not torch.equal(plain['post'], other['post'])


def _mask_family(cpu, c_net):
    """The masks of test_constrained_posterior_vs_fp64_statement: random non-empty words, then by residue index mod 7 -- single-type sets, sets without s_t, sets without
    the argmax of c_net -- a few empty words on generated residues (frozen) and arbitrary words, empty ones among them, on context residues."""
    gen, s_t = cpu['gen'], cpu['s']
    N, L = gen.shape
    rs = torch.Generator().manual_seed(4)
    allow = torch.randint(1, FULL + 1, (N, L), generator=rs)
    idx = torch.arange(N * L).view(N, L)
    single = idx % 7 == 1
    allow[single] = (1 << torch.randint(0, K, (N, L), generator=rs))[single]
    no_st = idx % 7 == 2
    allow[no_st] &= ~(1 << s_t)[no_st]
    no_top = idx % 7 == 3
    allow[no_top] &= ~(1 << c_net.argmax(-1))[no_top]
    allow[allow == 0] = bits_of('GP')
    empty = gen & (idx % 41 == 6)
    allow[empty] = 0
    allow[0, 0] = 0                                                         # context residues (every fifth): never read
    allow[1, 5] = 1 << 25
    assert int(empty.sum()) >= 5 and not gen[0, 0] and not gen[1, 5] and bool((single & gen).any() and (no_st & gen).any() and (no_top & gen).any())
    return allow, empty


@pytest.mark.gpu
def test_tempered_posterior_vs_fp64_statement():
    """post_out and the perplexity of a tempered step against the float64 statement at N = 3, L = 300, skewed c_net per residue with exact ties of the two largest
    classes on every 11th residue, tau in {0, 0.1, 0.5, 2}, without a mask and with the mask family of test_constrained_posterior_vs_fp64_statement.  Tolerances:
    TOL_POST / TOL_PPL above.  Disallowed classes are exactly zero, context and frozen rows exactly onehot(s_t), and at tau = 0 the posterior is the statement's on the
    one-hot prediction at the lowest-index maximum (the ties are there for this)."""
    N, L = 3, 300
    d, t, cpu, g = _kernel_case(N, L)
    gen, s_t = cpu['gen'], cpu['s']
    c_net = cpu['c_net'].clone()
    idx = torch.arange(N * L).view(N, L)
    tied = idx % 11 == 4
    top2 = c_net.topk(2, -1)
    c_net[tied] = c_net[tied].scatter(-1, top2[1][tied][:, 1:], top2[0][tied][:, :1])          # the runner-up takes the maximum's value: an exact tie
    assert int((tied & gen).sum()) >= 50 and bool((c_net[tied].topk(2, -1)[0].diff(dim=-1) == 0).all())
    c_dev = c_net.to(DEV)
    family, empty = _mask_family(cpu, c_net)
    onehot = torch.nn.functional.one_hot(s_t, K).float()
    worst = {}
    for tau in TAUS:
        for name, allow, frozen in (('free', None, torch.zeros_like(gen)), ('masked', family, empty)):
            words = torch.full((N, L), FULL) if allow is None else allow
            for masked in (True, False):
                out, sp = _step(d, t, g, None if allow is None else allow.to(torch.int32).to(DEV), tau=tau, ppl_masked=masked, c_net=c_dev)
                assert sp.tempered == 1
                want = posterior_statement(tempered_statement(c_net, gen, words, tau), s_t, gen, words, sp.alpha_bar)
                post, s_next = out['post'].cpu(), out['s'].cpu()
                err = (post.double() - want).abs().max().item()
                ppl_err = (out['ppl'].cpu().double() - perplexity_statement(want, gen, masked)).abs().max().item()
                print(f'tempered posterior tau={tau} {name} ppl_masked={masked}: max abs error {err:.3g}, perplexity error {ppl_err:.3g}')
                worst[tau] = (max(worst.get(tau, (0, 0))[0], err), max(worst.get(tau, (0, 0))[1], ppl_err))
                assert err < TOL_POST[tau], (tau, name, err)
                assert ppl_err < TOL_PPL[tau], (tau, name, ppl_err)
                live = gen & ~frozen
                assert torch.equal(post[frozen], onehot[frozen]) and torch.equal(s_next[frozen], s_t[frozen])
                assert torch.equal(post[~gen], onehot[~gen]) and torch.equal(s_next[~gen], s_t[~gen])
                assert bool((post[~allowed_bits(words) & live[..., None]] == 0).all())                  # exactly zero, not small
                assert obeys(s_next, words, live)
                if tau == 0:
                    # all the prediction's mass on the lowest-index allowed maximum: the posterior there is that of a one-hot x0, bit for bit what the plain step
                    # gives on the one-hot prediction
                    first = tempered_prediction(c_net, allowed_bits(words), 0.0).float()
                    assert bool((first.sum(-1)[live] == 1).all())
                    hot, _ = _step(d, t, g, None if allow is None else allow.to(torch.int32).to(DEV), ppl_masked=masked, c_net=first.to(DEV))
                    assert torch.equal(post[live], hot['post'].cpu()[live])
                    lowest = torch.where(allowed_bits(words) & (c_net.clamp_min(0) == torch.where(allowed_bits(words), c_net.clamp_min(0), torch.zeros(())).amax(-1, keepdim=True)),
                                         torch.arange(K).expand(N, L, K), K).amin(-1)
                    assert torch.equal(first.argmax(-1)[live & tied], lowest[live & tied])
    print('worst per tau (posterior, perplexity):', {tau: (f'{a:.3g}', f'{b:.3g}') for tau, (a, b) in worst.items()})


def _chi2_ok(draws, prob, n):
    """The rule of test_sequence_sampler_draws_from_the_posterior (restated from tests/test_aa_allowed.py): per-class chi-square over the classes with expectation
    > 10, bound 3 x their count."""
    freq = torch.zeros(K, dtype=torch.float64).scatter_add_(0, draws, torch.ones(n, dtype=torch.float64))
    exp = prob.double() * n
    keep = exp > 10
    chi2 = (((freq - exp) ** 2 / exp)[keep]).sum().item()
    print(f'chi2 {chi2:.2f} over {int(keep.sum())} classes')
    return chi2 < 3 * int(keep.sum()) and freq[~keep].sum() <= 10 * (~keep).sum() + 20 and int(keep.sum()) >= 2


@pytest.mark.gpu
def test_draws_follow_the_tempered_posterior():
    """N = 64, L = 256, one skewed prediction everywhere, tau = 0.5: s_next on the generated rows follows post_out by the chi-square rule, post_out is the statement's,
    and it is not the untempered posterior.  At least 4 classes keep an expectation above 10 (asserted on the statement, before the device is asked)."""
    N, L, tau = 64, 256, 0.5
    d, t, cpu, g = _kernel_case(N, L, skew_same=True)
    gen, n = cpu['gen'], int(cpu['gen'].sum())
    full = torch.full((N, L), FULL)
    ab = d._step_params(t, True, True, True).alpha_bar
    want = posterior_statement(tempered_statement(cpu['c_net'], gen, full, tau), cpu['s'], gen, full, ab)[gen][0]
    plain = posterior_statement(cpu['c_net'], cpu['s'], gen, full, ab)[gen][0]
    assert int((want * n > 10).sum()) >= 4 and (want - plain).abs().max().item() > 0.02
    out, _ = _step(d, t, g, None, tau=tau)
    pg = out['post'][g['gen']][0].cpu()
    assert (pg.double() - want).abs().max().item() < TOL_POST[tau]
    s_next = out['s'].cpu()
    assert torch.equal(s_next[~gen], cpu['s'][~gen])
    assert _chi2_ok(s_next[gen], pg, n)
    assert not _chi2_ok(s_next[gen], plain.float(), n)                      # the draws tell the two distributions apart


def _injected(N, L, salt=700):
    h = lambda shape, k, scale=1.0: synth.hash_tensor(shape, salt + k, scale=scale).to(DEV)
    return dict(axis=h((N, L, 3), 0, 2.0), bin=(h((N, L), 1) + 0.5).mul(8190).long().clamp(0, 8190), ubin=(h((N, L), 2) + 0.5).clamp(0, 0.999),
                gauss=h((N, L), 3, 2.0), z=h((N, L, 3), 4, 2.0), s_next=(h((N, L), 5) + 0.5).mul(20).long().clamp(0, 19))


def _rotation_statement(sp, lam, noise, v_net, X):
    """float64: R_pre = exp(lambda e) exp(v_net) and its log, e = the normalised axis times the IGSO(3) angle of the step's branch (fp32 scalars of the step)."""
    b = noise['bin'].cpu()
    X = X.cpu().double()
    hist = X[b] + noise['ubin'].cpu().double() * (X[b + 1] - X[b])
    sd = float(sp.igso3_std)
    gau = (sd * 2 + noise['gauss'].cpu().double() * sd).abs() % math.pi
    th = (gau if sp.igso3_gaussian else hist) * lam
    e = torch.nn.functional.normalize(noise['axis'].cpu().double(), dim=-1) * th[..., None]
    R_pre = G.so3_exp(e) @ G.so3_exp(v_net.double())
    return G.so3_log(R_pre), R_pre


@pytest.mark.gpu
@pytest.mark.parametrize('t', [30, 10], ids=['histogram', 'gaussian'])
def test_noise_scale_scales_the_structure_noise(t):
    """Injected noise at N = 3, L = 300, one t on each IGSO(3) branch.  lambda = 0.5: p_next is, bit for bit, the plain step's with the injected z halved (scaling by a
    power of two commutes with the rounding).  lambda in {0.5, 2, 0}: v_next against the float64 statement log(exp(lambda e) exp(v_net)) by rot_close, the comparison of
    test_denoising_steps_teacher_forced_vs_reference for v_next with its exemptions and its share of checked rows (230 of 256).  lambda = 0: p_next equals the plain
    step with injected z = 0, and two seeds of the device stream give the same v_next and p_next."""
    N, L = 3, 300
    d, _, cpu, g = _kernel_case(N, L)
    gen = cpu['gen']
    noise = _injected(N, L)
    X = d.trans_rot.angular_distrib_inv.X[t]
    plain, sp = _step(d, t, g, noise=noise)
    assert int(sp.igso3_gaussian) == (1 if t == 10 else 0) and sp.t_prev > 0
    half, _ = _step(d, t, g, lam=0.5, noise=noise)
    halved, _ = _step(d, t, g, noise=dict(noise, z=noise['z'] * 0.5))
    assert torch.equal(half['p'], halved['p']) and torch.equal(half['p_norm'], halved['p_norm']) and not torch.equal(half['p'], plain['p'])
    for k in ('s', 'post', 'ppl'):                                                     # lambda leaves the sequence alone
        assert torch.equal(half[k], plain[k]), k
    zero, _ = _step(d, t, g, lam=0.0, noise=noise)
    still, _ = _step(d, t, g, noise=dict(noise, z=torch.zeros_like(noise['z'])))
    assert torch.equal(zero['p'], still['p'])
    runs = {1.0: plain, 0.5: half, 0.0: zero, 2.0: _step(d, t, g, lam=2.0, noise=noise)[0]}
    min_checked = int(gen.sum()) * 230 // 256
    for lam, out in runs.items():
        want, R_pre = _rotation_statement(sp, lam, noise, cpu['v_net'], X)
        v = out['v'].cpu()
        assert torch.equal(v[~gen], cpu['v'][~gen])
        n, worst = rot_close(v[gen], want[gen], R_pre[gen])
        print(f't={t} lambda={lam}: {n} of {int(gen.sum())} rows checked, worst error / tolerance {worst:.3f}')
        assert n >= min_checked and worst < 1.0, (lam, n, worst)
    assert not torch.equal(runs[2.0]['v'], plain['v']) and not torch.equal(half['v'], plain['v'])
    a, _ = _step(d, t, g, lam=0.0, seed=5)
    b, _ = _step(d, t, g, lam=0.0, seed=6)
    assert torch.equal(a['v'], b['v']) and torch.equal(a['p'], b['p']) and torch.equal(a['p'], zero['p']) and torch.equal(a['v'], zero['v'])
    assert not torch.equal(a['s'], b['s'])                                             # (the seeds do differ: the types are still drawn)


# ------------------------------------------------------------------------------------------ GPU: whole loops
def _loop(d, monkeypatch, fuse, state, inputs, spec, graph=False):
    """Every slot of the trajectory buffers of one loop, run eagerly or from its captured graph, with the step's tail fused or as three launches."""
    monkeypatch.setenv('ABOPT_FUSE_STEP', '1' if fuse else '0')
    d.clear_graphs()
    out = d._denoise(spec, state, inputs, None, 11, 4096, False, graph)
    torch.cuda.synchronize()
    res = [a.clone() for a in out if a is not None]
    info = dict(d.last_run_info)
    d.clear_graphs()
    return res, info


def _same(a, b):
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), [int((x != y).sum()) for x, y in zip(a, b)]


@pytest.mark.gpu
def test_tempered_loop_fused_equals_three_launches_and_replays(monkeypatch):
    """Design flavour, N = 3, L = 40, T = 3, tau = 0.5, lambda = 0.5, device RNG: the fused tail of a step (step_tail_kernel) equals ABOPT_FUSE_STEP=0
    (denoise_step_kernel) in every slot, bit for bit; the graph replay equals the eager run; a loop whose steps carry tempered = 1 with (1, 1) equals the default loop,
    fused and unfused; a graph captured at the defaults is not served to the tempered call."""
    T = step_harness.T
    d = step_harness.model()
    v, p, s, res_feat, pair_feat, _, gen, mres = [a.to(DEV) for a in synth.eps_inputs(3, 40, [40, 33, 40], [(4, 19), (25, 31)], salt=300, num_steps=T, t=1)]
    state, inputs = (v, p * 10.0, s), (res_feat, pair_feat, gen, mres)
    plain, hot = _LoopSpec(T), _LoopSpec(T, seq_temperature=0.5, noise_scale=0.5)
    ref, info = _loop(d, monkeypatch, False, state, inputs, hot)
    got, _ = _loop(d, monkeypatch, True, state, inputs, hot)
    assert len(got) == 3 and info['steps'] == T
    _same(got, ref)
    replayed, info = _loop(d, monkeypatch, True, state, inputs, hot, graph=True)
    assert info['graph'] is True
    _same(replayed, got)
    base, _ = _loop(d, monkeypatch, True, state, inputs, plain)
    assert not torch.equal(base[0], got[0]) and not torch.equal(base[1], got[1]) and not torch.equal(base[2], got[2])
    # tempered = 1 with unit values, forced into every step of the loop: the default loop's bits, through both kernels
    params = FullDPM._step_params

    def forced(self, *args, **kw):
        sp = params(self, *args, **kw)
        sp.tempered, sp.seq_temperature, sp.noise_scale = 1, 1.0, 1.0
        return sp
    monkeypatch.setattr(FullDPM, '_step_params', forced)
    for fuse in (True, False):
        _same(_loop(d, monkeypatch, fuse, state, inputs, plain)[0], base)
    monkeypatch.setattr(FullDPM, '_step_params', params)
    # graphs: the default loop's is not the tempered loop's
    monkeypatch.setenv('ABOPT_FUSE_STEP', '1')
    d.clear_graphs()
    try:
        first = [a.clone() for a in d._denoise(plain, state, inputs, None, 11, 4096, False, True) if a is not None]
        assert d.last_run_info['graph'] is True and len(d._graphs) == 1
        second = [a.clone() for a in d._denoise(hot, state, inputs, None, 11, 4096, False, True) if a is not None]
        assert d.last_run_info['graph'] is True and len(d._graphs) == 2
        _same(first, base)
        _same(second, got)
        again = [a.clone() for a in d._denoise(plain, state, inputs, None, 11, 4096, False, True) if a is not None]
        assert len(d._graphs) == 2
        _same(again, base)
    finally:
        d.clear_graphs()


@pytest.mark.gpu
def test_sample_optimize_grouped_and_screen_carry_the_knobs():
    """model.sample with sample_opt={'seq_temperature': 0.5} differs from the default (the parent swallowed the key), and so does model.optimize; sample_replicated
    equals model.sample on the replicated batch and sample_grouped equals the per-complex sample_replicated calls at the launch's Philox offsets, with the keys in
    sample_opt; the screen with (None, None) equals the call without them in every field, runs with dock_noise_scale=0 (finite prmsd_std and redock_score spread)
    and keeps aa_allowed at design_temperature=0."""
    m = build_model(10, 3, device=DEV)
    batch = _design_batch()
    N, L = batch['aa'].shape
    opt = dict(sample_structure=True, sample_sequence=True, seed=11, graph=False)
    knobs = dict(seq_temperature=0.5, noise_scale=0.5)
    free = m.sample(dict(batch), dict(opt, contig=''))
    assert _same_traj(free, m.sample(dict(batch), dict(opt, contig='', seq_temperature=1.0, noise_scale=1.0)))
    cold = m.sample(dict(batch), dict(opt, contig='', seq_temperature=0.5))
    assert sorted(cold) == sorted(free) and not torch.equal(cold[0][2], free[0][2])
    assert torch.equal(cold[10][2].cpu(), free[10][2].cpu())                             # the initial state is not touched
    assert torch.equal(cold[9][1].cpu(), free[9][1].cpu())                               # tau alone leaves the first step's structure (and, alpha_bar_T being ~0, its types)
    assert any(not torch.equal(cold[t][2].cpu(), free[t][2].cpu()) for t in range(1, 9))
    calm = m.sample(dict(batch), dict(opt, contig='', noise_scale=0.5))
    assert not torch.equal(calm[9][1].cpu(), free[9][1].cpu()) and torch.equal(calm[9][2].cpu(), free[9][2].cpu())
    o_free, o_both = m.optimize(dict(batch), 4, dict(opt)), m.optimize(dict(batch), 4, dict(opt, **knobs))
    assert sorted(o_both) == sorted(o_free) == list(range(5)) and not _same_traj(o_free, o_both)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(o_free[4][:3], o_both[4][:3]))       # the forward noising is not touched
    # replicated: one complex, 4 samples
    c0 = {k: v[:1] for k, v in batch.items()}
    c1 = {k: v[1:2] for k, v in batch.items()}
    repl = {k: v.expand(4, *v.shape[1:]).contiguous() for k, v in c0.items()}
    rep = sampler.sample_replicated(m, dict(c0), 4, dict(opt, **knobs))
    assert _same_traj(rep, m.sample(repl, dict(opt, contig='', **knobs)))
    assert not _same_traj(rep, sampler.sample_replicated(m, dict(c0), 4, dict(opt)))
    # grouped: 2 complexes x 2 samples in one launch against one launch per complex
    grouped = sampler.sample_grouped(m, [dict(c0), dict(c1)], 2, dict(opt, rng_offset=0, **knobs))
    for gidx, c in enumerate((c0, c1)):
        single = sampler.sample_replicated(m, dict(c), 2, dict(opt, rng_offset=gidx * 2 * L, **knobs))
        for step in single:
            for a, b in zip(single[step], grouped[step]):
                assert torch.equal(a.cpu(), b[2 * gidx:2 * gidx + 2].cpu()), (gidx, step)
    # the screen
    P, S, k, D, contig, seed = 4, 3, 2, 3, '33-39', 5
    dock, design = screen_workers.models(DEV)
    one = screen_workers.complex_(DEV)
    kw = dict(contig=contig, screened_per_pose=k, seed=seed, poses_per_launch=P, screen_by='ppl')
    base = screen.optimize_antibody(dock, design, one, P, S, D, **kw)
    none = screen.optimize_antibody(dock, design, one, P, S, D, design_temperature=None, dock_noise_scale=None, **kw)
    assert sorted(base) == sorted(none)
    for name, v in base.items():
        assert torch.equal(none[name], v), name
    still = screen.optimize_antibody(dock, design, one, P, S, D, dock_noise_scale=0, **kw)
    assert sorted(still) == sorted(base) and still['prmsd_std'].shape == (P, k)
    assert bool(torch.isfinite(still['prmsd_std']).all()) and bool(torch.isfinite(still['redock_score']).all())
    assert bool(torch.isfinite(still['redock_score'].std(-1)).all()) and not torch.equal(still['pose_ca'], base['pose_ca'])
    no_c = model_.aa_allowed_mask(128, exclude='C', device=DEV)
    greedy = screen.optimize_antibody(dock, design, one, P, S, D, design_temperature=0, allowed_aa=no_c, **kw)
    assert greedy['seqs'].shape == (P, S, 7) and bool((greedy['seqs'] != 1).all()) and bool(((greedy['seqs'] >= 0) & (greedy['seqs'] < K)).all())
    assert torch.equal(greedy['pose_ca'], base['pose_ca'])                               # the docking stage draws no types: the temperature does not reach it
    with pytest.raises(ValueError, match='design_temperature'):
        screen.optimize_antibody(dock, design, one, P, S, D, design_temperature=-1, **kw)
    with pytest.raises(ValueError, match='dock_noise_scale'):
        screen.optimize_antibody(dock, design, one, P, S, D, dock_noise_scale=float('inf'), **kw)
