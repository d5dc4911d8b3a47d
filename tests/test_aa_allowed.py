"""Allowed residue types per position in the device sampler (include/abopt.h: aa_allowed; batch['aa_allowed']; screen.optimize_antibody(allowed_aa=...)).

One int32 word per residue, bit k = type k ('ACDEFGHIKLMNPQRSTVWY'[k]) may be drawn at that generated residue.  The plain fp64 statement of the constrained
posterior (`posterior_statement`) lives here; the CPU tests cover the mask builder, the refusal of an empty set, the graph key and the batch schema, the GPU tests the
three kernels directly and the mask's way through sample() / optimize(), the captured loop, the replicated / grouped samplers and the screen."""
import dataclasses

import pytest
import torch

import screen_workers
from conftest import build_model
from ab_opt_amd import hip, model as model_, sampler, screen
from ab_opt_amd.dpm import FullDPM, _LoopSpec, _graph_key
from ab_opt_amd.utils import synth

DEV = torch.device('cuda:0')
LETTERS = 'ACDEFGHIKLMNPQRSTVWY'
FULL = (1 << 20) - 1
K = 20


def bits_of(letters):
    return sum(1 << LETTERS.index(c) for c in letters)


def allowed_bits(allow):
    """(..., ) words -> (..., 20) bool."""
    return ((allow.long()[..., None] >> torch.arange(K, device=allow.device)) & 1).bool()


def obeys(s, allow, gen):
    """Every generated residue's type is in its set."""
    ok = ((allow.long() >> s.clamp(0, 62)) & 1).bool() & (s >= 0) & (s < K)
    return bool(ok[gen].all())


# ------------------------------------------------------------------------------------------ the fp64 statement
def posterior_statement(c_net, s_t, gen, allow, alpha_bar):
    """AminoacidCategoricalTransition.posterior (transition.py:166-174, alpha_bar on both factors as denoise() calls it, :202-245) restricted to the allowed types, in
    fp64: the unnormalised product of a disallowed class is 0 BEFORE the normalisation; a context residue and a generated residue with an empty set report onehot(s_t)."""
    ct = torch.zeros(*s_t.shape, K, dtype=torch.float64)
    inside = (s_t >= 0) & (s_t < K)
    ct[inside] = torch.nn.functional.one_hot(s_t[inside], K).double()
    ab = float(alpha_bar)
    unif = (1.0 - ab) / K
    raw = (ab * ct + unif) * (ab * c_net.double() + unif)
    bits = allowed_bits(allow) | ~gen[..., None]                       # the word is read on generated residues only
    raw = raw * bits
    post = raw / (raw.sum(-1, keepdim=True) + 1e-8)
    frozen = gen & ((allow.long() & FULL) == 0)
    return torch.where((gen & ~frozen)[..., None], post, ct)


def perplexity_statement(post, gen, masked):
    """calc_perplexity (dpm_full.py:380-399) of the posterior: mean over the residues (the generated ones when masked) of max softmax(post)."""
    top = torch.softmax(post, -1).max(-1)[0]
    w = gen.double() if masked else torch.ones_like(top)
    return (top * w).sum(-1) / w.sum(-1)


# ------------------------------------------------------------------------------------------ CPU
def test_aa_allowed_mask_builder():
    m = model_.aa_allowed_mask(12)
    assert m.dtype == torch.int32 and m.shape == (12,) and bool((m == FULL).all())
    for k, c in enumerate(LETTERS):                                      # letters to bits: the reference's AA enum order
        assert int(model_.aa_allowed_mask(3, at={2: c})[1]) == 1 << k
        assert int(model_.aa_allowed_mask(3, exclude=c)[0]) == FULL & ~(1 << k)
    assert model_.AA_LETTERS == LETTERS
    m = model_.aa_allowed_mask(10, exclude='CM', at={7: 'AST', 1: 'c', 10: 'Y'})
    assert m.dtype == torch.int32
    assert int(m[6]) == bits_of('AST') and int(m[0]) == bits_of('C') and int(m[9]) == bits_of('Y')       # `at` replaces the set, exclusions included; 1-based
    rest = [i for i in range(10) if i not in (0, 6, 9)]
    assert all(int(m[i]) == FULL & ~bits_of('CM') for i in rest)
    assert int(model_.aa_allowed_mask(4, exclude='cm')[0]) == FULL & ~bits_of('CM')
    for bad in (dict(exclude='B'), dict(exclude='AX'), dict(at={2: 'AZ'}), dict(at={1: 'A S'})):
        with pytest.raises(ValueError, match='unknown residue type'):
            model_.aa_allowed_mask(5, **bad)
    for pos in (0, 6):
        with pytest.raises(ValueError, match='outside 1..5'):
            model_.aa_allowed_mask(5, at={pos: 'A'})


def _cpu_inputs(N=2, L=8):
    gen = torch.zeros(N, L, dtype=torch.bool)
    gen[:, 2:5] = True
    z = torch.zeros(N, L, 3)
    return (z, z, torch.zeros(N, L, dtype=torch.long)), (torch.zeros(N, L, 128), torch.zeros(N, L, L, 64), gen, torch.ones(N, L, dtype=torch.bool))


def test_empty_allowed_set_on_a_generated_residue_is_refused():
    d = build_model(10, 3).diffusion
    (v, p, s), tail = _cpu_inputs()
    calls = {'sample': lambda a: d.sample(v, p, s, *tail, seed=1, aa_allowed=a), 'optimize': lambda a: d.optimize(v, p, s, 4, *tail, seed=1, aa_allowed=a)}
    for name, call in calls.items():
        bad = torch.full((2, 8), FULL, dtype=torch.int32)
        bad[1, 3] = 0
        with pytest.raises(ValueError, match='generated residue 4 of sample 1 has an empty set'):
            call(bad)
        bad64 = torch.full((8,), -1, dtype=torch.int64)                  # (L,) broadcast; bits 20.. do not count
        bad64[2] = 1 << 20
        with pytest.raises(ValueError, match='generated residue 3 of sample 0 has an empty set'):
            call(bad64)
        with pytest.raises(ValueError, match='aa_allowed must be'):
            call(torch.full((2, 7), FULL, dtype=torch.int32))
        with pytest.raises(TypeError, match='int32 or int64'):
            call(torch.ones(2, 8))
        ok = torch.full((1, 8), FULL, dtype=torch.int32)
        ok[0, 0] = ok[0, 7] = 0                                          # an empty word on a context residue is not looked at: the call goes on to the device
        with pytest.raises(RuntimeError, match='HIP device only'):
            call(ok)
        with pytest.raises(RuntimeError, match='HIP device only'):
            call(None)


def test_constrained_and_unconstrained_loops_have_different_graph_keys():
    (_, _, _), inputs = _cpu_inputs()
    token = object()
    free = _LoopSpec(10)
    tied = dataclasses.replace(free, constrained=True)
    assert free.constrained is False and tied != free
    a = torch.full((2, 8), FULL, dtype=torch.int32)
    b = torch.full((2, 8), bits_of('AST'), dtype=torch.int32)
    assert _graph_key(tied, inputs + (a,), token) != _graph_key(free, inputs, token)
    assert _graph_key(tied, inputs + (a,), token) == _graph_key(tied, inputs + (b,), token)       # the mask's contents are data, not key
    # sample() / optimize() / _run() say so themselves: the spec they hand to _denoise is constrained exactly when a mask is given, and the mask rides behind the inputs
    d = build_model(10, 3).diffusion
    seen = []

    class Stop(Exception):
        pass

    def denoise(self, spec, state, inputs, *args, **kw):
        seen.append((spec, inputs))
        raise Stop
    (v, p, s), tail = _cpu_inputs()
    state = lambda *args, **kw: (v, p, s)
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(FullDPM, '_denoise', denoise)
        for name, fake in (('lib', lambda: None), ('sample_init', state), ('add_noise', state), ('nonfinite_flag_reset', lambda: None)):
            mp.setattr(hip, name, fake)
        for call in (lambda m: d.sample(v, p, s, *tail, seed=1, aa_allowed=m), lambda m: d.optimize(v, p, s, 4, *tail, seed=1, aa_allowed=m),
                     lambda m: d._run((v, p, s), 7, *tail, True, True, True, None, 5, 0, False, aa_allowed=m)):
            for m in (None, b[0]):
                with pytest.raises(Stop):
                    call(m)
                spec, inputs = seen.pop()
                assert spec.constrained is (m is not None) and len(inputs) == (5 if m is not None else 4)
                if m is not None:
                    assert inputs[4].dtype == torch.int32 and inputs[4].shape == (2, 8) and bool((inputs[4] == bits_of('AST')).all())
    finally:
        mp.undo()


def test_batch_key_is_sliced_padded_and_grouped_with_the_batch():
    batch = synth.make_batch(4, synth.LAYOUT_128, seed=3, lengths=[32, 32, 32, 32])
    batch['aa_allowed'] = torch.arange(4 * 32, dtype=torch.int32).view(4, 32) + 1
    sub, (a, b) = sampler.shard_batch(batch, 2, 1)
    assert (a, b) == (2, 4) and torch.equal(sub['aa_allowed'], batch['aa_allowed'][2:4]) and sub['aa_allowed'].shape == sub['aa'].shape
    one = {k: v[:1] for k, v in batch.items()}
    padded = sampler.pad_complex(one, 40)
    assert padded['aa_allowed'].shape == (1, 40) and padded['aa_allowed'].dtype == torch.int32
    assert torch.equal(padded['aa_allowed'][:, :32], one['aa_allowed']) and bool((padded['aa_allowed'][:, 32:] == 0).all())
    assert not padded['generate_flag'][:, 32:].any()                    # padded residues are never generated: their empty word is never read


# ------------------------------------------------------------------------------------------ GPU: the three kernels, directly
_CASES = {}


def _kernel_case(N, L, skew_same=False):
    """Inputs of one direct abopt_denoise_step / abopt_sample_init / abopt_add_noise call at (N, L), built once per shape and left unchanged: t = 30 of the 100-step
    schedule, hash-filled state and network outputs, a skewed c_net (per residue, or one prediction everywhere), every fifth residue context."""
    key = (N, L, skew_same)
    if key not in _CASES:
        d = build_model(100, 2, device=DEV).diffusion
        t = 30
        c = synth.hash_tensor((1, 1, K), 9, scale=6.0).expand(N, L, K) if skew_same else synth.hash_tensor((N, L, K), 11, scale=6.0)
        gen = torch.ones(N, L, dtype=torch.bool)
        gen[:, ::5] = False
        s_t = torch.full((N, L), 7, dtype=torch.int64) if skew_same else (synth.hash_tensor((N, L), 12) + 0.5).mul(K).long().clamp(0, K - 1)
        cpu = dict(v=synth.hash_tensor((N, L, 3), 13, scale=2.0), p=synth.hash_tensor((N, L, 3), 14, scale=30.0), s=s_t, gen=gen,
                   v_net=synth.hash_tensor((N, L, 3), 15, scale=0.5), p_net=synth.hash_tensor((N, L, 3), 16), c_net=torch.softmax(c, -1).contiguous())
        _CASES[key] = (d, t, cpu, {k: v.to(DEV) for k, v in cpu.items()})
    return _CASES[key]


def _step(d, t, g, allow, seed=99, ppl_masked=True):
    N, L = g['gen'].shape
    sp = d._step_params(t, True, True, ppl_masked)
    inv = d.trans_rot.angular_distrib_inv
    out = dict(v=torch.empty(N, L, 3, device=DEV), p=torch.empty(N, L, 3, device=DEV), s=torch.empty(N, L, dtype=torch.int64, device=DEV),
               prmsd=torch.empty(N, device=DEV), ppl=torch.empty(N, device=DEV), p_norm=torch.empty(N, L, 3, device=DEV))
    out['post'] = hip.denoise_step(sp, None, seed, 0, g['v'], g['p'], g['s'], g['v_net'], g['p_net'], g['c_net'], torch.zeros(N, 40, device=DEV), g['gen'],
                                   inv.X[t], inv.cdf()[t], 40, out, want_post=True, aa_allowed=allow)
    return out, sp


def _init(g, allow, seed=99):
    return hip.sample_init(g['v'], g['p'], g['s'], g['gen'], None, seed, 0, 10.0, [0.0, 0.0, 0.0], True, True, aa_allowed=allow)


def _noised(d, g, allow, seed=99, opt_step=60):
    tt = torch.full([g['gen'].shape[0]], opt_step, dtype=torch.long, device=DEV)
    return hip.add_noise(tt, d.trans_pos.var_sched.alpha_bars, d.trans_rot.angular_distrib_fwd, None, seed, 0, g['v'], g['p'], g['s'], g['gen'], 10.0, [0.0, 0.0, 0.0],
                         want_eps=True, want_probs=True, aa_allowed=allow)


def _words(N, L, value):
    return torch.full((N, L), value, dtype=torch.int32, device=DEV)


@pytest.mark.gpu
def test_full_and_null_masks_are_bit_identical():
    """N = 3, L = 300 (the 256-thread stride loop and a ragged last wave): no mask, 0xFFFFF everywhere and -1 everywhere give the same bits in every output of the
    step (device RNG, posterior included), of the initial state and of the forward noising."""
    N, L = 3, 300
    d, t, _, g = _kernel_case(N, L)
    runs = []
    for allow in (None, _words(N, L, FULL), _words(N, L, -1)):
        step, _ = _step(d, t, g, allow)
        runs.append([step[k] for k in ('v', 'p', 's', 'prmsd', 'ppl', 'p_norm', 'post')] + list(_init(g, allow)) + list(_noised(d, g, allow)))
    assert len(runs[0]) == 7 + 3 + 5
    for other in runs[1:]:
        for i, (a, b) in enumerate(zip(runs[0], other)):
            assert torch.equal(a, b), i
    assert not torch.equal(runs[0][2], g['s']) and not torch.equal(runs[0][9], g['s'])       # (types were drawn at all)


@pytest.mark.gpu
def test_constrained_posterior_vs_fp64_statement():
    """post_out and the perplexity of a constrained step against the fp64 statement at N = 3, L = 300, skewed c_net per residue.  Masks: random non-empty words, then by
    residue index mod 7 -- single-type sets, sets without s_t, sets without the argmax of c_net -- a few empty words on generated residues (through the raw binding: the
    type is frozen, the posterior onehot(s_t)) and arbitrary words, empty ones among them, on context residues (untouched).
    Tolerances are the project's own for the unconstrained quantities: 2e-6 on the posterior (test_categorical_posterior_on_device_vs_reference) and 1e-5 on the
    perplexity (test_structure_only_steps_teacher_forced_vs_reference) -- the constrained posterior is the same fp32 expression over fewer terms."""
    N, L = 3, 300
    d, t, cpu, g = _kernel_case(N, L)
    gen, s_t = cpu['gen'], cpu['s']
    rs = torch.Generator().manual_seed(4)
    allow = torch.randint(1, FULL + 1, (N, L), generator=rs)
    idx = torch.arange(N * L).view(N, L)
    single = idx % 7 == 1
    allow[single] = (1 << torch.randint(0, K, (N, L), generator=rs))[single]
    no_st = idx % 7 == 2
    allow[no_st] &= ~(1 << s_t)[no_st]
    no_top = idx % 7 == 3
    allow[no_top] &= ~(1 << cpu['c_net'].argmax(-1))[no_top]
    allow[allow == 0] = bits_of('GP')
    empty = gen & (idx % 41 == 6)
    allow[empty] = 0
    allow[0, 0] = 0                                                         # context residues (every fifth): never read
    allow[1, 5] = 1 << 25
    assert int(empty.sum()) >= 5 and not gen[0, 0] and not gen[1, 5] and bool((single & gen).any() and (no_st & gen).any() and (no_top & gen).any())
    word = allow.to(torch.int32).to(DEV)
    for masked in (True, False):
        out, sp = _step(d, t, g, word, ppl_masked=masked)
        want = posterior_statement(cpu['c_net'], s_t, gen, allow, sp.alpha_bar)
        post, s_next = out['post'].cpu(), out['s'].cpu()
        err = (post.double() - want).abs().max().item()
        ppl_err = (out['ppl'].cpu().double() - perplexity_statement(want, gen, masked)).abs().max().item()
        print(f'constrained posterior: max abs error {err:.3g}, perplexity error {ppl_err:.3g} (ppl_masked={masked})')
        assert err < 2e-6
        assert ppl_err < 1e-5
        onehot = torch.nn.functional.one_hot(s_t, K).float()
        assert torch.equal(post[empty], onehot[empty]) and torch.equal(s_next[empty], s_t[empty])          # frozen
        assert torch.equal(post[~gen], onehot[~gen]) and torch.equal(s_next[~gen], s_t[~gen])              # context
        assert bool((post[~allowed_bits(allow) & gen[..., None] & ~empty[..., None]] == 0).all())          # exactly zero, not small
        live = gen & ~empty
        assert obeys(s_next, allow, live)
        assert torch.equal(s_next[single & live], allow[single & live].log2().round().long())
    # the structure of a frozen residue still moves, exactly as without the mask
    free, _ = _step(d, t, g, None)
    assert torch.equal(out['v'], free['v']) and torch.equal(out['p'], free['p']) and not torch.equal(out['v'].cpu()[empty], cpu['v'][empty])


def _chi2_ok(draws, prob, n):
    """The rule of test_sequence_sampler_draws_from_the_posterior: per-class chi-square over the classes with expectation > 10, bound 3 x their count."""
    freq = torch.zeros(K, dtype=torch.float64).scatter_add_(0, draws, torch.ones(n, dtype=torch.float64))
    exp = prob.double() * n
    keep = exp > 10
    chi2 = (((freq - exp) ** 2 / exp)[keep]).sum().item()
    print(f'chi2 {chi2:.2f} over {int(keep.sum())} classes')
    return chi2 < 3 * int(keep.sum()) and freq[~keep].sum() <= 10 * (~keep).sum() + 20 and int(keep.sum()) >= 2


@pytest.mark.gpu
def test_no_disallowed_type_is_ever_drawn():
    """N = 64, L = 256, one skewed prediction everywhere (the setup of test_sequence_sampler_draws_from_the_posterior), the set without the two most probable classes:
    every generated s_next is in the set and follows post_out (that test's chi-square rule, fixed seed); a single-type set gives that type on every generated row (the
    walk's fall-through included); sample_init is uniform over allowed types among 0..18 and gives 19 for {Y}; add_noise draws from the set."""
    N, L = 64, 256
    d, t, cpu, g = _kernel_case(N, L, skew_same=True)
    gen, n = cpu['gen'], int(cpu['gen'].sum())
    free, sp = _step(d, t, g, None)
    top2 = free['post'][g['gen']][0].topk(2)[1].tolist()
    allow_val = FULL & ~(1 << top2[0]) & ~(1 << top2[1])
    assert 7 in top2                                                        # s_t itself is one of them: the set excludes s_t
    out, _ = _step(d, t, g, _words(N, L, allow_val))
    s_next = out['s'].cpu()
    assert obeys(s_next, torch.full((N, L), allow_val), gen) and torch.equal(s_next[~gen], cpu['s'][~gen])
    pg = out['post'][g['gen']][0].cpu()
    assert pg[top2[0]] == 0 and pg[top2[1]] == 0 and abs(pg.sum().item() - 1) < 1e-5
    assert _chi2_ok(s_next[gen], pg, n)
    for only in (0, 12, 19):
        out, _ = _step(d, t, g, _words(N, L, 1 << only))
        assert bool((out['s'].cpu()[gen] == only).all())
        assert bool((_noised(d, g, _words(N, L, 1 << only))[2].cpu()[gen] == only).all())
    # initial state: uniform over allowed & 0..18 (TYR is never drawn while anything else is allowed), {Y} alone gives 19
    s_init = _init(g, _words(N, L, allow_val))[2].cpu()
    assert obeys(s_init, torch.full((N, L), allow_val & (FULL >> 1)), gen) and torch.equal(s_init[~gen], cpu['s'][~gen])
    low = allowed_bits(torch.tensor(allow_val & (FULL >> 1))).double()
    assert _chi2_ok(s_init[gen], low / low.sum(), n)
    assert bool((_init(g, _words(N, L, 1 << 19))[2].cpu()[gen] == 19).all())
    assert bool((_init(g, _words(N, L, bits_of('WY')))[2].cpu()[gen] == 18).all())
    # forward noising (optimize): the draw stays in the set, c_noisy is the reference's unconstrained c_t
    noisy, unmasked = _noised(d, g, _words(N, L, allow_val)), _noised(d, g, None)
    assert obeys(noisy[2].cpu(), torch.full((N, L), allow_val), gen) and torch.equal(noisy[4], unmasked[4])
    ct = noisy[4][g['gen']][0].cpu().double() * allowed_bits(torch.tensor(allow_val))
    assert _chi2_ok(noisy[2].cpu()[gen], ct / ct.sum(), n)


# ------------------------------------------------------------------------------------------ GPU: through the model
def _design_batch(N=4, L=32, seed=3, lengths=None):
    """N complexes of LAYOUT_128 cut to L residues, residues 9..20 (1-based) generated."""
    batch = synth.make_batch(N, synth.LAYOUT_128, seed=seed, lengths=lengths or [L] * N)
    gen = torch.zeros_like(batch['generate_flag'])
    gen[:, 8:20] = True
    batch['generate_flag'] = gen & batch['mask']
    return {k: v.to(DEV) for k, v in batch.items()}


def _mask_cm_ast(N, L, pin=12):
    return model_.aa_allowed_mask(L, exclude='CM', at={pin: 'AST'}, device=DEV)[None].expand(N, L).contiguous()


def _same_traj(a, b):
    return sorted(a) == sorted(b) and all(len(a[t]) == len(b[t]) and all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a[t], b[t])) for t in a)


def _traj_obeys(traj, allow, gen, aa, real=None):
    """Every state of the trajectory: allowed types on the generated residues, the input types on the context residues (`real`: the batch's residue mask -- the type of
    a padded residue is a draw from an all-zero row in the reference too, transition.py:241-244)."""
    allow, gen, aa = allow.cpu(), gen.cpu(), aa.cpu()
    ctx = ~gen if real is None else ~gen & real.cpu()
    return all(obeys(e[2].cpu(), allow, gen) and torch.equal(e[2].cpu()[ctx], aa[ctx]) for e in traj.values())


@pytest.mark.gpu
@pytest.mark.parametrize('flavour', ['abdock', 'abdesign'])
def test_sample_and_optimize_obey_the_mask_end_to_end(flavour):
    """model.sample and model.optimize(opt_step=4) at T = 10, N = 4, L = 32 (the session's 10-step model) with batch['aa_allowed'] = no C, no M, position 12 one of
    A/S/T: every state of the trajectory, the initial one included, holds allowed types on the generated residues and the input types elsewhere; without the key the
    trajectory equals the one of an all-allowing mask under the same seed, bit for bit."""
    m = build_model(10, 3, flavour, device=DEV)
    batch = _design_batch()
    N, L = batch['aa'].shape
    allow = _mask_cm_ast(N, L)
    opt = dict(sample_structure=True, sample_sequence=True, seed=11, graph=False)
    runs = {'sample': lambda b: m.sample(b, dict(opt, contig='')), 'optimize': lambda b: m.optimize(b, 4, dict(opt))}
    for name, run in runs.items():
        traj = run(dict(batch, aa_allowed=allow))
        assert sorted(traj) == list(range(11 if name == 'sample' else 5))
        assert _traj_obeys(traj, allow, batch['generate_flag'], batch['aa']), name
        pinned = torch.stack([e[2].cpu()[:, 11] for e in traj.values()])
        assert bool(((pinned == 0) | (pinned == 15) | (pinned == 16)).all())
        free = run(dict(batch))
        assert not _traj_obeys(free, allow, batch['generate_flag'], batch['aa']), name         # the unconstrained run does draw forbidden types here
        assert _same_traj(free, run(dict(batch, aa_allowed=torch.full_like(allow, FULL)))), name
        assert _same_traj(free, run(dict(batch, aa_allowed=torch.full((N, L), -1, dtype=torch.int64, device=DEV)))), name
    if flavour == 'abdock':                                                                     # with a contig the set applies to the residues that stay generated
        b = dict(batch, aa_allowed=allow)
        traj = m.sample(b, dict(opt, contig='11-14'))
        assert int(b['generate_flag'].sum()) == 4 * N and _traj_obeys(traj, allow, b['generate_flag'], batch['aa'])


@pytest.mark.gpu
def test_graph_replay_follows_the_mask_it_is_given():
    """The captured loop takes the mask as an input: captured with mask A and replayed with mask B under the same seed it obeys B and equals the eager run with B bit for
    bit; an unconstrained call afterwards gets a loop of its own (another key) and equals the unconstrained eager run."""
    m = build_model(10, 3, device=DEV)
    d = m.diffusion
    batch = _design_batch()
    N, L = batch['aa'].shape
    A, B = _mask_cm_ast(N, L), model_.aa_allowed_mask(L, exclude='ACDEFGHIKL', at={10: 'W'}, device=DEV)[None].expand(N, L).contiguous()
    run = lambda graph, **kw: m.sample(dict(batch, **kw), dict(sample_structure=True, sample_sequence=True, contig='', seed=11, graph=graph))
    d.clear_graphs()
    try:
        first = run(True, aa_allowed=A)
        assert d.last_run_info['graph'] is True and len(d._graphs) == 1
        assert _traj_obeys(first, A, batch['generate_flag'], batch['aa']) and _same_traj(first, run(False, aa_allowed=A))
        replay = run(True, aa_allowed=B)
        assert d.last_run_info['graph'] is True and len(d._graphs) == 1                        # the same captured loop
        assert _traj_obeys(replay, B, batch['generate_flag'], batch['aa']) and not _traj_obeys(replay, A, batch['generate_flag'], batch['aa'])
        assert _same_traj(replay, run(False, aa_allowed=B))
        free = run(True)
        assert d.last_run_info['graph'] is True and len(d._graphs) == 2
        assert _same_traj(free, run(False)) and not _same_traj(free, replay)
        assert _same_traj(run(True, aa_allowed=A), first)                                      # and the constrained loop is still served, with the mask it is given
    finally:
        d.clear_graphs()


@pytest.mark.gpu
def test_grouped_replicated_and_screen_carry_the_mask():
    """sample_replicated (N = 4) and sample_grouped (2 complexes x 2, the second shorter and padded, masks per complex, one complex without a mask) obey the masks of
    their complexes; screen.optimize_antibody(allowed_aa = no C) at the size of test_optimize_antibody_equals_the_composition_of_public_calls returns designs without C
    whose re-docked sequences (aar's recount) follow them, and allowed_aa=None equals an all-allowing mask in every result field."""
    m = build_model(10, 3, device=DEV)
    opt = dict(sample_structure=True, sample_sequence=True, seed=5, graph=False)
    batch = _design_batch(2, 32, lengths=[32, 27])
    c0 = {k: v[:1] for k, v in batch.items()}
    c1 = {k: v[1:2, :27] for k, v in batch.items()}
    a0 = model_.aa_allowed_mask(32, exclude='CM', at={12: 'AST'}, device=DEV)[None]
    a1 = model_.aa_allowed_mask(27, exclude='ACDEFGHIKLMN', device=DEV)[None]
    traj = sampler.sample_replicated(m, dict(c0, aa_allowed=a0), 4, dict(opt))
    assert _traj_obeys(traj, a0.expand(4, 32), c0['generate_flag'].expand(4, 32), c0['aa'].expand(4, 32))
    assert _same_traj(sampler.sample_replicated(m, dict(c0), 4, dict(opt)), sampler.sample_replicated(m, dict(c0, aa_allowed=torch.full_like(a0, -1)), 4, dict(opt)))
    pad = lambda t, v: torch.cat([t, t.new_full((1, 5), v)], 1)
    gen = torch.cat([c0['generate_flag'], pad(c1['generate_flag'], False)]).repeat_interleave(2, 0)
    aa = torch.cat([c0['aa'], pad(c1['aa'], 21)]).repeat_interleave(2, 0)
    real = torch.cat([c0['mask'], pad(c1['mask'], False)]).repeat_interleave(2, 0)
    for masks in ((a0, a1), (None, a1)):
        cx = [dict(c, **({} if a is None else dict(aa_allowed=a))) for c, a in zip((c0, c1), masks)]
        traj = sampler.sample_grouped(m, cx, 2, dict(opt), optimize_step=4)
        allow = torch.cat([torch.full_like(a0, FULL) if masks[0] is None else a0, pad(a1, 0)]).repeat_interleave(2, 0)
        assert traj[0][2].shape == (4, 32) and _traj_obeys(traj, allow, gen, aa, real)
    # the screen
    P, S, k, D, contig, seed = 4, 3, 2, 3, '33-39', 5
    dock, design = screen_workers.models(DEV)
    one = screen_workers.complex_(DEV)
    kw = dict(contig=contig, screened_per_pose=k, seed=seed, poses_per_launch=P, screen_by='ppl')
    no_c = model_.aa_allowed_mask(128, exclude='C', device=DEV)
    res = screen.optimize_antibody(dock, design, one, P, S, D, allowed_aa=no_c, **kw)
    assert res['seqs'].shape == (P, S, 7) and bool((res['seqs'] != 1).all()) and bool(((res['seqs'] >= 0) & (res['seqs'] < K)).all())
    dflag = screen.design_mask(one['generate_flag'][0], contig)
    assert torch.equal(res['aar'], (res['seqs'] == one['aa'][0][dflag]).sum(-1).float() / 7)                 # aar: recovery of the input sequence, as ever
    free = screen.optimize_antibody(dock, design, one, P, S, D, **kw)
    full = screen.optimize_antibody(dock, design, one, P, S, D, allowed_aa=torch.full((128,), FULL, dtype=torch.int32), **kw)
    assert sorted(free) == sorted(full) == sorted(res)
    for name, v in free.items():
        assert torch.equal(full[name], v), name
