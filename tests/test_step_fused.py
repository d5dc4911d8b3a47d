"""The fused tail of a denoising step (csrc/heads.hip: step_tail_kernel behind abopt_eps_net_step): the heads, the step's transitions and the
next evaluation's mixer in one launch must give, bit for bit, what the three launches give (ABOPT_FUSE_STEP=0: heads_mlp_kernel, denoise_step_kernel, mixer_kernel) --
over whole loops, where a wrong carry (the mixer output left in the workspace for the next step) shows from the second step on, and through the entry itself."""
import pytest
import torch

from ab_opt_amd import hip
from ab_opt_amd.dpm import FullDPM, _LoopSpec
from ab_opt_amd.utils import synth

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
T = 4


def _dpm(abdesign):
    m = FullDPM(128, 64, num_steps=T, eps_net_opt=dict(num_layers=2), _abdesign=abdesign).eval()
    return synth.fill_module_(m, seed=3).to(DEV)


@pytest.fixture(scope='module')
def design():
    return _dpm(True)


@pytest.fixture(scope='module')
def dock():
    return _dpm(False)


def _inputs(N, L, lengths, gen_ranges, salt):
    v, p, s, res_feat, pair_feat, _, gen, mres = [a.to(DEV) for a in synth.eps_inputs(N, L, lengths, gen_ranges, salt=salt, num_steps=T, t=1)]
    return (v, p * 10.0, s), res_feat, pair_feat, gen, mres          # s: 0..20 and 21 on padding, as a batch has them


def _noise(N, L, salt):
    h = lambda shape, k, scale=1.0, offset=0.0: synth.hash_tensor(shape, salt + k, scale=scale, offset=offset).to(DEV)
    return {t: dict(axis=h((N, L, 3), 10 * t, 2.0), bin=(h((N, L), 10 * t + 1) + 0.5).mul(8190).long().clamp(0, 8190), ubin=(h((N, L), 10 * t + 2) + 0.5).clamp(0, 0.999),
                    gauss=h((N, L), 10 * t + 3, 2.0), z=h((N, L, 3), 10 * t + 4, 2.0), s_next=(h((N, L), 10 * t + 5) + 0.5).mul(20).long().clamp(0, 19)) for t in range(T, 0, -1)}


def _loop(dpm, monkeypatch, fuse, state, res_feat, pair_feat, gen, mres, spec, noise=None, aa_allowed=None, graph=False):
    monkeypatch.setenv('ABOPT_FUSE_STEP', '1' if fuse else '0')
    dpm.clear_graphs()
    inputs = dpm._inputs(res_feat, pair_feat, gen, mres, aa_allowed)
    out = dpm._denoise(spec, state, inputs, noise, 11, 4096, False, graph)
    torch.cuda.synchronize()
    steps = dpm.last_run_info['steps']
    res = [a[a.shape[0] - 1 - steps:].clone() for a in out if a is not None]      # slot K the start ... the slot of the last step taken (a stop_after cut leaves the rest unwritten)
    dpm.clear_graphs()
    return res


def _same(a, b):
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), [int((x != y).sum()) for x, y in zip(a, b)]


CASES = {
    'straddling_and_partial_workgroups': dict(N=3, L=40, lengths=[40, 33, 40], gen=[(4, 19), (25, 31)]),
    'ragged_mask_generate_not_a_prefix': dict(N=2, L=64, lengths=[64, 50], gen=[(5, 12), (30, 41)]),
    'stop_after_one_step': dict(N=2, L=64, lengths=[64, 64], gen=[(8, 40)], spec=dict(stop_after=1)),
    'respaced': dict(N=2, L=40, lengths=[40, 36], gen=[(3, 30)], spec=dict(timesteps=(4, 2, 1))),
    'sequence_fixed': dict(N=2, L=40, lengths=[40, 36], gen=[(3, 30)], spec=dict(sample_sequence=False)),
    'structure_fixed': dict(N=2, L=40, lengths=[40, 36], gen=[(3, 30)], spec=dict(sample_structure=False)),
    'aa_allowed_with_a_frozen_residue': dict(N=2, L=40, lengths=[40, 36], gen=[(3, 30)], allowed=True),
    'injected_noise': dict(N=3, L=40, lengths=[40, 33, 40], gen=[(4, 19), (25, 31)], noise=True),
}


@pytest.mark.parametrize('name', list(CASES))
def test_fused_step_loop_is_bit_identical_to_three_launches(design, monkeypatch, name):
    """Every slot of tv, tp, ts of an eager loop over all T = 4 steps (the step that lands on 0 included: no noise, no bin search), fused against ABOPT_FUSE_STEP=0."""
    c = CASES[name]
    N, L = c['N'], c['L']
    state, res_feat, pair_feat, gen, mres = _inputs(N, L, c['lengths'], c['gen'], salt=300)
    allowed = None
    if c.get('allowed'):
        allowed = torch.full((N, L), 0xFFFFF, dtype=torch.int32, device=DEV)
        allowed[:, 3:12] = 0b1010_0110_0001_0000_1001          # a few types only
        allowed[:, 12] = 0                                   # frozen
        allowed[:, 13] = 1 << 19                              # one type
    spec = _LoopSpec(T, constrained=allowed is not None, **c.get('spec', {}))
    noise = _noise(N, L, 700) if c.get('noise') else None
    ref = _loop(design, monkeypatch, False, state, res_feat, pair_feat, gen, mres, spec, noise, allowed)
    got = _loop(design, monkeypatch, True, state, res_feat, pair_feat, gen, mres, spec, noise, allowed)
    assert len(got) == 3
    _same(got, ref)
    assert got[0].shape[0] - 1 == (1 if name == 'stop_after_one_step' else 3 if name == 'respaced' else T)
    assert not torch.equal(got[0][0], got[0][-1]) or not spec.sample_structure          # the loop moved the state
    assert not torch.equal(got[2][0], got[2][-1]) or not spec.sample_sequence


def test_fused_step_loop_replayed_from_a_graph(design, monkeypatch):
    state, res_feat, pair_feat, gen, mres = _inputs(3, 40, [40, 33, 40], [(4, 19), (25, 31)], salt=300)
    spec = _LoopSpec(T)
    eager = _loop(design, monkeypatch, True, state, res_feat, pair_feat, gen, mres, spec)
    graph = _loop(design, monkeypatch, True, state, res_feat, pair_feat, gen, mres, spec, graph=True)
    assert design.last_run_info['graph']
    _same(graph, eager)


def test_abdock_loop_takes_the_unfused_form_of_the_entry(dock, monkeypatch):
    """prmsd and perplexity are per-sample reductions: the AbDock flavour keeps the three launches behind abopt_eps_net_step, whatever the switch says."""
    state, res_feat, pair_feat, gen, mres = _inputs(3, 40, [40, 33, 40], [(4, 19), (25, 31)], salt=300)
    spec = _LoopSpec(T)
    ref = _loop(dock, monkeypatch, False, state, res_feat, pair_feat, gen, mres, spec)
    got = _loop(dock, monkeypatch, True, state, res_feat, pair_feat, gen, mres, spec)
    assert len(got) == 5
    _same(got, ref)


@pytest.mark.parametrize('injected', [False, True])
def test_step_entry_equals_forward_then_denoise_step(design, monkeypatch, injected):
    """abopt_eps_net_step(carry_in=0, carry_out=0) against abopt_eps_net_forward followed by abopt_denoise_step on the same inputs: every output, post_out and
    p_next_norm included."""
    monkeypatch.setenv('ABOPT_FUSE_STEP', '1')
    N, L, t = 3, 40, 3
    (v, p, s), res_feat, pair_feat, gen, mres = _inputs(N, L, [40, 33, 40], [(4, 19), (25, 31)], salt=300)
    d = design
    ew = d.eps_net.packed()
    beta = d.trans_pos.var_sched.betas[t].expand(N).contiguous()
    p_norm = ((p - d.position_mean) / d.position_scale).contiguous()
    X, cdf = d._loop_tables(d._loop_steps(_LoopSpec(T)))
    j = T - t
    sp = d._step_params(t, True, True, True, False, t - 1)
    noise = _noise(N, L, 700)[t] if injected else None
    f32 = dict(dtype=torch.float32, device=DEV)

    def outs():
        return dict(v=torch.empty(N, L, 3, **f32), p=torch.empty(N, L, 3, **f32), s=torch.empty(N, L, dtype=torch.int64, device=DEV), p_norm=torch.empty(N, L, 3, **f32))
    net_a = hip.eps_net_forward(ew, v, p_norm, s, res_feat, pair_feat, beta, gen, mres, False, d.num_bins)
    out_a = outs()
    post_a = hip.denoise_step(sp, noise, 11, 4096, v, p, s, net_a['v_next'], net_a['eps_pos'], net_a['c'], None, gen, X[j], None if injected else cdf[j], d.num_bins, out_a,
                              want_post=True)
    net_b = {k: (torch.empty_like(a) if a is not None else None) for k, a in net_a.items()}
    out_b = outs()
    post_b = hip.eps_net_step(ew, v, p_norm, s, res_feat, pair_feat, beta, gen, mres, d.num_bins, net_b, sp, noise, 11, 4096, p, X[j], None if injected else cdf[j], out_b,
                              want_post=True)
    torch.cuda.synchronize()
    for k in ('v_next', 'R_next', 'eps_pos', 'c'):
        assert torch.equal(net_a[k], net_b[k]), k
    for k in out_a:
        assert torch.equal(out_a[k], out_b[k]), k
    assert torch.equal(post_a, post_b)
    assert not torch.equal(out_a['s'], s)
