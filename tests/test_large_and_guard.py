"""Where an address stops fitting in 32 bits, and what a model object is worth after its fp16 range guard has fired (findings 1, 3, 5).
Needs an MI355X; the >4 GB test needs about 45 GB of free device memory and skips, with the numbers, only below that."""
import copy
import pickle
import warnings

import pytest
import torch

from conftest import max_abs
from ab_opt_amd.utils import synth
from test_hip_parity import DEV, dev, _block_on_device, _rand_eps_inputs

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ the bias cache above 4 GB
def test_pair_bias_cache_slab_above_4GB(monkeypatch):
    """One GABlock over N = 1504 DISTINCT samples of L = 256 through the cached path (hip.ga_block_forward_cached) against the uncached
    one (bit for bit, whole batch) and against the oracle (8 samples, 3e-5 as test_ga_block_bench_geometry_vs_oracle at the same input scales).

    The cached 16-row kernels read a row's bias of key chunk ch at byte  ch * (N * L * 768) + row * 768 + lane offset  of the layer's
    chunk-major slab (csrc/ipa_core.hip: pb_chunk).  nchunk = 16 at L = 256, so
        the slab passes 2^32 bytes from           N >= 2^32 / (16 * 256 * 768) = 1365.3   (the 32-row kernel stands aside from there: plan_ipa_core)
        chunk 15 starts beyond 2^32 for ALL rows  N >= 2^32 / (15 * 256 * 768) = 1456.4
    N = 1504: chunk 15 of every sample starts at byte 4,435,476,480 (140 MB of margin) and chunk 14 lies beyond 2^32 from sample 790 on.
    A 32-bit product wraps INSIDE the allocation and reads another row's bias (every sample has its own z).  N % 8 == 0 selects the XCD-aware block
    mapping (xcd_remap = 1); N * 16 query blocks > CUs selects ipa_core_persist_kernel on the cached side, the one-block kernel with the bias
    computed in place on the uncached side."""
    from ab_opt_amd import hip
    from oracle import ipa, geometry as G
    N, L = 1504, 256
    nchunk = (L + 15) // 16
    assert (nchunk - 1) * N * L * 768 >= (1 << 32) + (64 << 20) and not hip.pair_terms_used(N, L)
    z_bytes, cache_bytes, ws_bytes = N * L * L * 64 * 4, hip.pair_bias_cache_bytes(N, L, 1), hip.lib().abopt_ga_workspace_bytes(N, L, 128, 64)
    assert cache_bytes == N * L * nchunk * 768 > (1 << 32)
    need = z_bytes + cache_bytes + ws_bytes + 8 * N * L * 128 * 4             # + x, three outputs, R / t / v and slack
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(DEV)[0]
    print(f'slab test: need {need / 2**30:.1f} GiB (z {z_bytes / 2**30:.1f}, cache {cache_bytes / 2**30:.1f}, workspace {ws_bytes / 2**30:.1f}), free {free / 2**30:.1f} GiB')
    if free < need * 1.25:
        pytest.skip(f'needs {need * 1.25 / 2**30:.1f} GiB of free device memory (1.25 x {need / 2**30:.1f}), {free / 2**30:.1f} GiB are free')
    monkeypatch.setenv('ABOPT_CORE_NO_SPLIT', '1')                             # the pin of test_pair_bias_cache_is_bit_identical: same kernel form on both sides
    blk = _block_on_device(seed=5)
    sd = {k: v.cpu() for k, v in blk.state_dict().items()}
    _, ws = blk.packed()
    lengths = [256, 250, 256, 231, 256, 256, 17, 256] * (N // 8)             # ragged: samples 1, 3, 6 (mod 8)
    gtor = torch.Generator(device=DEV).manual_seed(9100)
    r = lambda *shape, s=1.0: torch.randn(*shape, device=DEV, generator=gtor) * s
    mask = dev(synth.mask_from_lengths(lengths, L))
    v, t, x = r(N, L, 3, s=1.5), r(N, L, 3, s=2.0), r(N, L, 128)
    R = dev(G.so3_exp(v.cpu()))
    ids = [0, 377, 751, 1125, 1435, 1470, 1497, 1503]                        # 4 of 8 in the last 5 % (>= 1429); lengths 256 250 256 256 231 17 250 256
    z = cache = plain = cached = auto = None
    try:
        z = torch.empty(N, L, L, 64, device=DEV)
        for lo in range(0, N, 94):                                            # generated on the device, every sample its own values
            z[lo:lo + 94].normal_(generator=gtor)
        cache = hip.pair_bias_cache_layers([blk.proj_pair_bias.weight], z)[0]
        assert cache.numel() * 4 == cache_bytes
        plain = hip.ga_block_forward(ws, R, t, x, z, mask)
        cached = hip.ga_block_forward_cached(ws, R, t, x, z, mask, cache)
        monkeypatch.delenv('ABOPT_CORE_NO_SPLIT')                             # ... and the form the library picks by itself
        auto = hip.ga_block_forward_cached(ws, R, t, x, z, mask, cache)
        torch.cuda.synchronize()
        ix = torch.tensor(ids, device=DEV)
        ref = ipa.ga_block(sd, '', R[ix].cpu(), t[ix].cpu(), x[ix].cpu(), z[ix].cpu(), mask[ix].cpu(), mode='mm')
        errs = {}
        for name, out in (('uncached', plain), ('cached', cached), ('cached, own choice', auto)):
            assert torch.isfinite(out).all(), name
            errs[name] = {i: max_abs(out[i].cpu(), ref[k]) for k, i in enumerate(ids)}
            print(f'slab test: {name}: max abs error vs oracle per sample ' + ', '.join(f'{i}: {e:.2e}' for i, e in errs[name].items()))
        per = (cached - plain).abs().amax((1, 2))
        bad = torch.nonzero(per > 0).flatten()
        print(f'slab test: {bad.numel()} of {N} samples differ between the cached and the uncached block; worst max abs {per.max().item():.3e}')
        # (i) the whole batch, bit for bit
        assert bad.numel() == 0 and torch.equal(cached, plain), \
            f'{bad.numel()} of {N} samples differ between the cached and the uncached block; first {int(bad[0])} (max abs {per[bad[0]].item():.3e}), worst {int(per.argmax())} ({per.max().item():.3e})'
        # (ii) absolute, so that two equally wrong paths cannot agree; (iii) ragged lengths are among the checked samples
        for name, e in errs.items():
            assert max(e.values()) < 3e-5, (name, e)
    finally:
        del z, cache, plain, cached, auto
        hip.Workspace._bufs.clear()
        torch.cuda.empty_cache()


def test_dispatch_on_either_side_of_the_32_bit_limits(monkeypatch):
    """abopt_pair_terms_used is the dispatcher's choice of the 32-row kernels, whose single buffer descriptor reaches 4 GB of bias cache and whose z descriptors
    reach L = 2048: with ABOPT_CORE32=1 (whenever it can) the answer flips exactly at 1365 | 1366 distinct samples of L = 256 and at L = 2048 | 2049; with shared
    pair features the DISTINCT entries count."""
    from ab_opt_amd import hip
    monkeypatch.setenv('ABOPT_CORE32', '1')
    assert 1365 * 256 * 16 * 768 < (1 << 32) <= 1366 * 256 * 16 * 768
    assert hip.pair_terms_used(1365, 256) and not hip.pair_terms_used(1366, 256) and not hip.pair_terms_used(3000, 256)
    assert hip.pair_terms_used(1, 2048) and not hip.pair_terms_used(1, 2049)
    assert hip.pair_terms_used(3000, 256, pair_feat_shared=3) and not hip.pair_terms_used(1366 * 2, 256, pair_feat_shared=2)
    monkeypatch.delenv('ABOPT_CORE32')
    assert not hip.pair_terms_used(1366, 256) and not hip.pair_terms_used(3000, 256) and not hip.pair_terms_used(1, 2049)


# ------------------------------------------------------------------------------------------ range-guard lifecycle
def _guard_case(seed=5100):
    T, N, L = 10, 2, 48
    m = synth.fresh_model(T, 3, device=DEV)
    v, p, s, rf, pf, gen, mres = _rand_eps_inputs(N, L, [48, 40], seed, [(6, 17), (30, 37)])
    beta = m.diffusion.trans_pos.var_sched.betas[7].expand([N]).contiguous()
    big = rf * (1.0e5 / rf.abs().max())                                        # the oversized res_feat of test_fp16_range_guard_falls_back_to_fp32_layers
    return m, (v, p, s, rf, pf, beta, gen, mres), (v, p, s, big, pf, beta, gen, mres)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_model_survives_copy_and_save_after_range_guard_fallback(tmp_path):
    """After one fallback the module holds packed_fp32()'s ctypes structs (_pack32): it must still deep-copy, pickle and torch.save, the copies must compute what the
    original computes (ordinary and oversized inputs, bit for bit), and invalidate_packed() must drop the fp32 pack with the fp16 one -- the fallback after a
    weight change through .data serves the NEW weights."""
    from ab_opt_amd import hip
    m, ordinary, oversized = _guard_case()
    net = m.diffusion.eps_net
    assert net._pack32 is None
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        base = [o.clone() for o in net(*ordinary)]
    with pytest.warns(RuntimeWarning, match='fp16 range'):
        fb = [o.clone() for o in net(*oversized)]
    assert net._pack32 is not None and all(torch.isfinite(o).all() for o in fb) and not hip.nonfinite_flag()
    copies = dict(deepcopy=copy.deepcopy(m), pickle=pickle.loads(pickle.dumps(m)))
    torch.save(m, tmp_path / 'model.pt')
    copies['torch.save'] = torch.load(tmp_path / 'model.pt', weights_only=False)
    for name, c in copies.items():
        cn = c.diffusion.eps_net
        assert cn._pack is None and cn._pack32 is None, name
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            assert _same(cn(*ordinary), base), name
        with pytest.warns(RuntimeWarning, match='fp16 range'):
            assert _same(cn(*oversized), fb), name
    # a weight changed behind the version counter: invalidate_packed() is the documented call, and it must reach the fp32 pack too
    w = net.encoder.blocks[2].mlp_transition[2].weight
    w.data.mul_(1.25)
    net.eps_crd_net[2].weight.data.add_(0.01)
    net.invalidate_packed()
    assert net._pack is None and net._pack32 is None
    with pytest.warns(RuntimeWarning, match='fp16 range'):
        changed = [o.clone() for o in net(*oversized)]
    assert not torch.equal(changed[2], fb[2])
    m2 = synth.fresh_model(10, 4, device=DEV)                                  # other weights until the load
    m2.load_state_dict(m.state_dict())
    with pytest.warns(RuntimeWarning, match='fp16 range'):
        assert _same(m2.diffusion.eps_net(*oversized), changed)
    # train() / eval() round trip: packs dropped, same answers
    m.train()
    assert net._pack is None and net._pack32 is None
    m.eval()
    with pytest.warns(RuntimeWarning, match='fp16 range'):
        assert _same(net(*oversized), changed)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert _same(net(*ordinary), m2.diffusion.eps_net(*ordinary))
    assert not hip.nonfinite_flag()


def test_guarded_call_owns_the_flag():
    """The rule: EpsilonNet.forward clears the flag in stream order BEFORE its call and reads it once after, so the flag it acts on is its own.  A flag left up by an
    earlier raw hip.eps_net_forward is not inherited (no spurious fallback, no warning), and after a guarded call -- ordinary or fallback -- the flag is down."""
    from ab_opt_amd import hip
    m, ordinary, oversized = _guard_case(5150)
    d, net = m.diffusion, m.diffusion.eps_net
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        base = [o.clone() for o in net(*ordinary)]
    assert not hip.nonfinite_flag(reset=False)
    raw = hip.eps_net_forward(net.packed(), *oversized, d.abdock, d.num_bins, False)
    assert not torch.isfinite(raw['R_next']).all() and hip.nonfinite_flag(reset=False)          # up, and left up
    with warnings.catch_warnings():
        warnings.simplefilter('error')                                      # an inherited flag would warn here
        again = net(*ordinary)
    assert _same(again, base) and net._pack32 is None                        # ... and would have built the fp32 pack
    assert not hip.nonfinite_flag(reset=False)
    with pytest.warns(RuntimeWarning, match='fp16 range'):
        net(*oversized)
    assert not hip.nonfinite_flag(reset=False)
    hip.eps_net_forward(net.packed(), *oversized, d.abdock, d.num_bins, False)
    hip.nonfinite_flag_reset()                                               # the stream-ordered clear on its own
    assert not hip.nonfinite_flag(reset=False)


def test_eps_net_captured_in_a_user_graph_leaves_the_flag_to_the_caller():
    """eps_net(...) inside a caller's torch.cuda.graph: forward must not touch the flag from the host (a synchronisation during capture is an error).  The replays equal
    the eager call bit for bit and leave the flag down; a replay on the oversized res_feat returns non-finite outputs (no fallback inside a graph) and leaves the
    flag UP for the caller: hip.nonfinite_flag(reset=True) is True, then False."""
    from ab_opt_amd import hip
    m, ordinary, oversized = _guard_case(5170)
    net = m.diffusion.eps_net
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        eager = [o.clone() for o in net(*ordinary)]                           # (also packs the weights and sizes the workspace outside the capture)
    static = [a.clone() for a in ordinary]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        net(*static)                                                        # warm-up on the capturing stream: its workspace exists before the capture
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            outs = net(*static)
    torch.cuda.current_stream().wait_stream(side)
    hip.nonfinite_flag(reset=True)
    for _ in range(2):
        for o in outs:
            o.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert _same(outs, eager)
        assert not hip.nonfinite_flag(reset=False)
    static[3].copy_(oversized[3])
    g.replay()
    torch.cuda.synchronize()
    assert not torch.isfinite(outs[1]).all()
    assert hip.nonfinite_flag(reset=True) is True and hip.nonfinite_flag(reset=True) is False
    static[3].copy_(ordinary[3])
    g.replay()
    torch.cuda.synchronize()
    assert _same(outs, eager) and not hip.nonfinite_flag(reset=False)
