"""Carried fragments (csrc/forward_plan.h: carry_next; csrc/ipa_core.hip: ipa_core32_kernel<true, *, true>): the fused kernel of block i writes
block i + 1's q / k / v fragments as its last phase, from the rows it still holds, and that block's node_frags launch disappears.  The phase runs node_frags' own
task (csrc/node_task.h) and writes the other fragment pair of the workspace, so everything here is torch.equal against the same call under ABOPT_FUSE_NODE=0 (every
block behind a node_frags launch of its own) -- on a three-block EpsilonNet with the pair-bias cache, pair terms and ABOPT_CORE32=1, so that the small shapes take
the 32-row kernels: one chain not carried / carried / carried over the fragment slots 0, 1, 0.  That these shapes do carry on a 256-CU device (and that L = 17 does
not) is pinned without a device in tests/test_forward_plan_carry.py::test_shapes_of_the_gpu_test_are_carried, with the workspace's own fit rule."""
import ctypes as C

import pytest
import torch

from ab_opt_amd import hip
from ab_opt_amd.dpm import FullDPM, _LoopSpec
from ab_opt_amd.utils import synth

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
T = 3
KEYS = ('v_next', 'R_next', 'eps_pos', 'c')


@pytest.fixture(scope='module')
def design():
    m = FullDPM(128, 64, num_steps=T, eps_net_opt=dict(num_layers=3), _abdesign=True).eval()
    return synth.fill_module_(m, seed=5).to(DEV)


@pytest.fixture(autouse=True)
def core32(monkeypatch):
    monkeypatch.setenv('ABOPT_CORE32', '1')
    monkeypatch.setenv('ABOPT_CORE_NO_SPLIT', '1')


def _inputs(N, L, lengths, gen_ranges, salt, hole=None, complexes=None):
    v, p, s, res_feat, pair_feat, beta, gen, mres = [a.to(DEV) for a in synth.eps_inputs(N, L, lengths, gen_ranges, salt=salt, num_steps=T, t=2)]
    if hole is not None:                                    # a mask that is not a prefix: residues missing inside the first sample
        mres[0, hole[0]:hole[1]] = False
        gen &= mres
        s = torch.where(mres, s, torch.full_like(s, 21))
    if complexes is not None:                               # consecutive groups of N / complexes samples share the pair features of their complex
        pair_feat = pair_feat[:complexes].contiguous()
    return v, p, s, res_feat, pair_feat, beta, gen, mres


def _forward(d, monkeypatch, fuse, inp, terms=True, shared=0, ew=None):
    v, p, s, rf, pf, beta, gen, mres = inp
    monkeypatch.setenv('ABOPT_FUSE_NODE', '1' if fuse else '0')
    pbc = hip.pair_bias_cache(d.eps_net.encoder.packed_array(), len(d.eps_net.encoder.blocks), pf)
    out = hip.eps_net_forward(ew if ew is not None else d.eps_net.packed(), v, p, s, rf, pf, beta, gen, mres, d.abdock, d.num_bins, False, pair_bias_cache=pbc,
                              pair_feat_shared=shared, pair_terms=hip.pair_terms(pf) if terms else None)
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in KEYS}


def _same(got, ref):
    for k in KEYS:
        assert torch.isfinite(got[k]).all(), k
        assert torch.equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))


CASES = {
    # N, L, lengths, hole                                                      what the shape exercises
    'three_chunks_last_block_one_row': (2, 33, [33, 33], None),              # the last 32-row block owns one row, its second row tile does not exist
    'second_row_tile_exactly_absent': (2, 48, [48, 48], None),               # three chunks: block 1 has rows 32..47 and no second tile
    'partial_second_tile_ragged': (3, 70, [70, 52, 33], None),               # five chunks, the last tile partial; ragged lengths
    'full_blocks_xcd_mapping': (8, 64, [64] * 8, None),                      # N % 8 == 0: the XCD-aware block mapping
    'mask_not_a_prefix': (3, 70, [70, 64, 41], (9, 21)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_carried_fragments_are_bit_identical(design, monkeypatch, name):
    N, L, lengths, hole = CASES[name]
    inp = _inputs(N, L, lengths, [(3, 11), (20, 29)], salt=900 + N, hole=hole)
    ref = _forward(design, monkeypatch, False, inp)
    got = _forward(design, monkeypatch, True, inp)
    _same(got, ref)


def test_fp32_qk_slots(design, monkeypatch):
    """without pair terms the 32-row kernels read q / k as fp32 slots: the carried projections write that form (the next block's plan says which)"""
    inp = _inputs(3, 70, [70, 52, 33], [(3, 11), (20, 29)], salt=910)
    _same(_forward(design, monkeypatch, True, inp, terms=False), _forward(design, monkeypatch, False, inp, terms=False))


def test_grouped_launch_with_shared_pair_features(design, monkeypatch):
    """N = 4 samples of two complexes in one launch (pair_feat_shared = 2): the block index -> (sample, row block) map of the grouped form"""
    inp = _inputs(4, 48, [48, 40, 48, 37], [(3, 11), (20, 29)], salt=920, complexes=2)
    _same(_forward(design, monkeypatch, True, inp, shared=2), _forward(design, monkeypatch, False, inp, shared=2))


def test_plain_block_in_the_middle(design, monkeypatch):
    """block 1 without packed operands (GEMM projections, GEMM tail): nothing is carried into it or out of it, block 2 runs its own node_frags"""
    ew = design.eps_net.packed()
    arr = (hip.GaWeights * 3)()
    for i, b in enumerate(design.eps_net.encoder.blocks):
        src = b.packed()[1]
        for name, _ in hip.GaWeights._fields_:
            setattr(arr[i], name, None if i == 1 and name in ('w_node_frag', 'w_out_frag', 'w_out_terms', 'w_mlp_frag') else getattr(src, name))
    mixed = hip.EpsWeights()
    for name, _ in hip.EpsWeights._fields_:
        setattr(mixed, name, getattr(ew, name))
    mixed.blocks = C.cast(arr, C.POINTER(hip.GaWeights))
    inp = _inputs(3, 70, [70, 52, 33], [(3, 11), (20, 29)], salt=930)
    _same(_forward(design, monkeypatch, True, inp, ew=mixed), _forward(design, monkeypatch, False, inp, ew=mixed))


def test_below_the_alias_limit(design, monkeypatch):
    """L = 17: two padded row tiles per sample are more than proj | feat of 17 rows hold, the workspace has no second fragment pair and the plan carries nothing"""
    inp = _inputs(2, 17, [17, 12], [(3, 11)], salt=940)
    _same(_forward(design, monkeypatch, True, inp), _forward(design, monkeypatch, False, inp))


def _loop(dpm, monkeypatch, fuse, state, inputs, graph):
    monkeypatch.setenv('ABOPT_FUSE_NODE', '1' if fuse else '0')
    out = dpm._denoise(_LoopSpec(T), state, inputs, None, 11, 4096, False, graph)
    torch.cuda.synchronize()
    assert dpm.last_run_info['steps'] == T and dpm.last_run_info['pair_terms'] and bool(dpm.last_run_info['graph']) == graph
    return [a.clone() for a in out if a is not None]


def test_step_loop_eager_and_replayed(design, monkeypatch):
    """three steps of abopt_eps_net_step with the mixer carried from step to step: eager, captured and replayed, and replayed again"""
    v, p, s, rf, pf, _, gen, mres = _inputs(3, 70, [70, 52, 33], [(3, 11), (20, 29)], salt=950)
    state, inputs = (v, p * 10.0, s), design._inputs(rf, pf, gen, mres, None)
    design.clear_graphs()
    ref = _loop(design, monkeypatch, False, state, inputs, False)
    eager = _loop(design, monkeypatch, True, state, inputs, False)
    first = _loop(design, monkeypatch, True, state, inputs, True)
    second = _loop(design, monkeypatch, True, state, inputs, True)
    design.clear_graphs()
    for got in (eager, first, second):
        assert len(got) == len(ref) == 3 and all(torch.equal(a, b) for a, b in zip(got, ref)), [int((a != b).sum()) for a, b in zip(got, ref)]
    assert not torch.equal(ref[0][0], ref[0][-1])           # the loop moved the state
