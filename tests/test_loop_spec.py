"""The sampling driver's host logic: one description of a denoising loop (dpm._LoopSpec) from sample() / optimize() to the captured graph's cache key, one range-guard
protocol, one input normaliser, one list of derived fields per class.  Everything but the last test runs without a GPU (the device calls are recording fakes)."""
import copy
import dataclasses
import pickle
import warnings

import pytest
import torch

from conftest import build_model
from ab_opt_amd import hip, modules
from ab_opt_amd.dpm import FullDPM, _LoopSpec, _graph_key, _loop_inputs
from ab_opt_amd.utils import synth


def _inputs(N=2, L=8, Nc=None, Nr=None):
    Nc, Nr = N if Nc is None else Nc, N if Nr is None else Nr
    return torch.zeros(Nr, L, 128), torch.zeros(Nc, L, L, 64), torch.zeros(N, L, dtype=torch.bool), torch.ones(N, L, dtype=torch.bool)


# ------------------------------------------------------------------------------------------ the spec and the graph key
class _Stop(Exception):
    pass


@pytest.fixture
def spec_of(monkeypatch):
    """spec_of(lambda d: d.sample(...)) -> the _LoopSpec that call hands to FullDPM._denoise (the device work before it is faked, the loop itself never starts)."""
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


def test_sample_and_optimize_each_describe_their_loop_once(spec_of):
    rf, pf, gen, mres = _inputs()
    v = p = torch.zeros(2, 8, 3)
    s = torch.zeros(2, 8, dtype=torch.long)
    a = spec_of(lambda d: d.sample(v, p, s, rf, pf, gen, mres, seed=1))
    assert a == _LoopSpec(t_start=10, stop_after=None, sample_structure=True, sample_sequence=True, ppl_masked=True, optimize_mode=False, use_bias_cache=None)
    b = spec_of(lambda d: d.optimize(v, p, s, 4, rf, pf, gen, mres, sample_sequence=0, seed=1, use_bias_cache=True))
    assert b == _LoopSpec(t_start=4, stop_after=None, sample_structure=True, sample_sequence=False, ppl_masked=False, optimize_mode=True, use_bias_cache=True)


def test_run_turns_its_positional_arguments_into_the_same_spec(spec_of):
    rf, pf, gen, mres = _inputs()
    got = spec_of(lambda d: d._run(None, 7, rf, pf, gen, mres, 1, 0, True, None, 5, 0, False, stop_after=3, optimize_mode=True, use_bias_cache=False))
    assert got == _LoopSpec(7, 3, True, False, True, True, False)


def test_every_field_of_the_spec_tells_graph_keys_apart():
    """Iterates over dataclasses.fields: a field added to _LoopSpec later is covered (and must be hashable) without an edit here."""
    inputs, token = _inputs(), object()
    base = _LoopSpec(10, 5, True, True, True, False, True)
    hash(base)
    assert _graph_key(base, inputs, token) == _graph_key(dataclasses.replace(base), inputs, token)
    for f in dataclasses.fields(_LoopSpec):
        old = getattr(base, f.name)
        other = dataclasses.replace(base, **{f.name: (not old) if isinstance(old, bool) else old + 1})
        assert other != base and _graph_key(other, inputs, token) != _graph_key(base, inputs, token), f.name
    assert _graph_key(dataclasses.replace(base, stop_after=None), inputs, token) != _graph_key(base, inputs, token)
    assert _graph_key(dataclasses.replace(base, use_bias_cache=None), inputs, token) != _graph_key(base, inputs, token)
    # ... and so do the shapes and the pack token
    assert _graph_key(base, _inputs(Nc=1), token) != _graph_key(base, inputs, token) != _graph_key(base, _inputs(L=9), token)
    assert _graph_key(base, inputs, object()) != _graph_key(base, inputs, token)


# ------------------------------------------------------------------------------------------ the range guard
@pytest.fixture
def guard_log(monkeypatch):
    log, flag = [], [False]
    monkeypatch.setattr(hip, 'nonfinite_flag_reset', lambda: log.append('reset'))

    def read(reset=True):
        log.append(('read', reset))
        return flag[0]
    monkeypatch.setattr(hip, 'nonfinite_flag', read)

    def run(range_safe):
        log.append('rerun' if range_safe else 'run')
        return 'fp32' if range_safe else 'fp16'
    return log, flag, run


def test_range_guard_with_the_flag_down_is_reset_run_read(guard_log):
    log, flag, run = guard_log
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert modules._range_guarded(run) == 'fp16'
    assert log == ['reset', 'run', ('read', False)]


def test_range_guard_with_the_flag_up_warns_reruns_and_resets(guard_log):
    log, flag, run = guard_log
    flag[0] = True

    def api(*tail):                 # stands for sample() / EpsilonNet.forward
        return modules._range_guarded(run, *tail)

    def user(*tail):
        return api(*tail)           # <- the line the warning must name
    with pytest.warns(RuntimeWarning, match='fp16 range') as rec:
        assert user() == 'fp32'
    assert log == ['reset', 'run', ('read', False), 'rerun', 'reset']
    assert len(rec) == 1 and rec[0].filename == __file__ and rec[0].lineno == user.__code__.co_firstlineno + 1
    head = 'ab_opt_amd: a denoiser activation left the fp16 range (|x| >= 65504) or an input was not finite; '
    assert str(rec[0].message) == head + 'this call is repeated with the dense layers as fp32 GEMMs (slower, fp32 range)'
    with pytest.warns(RuntimeWarning, match='fp16 range') as rec:
        user('EpsilonNet.forward is repeated with the dense layers as fp32 GEMMs')
    assert str(rec[0].message) == head + 'EpsilonNet.forward is repeated with the dense layers as fp32 GEMMs'


def test_sample_reruns_the_same_spec_eagerly_on_fp32_packs(guard_log, monkeypatch):
    """The answer to a raised flag is the first call again -- same spec, same state, inputs, seed and offset -- with range_safe=True (which _denoise runs eagerly)."""
    log, flag, _ = guard_log
    flag[0] = True
    d = build_model(10, 3).diffusion
    rf, pf, gen, mres = _inputs()
    calls = []

    def denoise(self, spec, state, inputs, noise, seed, rng_offset, pbar, graph=None, range_safe=False):
        calls.append((spec, state, inputs, noise, seed, rng_offset, pbar, graph, range_safe))
        z = torch.zeros(5, 2, 8, 3)
        return z, z, torch.zeros(5, 2, 8, dtype=torch.long), torch.zeros(5, 2), torch.zeros(5, 2)
    monkeypatch.setattr(FullDPM, '_denoise', denoise)
    monkeypatch.setattr(hip, 'lib', lambda: None)
    monkeypatch.setattr(hip, 'add_noise', lambda *a, **kw: (rf[..., :3], rf[..., :3], torch.zeros(2, 8, dtype=torch.long)))
    with pytest.warns(RuntimeWarning, match='fp16 range'):
        traj = d.optimize(rf[..., :3], rf[..., :3], torch.zeros(2, 8, dtype=torch.long), 4, rf, pf, gen, mres, seed=9, rng_offset=64, graph=True)
    assert sorted(traj) == [0, 1, 2, 3, 4]
    first, second = calls
    assert first[0] == second[0] == _LoopSpec(4, None, True, True, ppl_masked=False, optimize_mode=True)
    assert all(a is b for a, b in zip(first[1:8], second[1:8])) and (first[8], second[8]) == (False, True)


# ------------------------------------------------------------------------------------------ the input normaliser
def test_loop_inputs_rejects_a_ragged_batch_and_passes_ready_tensors_through():
    with pytest.raises(ValueError, match='pair_feat holds 2 complexes for a batch of 3 samples: the batch must be a whole number of samples per complex'):
        _loop_inputs(_inputs(N=3, Nc=2))
    with pytest.raises(ValueError, match='pair_feat holds 0 complexes'):
        _loop_inputs(_inputs(N=2, Nc=0))
    with pytest.raises(ValueError, match='res_feat must hold one entry per sample or one per complex'):
        _loop_inputs(_inputs(N=6, Nc=2, Nr=3))
    for kw in (dict(), dict(N=6, Nc=2, Nr=2), dict(N=6, Nc=2, Nr=6), dict(N=4, Nc=1, Nr=1)):
        ready = _inputs(**kw)
        assert all(a is b for a, b in zip(_loop_inputs(ready), ready)), kw
    rf, pf, gen, mres = _inputs()
    got = _loop_inputs((rf.half(), pf.double().transpose(1, 2), gen.t().contiguous().t(), mres))
    assert [a.dtype for a in got] == [torch.float32, torch.float32, torch.bool, torch.bool] and all(a.is_contiguous() for a in got) and got[3] is mres


# ------------------------------------------------------------------------------------------ derived fields
def test_copies_and_pickles_start_without_any_derived_field():
    """Every field a class lists in _DERIVED, populated by hand with something that cannot be pickled (a ctypes struct with pointers, as the packs hold): the deep copy and
    the pickle must carry the field's empty value instead, and invalidate_packed() must reach the packs."""
    d = synth.fresh_model(10, 3).diffusion
    owners = [m for m in d.modules() if getattr(m, '_DERIVED', None)]
    assert {type(m).__name__ for m in owners} == {'FullDPM', 'EpsilonNet', 'GABlock'} and len(owners) == 2 + len(d.eps_net.encoder.blocks)
    assert set(FullDPM._DERIVED) == {'_graphs', '_graph_seen', '_host_sched'} and set(modules.EpsilonNet._DERIVED) == {'_pack', '_pack32'}

    def populate():
        for m in owners:
            for name in m._DERIVED:
                setattr(m, name, hip.EpsWeights())
    with pytest.raises(ValueError, match='pointers cannot be pickled'):
        pickle.dumps(hip.EpsWeights())
    populate()
    for name, c in (('deepcopy', copy.deepcopy(d)), ('pickle', pickle.loads(pickle.dumps(d)))):
        for m in c.modules():
            for field, empty in getattr(m, '_DERIVED', {}).items():
                got = getattr(m, field)
                assert type(got) is type(empty()) and not got, (name, type(m).__name__, field)
    d.eps_net.invalidate_packed()
    assert all(getattr(m, f) is None for m in owners[1:] for f in m._DERIVED)
    assert isinstance(d._graphs, hip.EpsWeights)                              # the packs' owner does not reach into the driver's caches


# ------------------------------------------------------------------------------------------ on the device
def _same_traj(a, b):
    return sorted(a) == sorted(b) and all(len(a[t]) == len(b[t]) and all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a[t], b[t])) for t in a)


@pytest.mark.gpu
@pytest.mark.parametrize('call', ['sample', 'optimize'])
@pytest.mark.parametrize('flavour', ['abdock', 'abdesign'])
def test_eager_captured_and_automatic_loops_agree_and_a_repack_evicts(flavour, call):
    """sample() and optimize(opt_step=4) of both model flavours (N = 2, L = 32, T = 10): graph=False, graph=True and the second 'auto' call return the same trajectory
    bit for bit in every slot, with last_run_info['graph'] False / True / True; after invalidate_packed() a further captured call builds on the new pack, evicts the graph of
    the old one (exactly one stays, and it holds the new token) and still returns the same trajectory."""
    dev = torch.device('cuda:0')
    d = build_model(10, 3, flavour, device=dev).diffusion
    d.clear_graphs()
    v, p, s, rf, pf, _, gen, mres = [a.to(dev) for a in synth.eps_inputs(2, 32, [32, 27], [(4, 12)], num_steps=10, t=7)]
    if call == 'sample':
        run = lambda graph: d.sample(v, p * 10, s, rf, pf, gen, mres, seed=5, graph=graph)
    else:
        run = lambda graph: d.optimize(v, p * 10, s, 4, rf, pf, gen, mres, seed=5, graph=graph)
    try:
        eager = run(False)
        assert d.last_run_info['graph'] is False and len(d._graphs) == 0 and sorted(eager) == list(range(5 if call == 'optimize' else 11))
        captured = run(True)
        assert d.last_run_info['graph'] is True and len(d._graphs) == 1
        d.clear_graphs()
        first = run('auto')                                                     # still eager
        assert d.last_run_info['graph'] is False and len(d._graphs) == 0
        second = run('auto')
        assert d.last_run_info['graph'] is True and len(d._graphs) == 1
        assert _same_traj(captured, eager) and _same_traj(first, eager) and _same_traj(second, eager)
        old = next(iter(d._graphs.values())).token
        assert old is d.eps_net.packed()
        d.eps_net.invalidate_packed()
        third = run(True)
        assert d.last_run_info['graph'] is True and len(d._graphs) == 1
        new = next(iter(d._graphs.values())).token
        assert new is d.eps_net.packed() and new is not old
        assert _same_traj(third, eager)
    finally:
        d.clear_graphs()
