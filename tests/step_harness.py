"""What the tests of the step entry's optional facts share (tests/test_step_rows.py: context_outputs_unused; tests/test_step_compact.py: the row list): a three-block
AbDesign model, the environment under which their small shapes take the 32-row kernels, a chain of calls of hip.eps_net_step run eagerly or from a replayed graph, the
comparison of two such chains and a keyed cache of the chain they compare against.  A test module keeps its shapes, masks, inputs and the assertions of its own."""
import torch

from ab_opt_amd import hip
from ab_opt_amd.dpm import FullDPM, _LoopSpec
from ab_opt_amd.utils import synth

DEV = torch.device('cuda:0')
T = 3
NET = ('v_next', 'R_next', 'eps_pos', 'c')
OUT = ('v', 'p', 's', 'p_norm')


def model():
    m = FullDPM(128, 64, num_steps=T, eps_net_opt=dict(num_layers=3), _abdesign=True).eval()
    return synth.fill_module_(m, seed=5).to(DEV)


def core32_env(monkeypatch):
    """the 32-row kernels at small shapes, and every switch of the row forms as the library defaults it"""
    monkeypatch.setenv('ABOPT_CORE32', '1')
    monkeypatch.setenv('ABOPT_CORE_NO_SPLIT', '1')
    for name in ('ABOPT_STEP_ROWS', 'ABOPT_STEP_COMPACT', 'ABOPT_PAIR_TERMS'):
        monkeypatch.delenv(name, raising=False)


def steps(d, inp, nsteps, terms, pbc, pterms, **step_kwargs):
    """nsteps calls of the step entry from t = T down, the mixer carried from call to call; every call has network and output buffers of its own.  step_kwargs go to
    hip.eps_net_step; query_rows=True stands for the row list of inp['gen'] with inp['tiles'] tiles, built here, once"""
    N, L = inp['N'], inp['L']
    f32 = dict(dtype=torch.float32, device=DEV)
    ew = d.eps_net.packed()
    X, cdf = d._loop_tables(d._loop_steps(_LoopSpec(T)))
    v, p, s = inp['v'], inp['p'], inp['s']
    p_norm = ((p - d.position_mean) / d.position_scale).contiguous()
    if step_kwargs.get('query_rows') is True:
        step_kwargs['query_rows'] = (*hip.query_row_list(inp['gen']), inp['tiles'])
    res = []
    for j in range(nsteps):
        t = T - j
        net = dict(v_next=torch.empty(N, L, 3, **f32), R_next=torch.empty(N, L, 3, 3, **f32), eps_pos=torch.empty(N, L, 3, **f32), c=torch.empty(N, L, 20, **f32),
                   prmsd_logits=None)
        out = dict(v=torch.empty(N, L, 3, **f32), p=torch.empty(N, L, 3, **f32), s=torch.empty(N, L, dtype=torch.int64, device=DEV), p_norm=torch.empty(N, L, 3, **f32))
        beta = d.trans_pos.var_sched.betas[t].expand(N).contiguous()
        post = hip.eps_net_step(ew, v, p_norm, s, inp['res_feat'], inp['pair_feat'], beta, inp['gen'], inp['mres'], d.num_bins, net,
                                d._step_params(t, True, True, True, False, t - 1), None, 11, 4096, p, X[j], cdf[j], out, pair_bias_cache=pbc,
                                pair_feat_shared=inp['group'], pair_terms=pterms if terms else None, want_post=True, carry_in=j > 0, carry_out=j + 1 < nsteps,
                                **step_kwargs)
        res.append(dict(net=net, out=out, post=post))
        v, p, s, p_norm = out['v'], out['p'], out['s'], out['p_norm']
    return res


def run(d, inp, nsteps, terms, replays=0, **step_kwargs):
    """steps(...) eagerly (replays = 0), or captured once and replayed `replays` times: (the results of the last replay, abopt_nonfinite_flag)"""
    pf = inp['pair_feat']
    pbc = hip.pair_bias_cache(d.eps_net.encoder.packed_array(), len(d.eps_net.encoder.blocks), pf)
    pterms = hip.pair_terms(pf)
    hip.nonfinite_flag(reset=True)
    if not replays:
        res = steps(d, inp, nsteps, terms, pbc, pterms, **step_kwargs)
    else:
        hip.prof_enable(False)
        steps(d, inp, 1, terms, pbc, pterms, **step_kwargs)                 # warm: kernel attributes, host-side caches
        torch.cuda.synchronize()
        before = set(hip.Workspace._bufs)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            res = steps(d, inp, nsteps, terms, pbc, pterms, **step_kwargs)
        keep = [hip.Workspace._bufs.pop(k) for k in set(hip.Workspace._bufs) - before]       # the slab the capture allocated lives in the graph's pool
        for _ in range(replays):
            for r in res:
                for a in list(r['net'].values()) + list(r['out'].values()) + [r['post']]:
                    if a is not None:
                        a.fill_(7)                                            # a replay that wrote nothing would be seen
            g.replay()
        torch.cuda.synchronize()
        clone = lambda d_: {k: (a.clone() if a is not None else None) for k, a in d_.items()}
        res = [dict(net=clone(r['net']), out=clone(r['out']), post=r['post'].clone()) for r in res]      # own storage: the buffers are the graph's static ones
        del keep, g
    torch.cuda.synchronize()
    flag = hip.nonfinite_flag(reset=True)
    return res, flag


def check(got, flag_got, ref, flag_ref, gen, everything):
    """what the step hands on and the posterior equal on every row; the network's outputs finite, equal on generated rows and -- everything -- on every row"""
    assert not flag_ref and not flag_got                                    # abopt_nonfinite_flag reads 0
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        for k in OUT:
            assert torch.equal(a['out'][k], b['out'][k]), (k, int((a['out'][k] != b['out'][k]).sum()))
        assert torch.equal(a['post'], b['post'])
        for k in NET:
            assert torch.isfinite(a['net'][k]).all() and torch.isfinite(b['net'][k]).all(), k
            assert torch.equal(a['net'][k][gen], b['net'][k][gen]), (k, int((a['net'][k][gen] != b['net'][k][gen]).sum()))
            if everything:
                assert torch.equal(a['net'][k], b['net'][k]), k


def cached_reference(cache, inputs, d, shape, mask, terms, nsteps, **step_kwargs):
    """(inputs(shape, mask), *run(...)) of the form a module compares against, computed once per (shape, mask, terms, steps) of its cache and shared"""
    key = (shape, mask, terms, nsteps)
    if key not in cache:
        inp = inputs(shape, mask)
        cache[key] = (inp,) + run(d, inp, nsteps, terms, **step_kwargs)
    return cache[key]
