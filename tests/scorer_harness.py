"""What the tests of the candidate scorers share (tests/test_interface_geometry.py, test_sasa.py, test_pose_clusters.py, test_sequence_clusters.py; test_lddt.py
takes `stages` and `spawn2` only): test inputs on the device, the screen's models without a captured loop, the screen's three stages written out with the public calls, two
spawned gloo ranks and what each of them runs, and the bodies of the properties every scorer has -- a grouped call equals the per-group calls, a call is
capturable, the screen does not depend on the launch size or the number of ranks.  A test module keeps its definition (the float64 / fp32 statement), its
inputs, its shapes and the assertions of its own."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import screen_workers                                               # noqa: E402

DEV = torch.device('cuda:0')


def dev(case, *names):
    """the named numpy arrays of a test case as device tensors"""
    return [torch.from_numpy(np.array(case[n])).to(DEV) for n in names]


@pytest.fixture
def screen_models():
    """(dock, design) of screen_workers with no captured denoising loop before or after the test.  The models are the session's cached ones and a loop is captured
    into a hipGraph from its second call with the same shapes, with the kernel forms of the environment at that moment (the graph key does not hold
    ABOPT_PAIR_TERMS / ABOPT_CORE_NO_SPLIT): a graph captured by one test must not be replayed under another test's switches.  A test module imports this name to
    use the fixture."""
    pair = screen_workers.models(DEV)
    for m in pair:
        m.diffusion.clear_graphs()
    yield pair
    for m in pair:
        m.diffusion.clear_graphs()


def pin_denoiser_form(monkeypatch):
    """ABOPT_PAIR_TERMS=0 / ABOPT_CORE_NO_SPLIT=1 pin one arithmetic form of the denoiser, whatever the batch of a launch: what DESIGN.md section 6.1 prescribes for
    a bit-for-bit comparison of runs with different launch sizes, and tests/test_screen.py does."""
    monkeypatch.setenv('ABOPT_PAIR_TERMS', '0')
    monkeypatch.setenv('ABOPT_CORE_NO_SPLIT', '1')


def assert_same_results(got, want, tag):
    """two result dicts hold the same fields, torch.equal one by one (a result loaded from a rank's file lives on the CPU)"""
    assert set(got) == set(want), (tag, sorted(set(got) ^ set(want)))
    for name, v in want.items():
        assert torch.equal(got[name], v.to(got[name].device)), (tag, name)


# ------------------------------------------------------------------------------------------ the properties of a call
def group_slice(tensors, g, S, per_group):
    """group g of a dict of tensors: the rows g S .. (g + 1) S of every entry, the one row g of those named in per_group"""
    return {k: None if v is None else v[g:g + 1] if k in per_group else v[g * S:(g + 1) * S] for k, v in tensors.items()}


def grouped_equals_per_group(call, cases, per_group):
    """cases: (tag, G, S, inputs) with inputs a dict of tensors; call(**inputs) -> a dict of tensors.  G groups in one call against G single-group calls:
    torch.equal on every field.  per_group names the inputs and results that have one row per group; every other one has one per candidate."""
    for tag, G, S, inputs in cases:
        whole = call(**inputs)
        for g in range(G):
            assert_same_results(call(**group_slice(inputs, g, S, per_group)), group_slice(whole, g, S, per_group), (tag, g))


def capture_replays_on_other_inputs(call, inputs, other):
    """call(**inputs) recorded with torch.cuda.graph and replayed, then replayed on `other` (name -> tensor) copied into the static inputs, without a
    synchronisation between the copy and the replay: the second replay leaves what the eager call gives on those inputs, field by field.
    -> (a copy of what the first replay left, what the second left) for the caller's own assertions."""
    call(**inputs)                                                                  # library load, device queries, workspace
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = call(**inputs)
    graph.replay()
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in held.items()}
    for name, src in other.items():
        inputs[name].copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    assert_same_results(held, call(**inputs), 'replayed on other inputs against the eager call')
    return first, held


# ------------------------------------------------------------------------------------------ the screen
def stages(dock, design, one, P, S, k, D, contig, seed):
    """The three stages written out with the public calls (tests/test_screen.py: _composition) -> the poses and the re-docks as (pos, mask)."""
    from ab_opt_amd import geometry, hip, sampler, screen
    from ab_opt_amd.model import generate_mask_from_str
    rep = lambda t, n: t.expand(n, *t.shape[1:]).contiguous()
    aa, cn, rn = one['aa'], one['chain_nb'], one['res_nb']
    gen = one['generate_flag'][0]
    t1 = sampler.sample_replicated(dock, one, P, dict(sample_structure=True, sample_sequence=False, seed=screen.stage_seed(seed, 'dock'), rng_offset=0))[0]
    g1 = rep(gen[None], P)
    pose_pos, pose_mask = geometry.reconstruct_backbone_partially(rep(one['pos_heavyatom'], P), hip.so3_exp(t1[0]), t1[1], torch.where(g1, t1[2], rep(aa, P)),
                                                                  rep(cn, P), rep(rn, P), rep(one['mask_heavyatom'], P), g1)
    dflag = gen & generate_mask_from_str(contig, gen)
    cx = [dict(one, pos_heavyatom=pose_pos[i:i + 1], mask_heavyatom=pose_mask[i:i + 1], generate_flag=dflag[None]) for i in range(P)]
    t2 = sampler.sample_grouped(design, cx, S, dict(sample_structure=False, sample_sequence=True, seed=screen.stage_seed(seed, 'design'), rng_offset=0))[0]
    g2 = rep(dflag[None], P * S)
    aa2 = torch.where(g2, t2[2], rep(aa, P * S))
    des_pos, des_mask = geometry.reconstruct_backbone_partially(pose_pos.repeat_interleave(S, 0), hip.so3_exp(t2[0]), t2[1], aa2, rep(cn, P * S), rep(rn, P * S),
                                                                pose_mask.repeat_interleave(S, 0), g2)
    chosen = torch.sort(t2[4].to(DEV).view(P, S), dim=1, stable=True)[1][:, :k]
    rows = (torch.arange(P, device=DEV)[:, None] * S + chosen).reshape(-1)
    npos, nmask, naa = des_pos[rows], des_mask[rows], aa2[rows]
    cx = [dict(one, pos_heavyatom=npos[i:i + 1], mask_heavyatom=nmask[i:i + 1], aa=naa[i:i + 1], generate_flag=gen[None]) for i in range(P * k)]
    t3 = sampler.sample_grouped(dock, cx, D, dict(sample_structure=True, sample_sequence=False, seed=screen.stage_seed(seed, 'redock'), rng_offset=0))[0]
    g3 = rep(gen[None], P * k * D)
    rpos, rmask = geometry.reconstruct_backbone_partially(npos.repeat_interleave(D, 0), hip.so3_exp(t3[0]), t3[1], torch.where(g3, t3[2], naa.repeat_interleave(D, 0)),
                                                          rep(cn, P * k * D), rep(rn, P * k * D), nmask.repeat_interleave(D, 0), g3)
    return pose_pos, pose_mask, rpos, rmask


def screen_is_launch_size_invariant(models, extra, new_fields=()):
    """screen_workers.SCREEN with the options `extra`, with all, 1 and 2 poses per launch: every field bit for bit, those of new_fields among them.  Call
    pin_denoiser_form first.  -> the result with all poses in one launch"""
    from ab_opt_amd import screen
    dock, design = models
    one = screen_workers.complex_(DEV)
    kw = dict(screen_workers.SCREEN, **extra)
    runs = [screen.optimize_antibody(dock, design, one, poses_per_launch=n, **kw) for n in (kw['num_poses'], 1, 2)]
    assert set(new_fields) <= set(runs[0])
    for n, r in zip((1, 2), runs[1:]):
        assert_same_results(r, runs[0], ('poses_per_launch', n))
    return runs[0]


def spawn2(fn, tmp_path):
    """fn(rank, 2, port, str(tmp_path)) in two spawned processes"""
    import socket
    import torch.multiprocessing as mp
    for attempt in range(2):
        sk = socket.socket(); sk.bind(('127.0.0.1', 0)); port = sk.getsockname()[1]; sk.close()
        try:
            mp.spawn(fn, args=(2, port, str(tmp_path)), nprocs=2, join=True)
            return
        except Exception as e:             # a rendezvous that failed (the free port was taken between close() and the workers' bind, a slow first import
            msg = str(e)                   # on a fresh box) is retried once on a new port; anything the workers compute is not
            if attempt == 1 or not any(w in msg for w in ('init_process_group', 'ddress already in use', 'onnection', 'timed out', 'Timeout')):
                raise


def rank_worker(rank, world, port, outdir, runs):
    """One spawned rank of a two-rank screen: both ranks share cuda:0 and the process group is gloo, so the gather goes through host memory.  runs(device, outdir)
    -> {file stem: keyword arguments on top of screen_workers.SCREEN}; every run takes two poses (units) per launch and is saved, on the CPU, as
    <outdir>/<stem>_<rank>.pt.  The *_workers modules wrap this in module-level functions, which mp.spawn can pickle."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from ab_opt_amd import screen
        dock, design = screen_workers.models(DEV)
        for stem, extra in runs(DEV, outdir).items():
            res = screen.optimize_antibody(dock, design, screen_workers.complex_(DEV), poses_per_launch=2, **dict(screen_workers.SCREEN, **extra))
            torch.save({k: v.cpu() for k, v in res.items()}, os.path.join(outdir, f'{stem}_{rank}.pt'))
    finally:
        dist.destroy_process_group()


def two_ranks_return(worker, tmp_path, refs):
    """refs: {file stem: the result of one process}.  Two gloo ranks sharing cuda:0 (5 poses split 3 + 2, two per launch) each return every one of them, bit for bit."""
    spawn2(worker, tmp_path)
    for stem, want in refs.items():
        for r in range(2):
            assert_same_results(torch.load(tmp_path / f'{stem}_{r}.pt'), want, (stem, r))
