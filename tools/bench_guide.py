"""What guided sampling costs: the guidance kernel alone, and a replayed sampling loop with and without it.

    python tools/bench_guide.py --kernel [--shapes 32x256,1000x48,128x256]
    python tools/bench_guide.py --loop plain|guided [--batch 32 --length 256 --repeats 7]

--kernel: hip.guide_positions (the C entry behind it) on N x L positions, by events, median of 10 calls (smallest - largest).  Every call works on the same
buffers, so after the first the generated residues have been pushed out of reach and later calls see fewer close pairs; --fresh copies the inputs back before
every call and reports the copy beside it.  Inputs: positions normal(10 A), the six CDR segments of the bench layout generated, roles random in 0..3.
--loop: the bench workload (AbDesign flavour, T = 100, distinct pair features) as ONE captured loop of 100 steps, replayed; ms per step, median of the repeats.
One process measures one arm: a captured loop carries a state of its own, so an A/B alternates processes of the two arms on one box
in one session."""
import argparse
import dataclasses
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ab_opt_amd import hip  # noqa: E402
from ab_opt_amd.dpm import _LoopSpec  # noqa: E402
from ab_opt_amd.utils import synth  # noqa: E402

KNOBS = dict(guide_attract=0.5, guide_attract_radius=8.0, guide_repel=0.5, guide_repel_radius=3.0, guide_max_shift=2.0)


def events(fn, reps=10, before=None):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), min(out), max(out)


def make(N, L, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    p = torch.randn(N, L, 3, generator=g, device=dev) * 10
    gen = torch.zeros(N, L, dtype=torch.bool, device=dev)
    for a, b in (synth.LAYOUT_256 if L == 256 else synth.LAYOUT_128)['cdrs']:
        gen[:, a:min(b, L)] = True
    role = torch.randint(0, 4, (N, L), generator=g, device=dev, dtype=torch.int32)
    return p, gen, torch.ones(N, L, dtype=torch.bool, device=dev), role


def kernel(shapes, fresh):
    dev = torch.device('cuda:0')
    fmt = lambda t: f'{t[0] * 1e3:.1f} us ({t[1] * 1e3:.1f}-{t[2] * 1e3:.1f})'
    for shape in shapes.split(','):
        N, L = (int(v) for v in shape.split('x'))
        p0, gen, res, role = make(N, L, dev)
        p, pn = p0.clone(), p0 / 10.0
        pn0 = pn.clone()
        mean = (hip.C.c_float * 3)(0.0, 0.0, 0.0)
        entry = lambda: hip._check(hip.lib().abopt_guide_positions(hip.ptr(p), hip.ptr(pn), hip.ptr(gen), hip.ptr(res), hip.ptr(role), 0, N, L, KNOBS['guide_attract'],
                                                                   KNOBS['guide_attract_radius'], KNOBS['guide_repel'], KNOBS['guide_repel_radius'],
                                                                   KNOBS['guide_max_shift'], 10.0, mean, hip.stream()))
        reset = (lambda: (p.copy_(p0), pn.copy_(pn0))) if fresh else None
        t_entry = events(entry, before=reset)
        t_py = events(lambda: hip.guide_positions(p, pn, gen, res, role, *KNOBS.values(), 10.0, (0.0, 0.0, 0.0)), before=reset)
        t_copy = events(lambda: (p.copy_(p0), pn.copy_(pn0)))
        moved = int((gen & res).sum())
        print(f'{N} x {L}: C entry {fmt(t_entry)} | Python call {fmt(t_py)} | the two copies a fresh call is preceded by {fmt(t_copy)} | {moved // N} moved rows and '
              f'{int(((role & 2) != 0)[~gen].sum()) // N} repellers per sample', flush=True)


def loop(arm, N, L, repeats):
    import bench
    dev = torch.device('cuda:0')
    T = 100
    dpm, state, res_feat, pair_feat, gen, mres = bench.build_workload(dev, N, L, T, seed=2022)
    role = torch.randint(0, 4, (N, L), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(dev)
    spec = _LoopSpec(T)
    inputs = (res_feat, pair_feat, gen, mres)
    if arm == 'guided':
        spec, inputs = dataclasses.replace(spec, guided=True, **hip.check_guidance(**KNOBS)), inputs + (role,)
    run = lambda: dpm._denoise(spec, state, inputs, None, 1234, 0, False, True)
    run()                                                   # capture + first replay
    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / T * 1e3)
    assert dpm.last_run_info['graph'] is True and bool(torch.isfinite(out[1][0]).all())
    print(f'{arm} loop, N = {N}, L = {L}, T = {T}, replayed: {float(np.median(ms)):.4f} ms per step, median of {repeats} ({min(ms):.4f}-{max(ms):.4f})', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--shapes', default='32x256,1000x48,128x256')
    ap.add_argument('--fresh', action='store_true', help='copy the inputs back before every timed call')
    ap.add_argument('--loop', choices=('plain', 'guided'), default=None)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--length', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=7)
    args = ap.parse_args()
    if args.kernel:
        kernel(args.shapes, args.fresh)
    if args.loop:
        loop(args.loop, args.batch, args.length, args.repeats)


if __name__ == '__main__':
    main()
