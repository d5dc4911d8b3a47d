"""Device time of hip.align_traceback and hip.superposed_rmsd_mapped beside hip.align_sequences on the same rows.

    python tools/bench_alignment.py [--shapes 128x1,128x1024,1000x1000 --lengths 16,256 --reps 10]

Per shape Q x R and length n (every row n residues, NULL masks, all Q R pairs): each call captured once and replayed, by events, median of --reps replays
(smallest - largest), ms.  Sequences are uniform over the twenty types, the table is model.identity_table(), gaps -20 / -1, as in tools/bench_similarity.py;
coordinates are random walks of 3.8 A steps; the mapped RMSD runs on the maps the traceback wrote.  `traceback / align` is what the bits in LDS and the walk
cost over the three integers alone.  Every pair runs the whole n x n table: there is no band and no early exit to favour an input."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ab_opt_amd import hip, model  # noqa: E402


def replays(fn, reps):
    """fn() captured once and replayed: (median, min, max) ms of a replay, by events"""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = fn()                                                  # noqa: F841 (the outputs live as long as the graph)
    graph.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='128x1,128x1024,1000x1000')
    ap.add_argument('--lengths', default='16,256')
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    tdev = model.identity_table().to(dev)
    fmt = lambda t: f'{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})'
    for n in (int(v) for v in args.lengths.split(',')):
        for shape in args.shapes.split(','):
            Q, R = (int(v) for v in shape.split('x'))
            g = torch.Generator(device=dev).manual_seed(Q * R + n)
            q, r = (torch.randint(0, 20, (k, n), generator=g, device=dev).to(torch.uint8) for k in (Q, R))
            walk = lambda k, m: (torch.nn.functional.normalize(torch.randn(k, m, 3, generator=g, device=dev), dim=2) * 3.8).cumsum(1).contiguous()
            qca, rca = walk(Q, n), walk(R, n)
            al = replays(lambda: hip.align_sequences(q, r, tdev, -20, -1), args.reps)
            tb = replays(lambda: hip.align_traceback(q, r, tdev, -20, -1), args.reps)
            lean = replays(lambda: hip.align_traceback(q, r, tdev, -20, -1, want_ops=False), args.reps)
            qmap = hip.align_traceback(q, r, tdev, -20, -1, want_ops=False)['qmap']
            mapped = replays(lambda: hip.superposed_rmsd_mapped(qca, rca, qmap), args.reps)
            pairs = float((qmap >= 0).sum(1).float().mean())
            qmap = torch.arange(n, device=dev, dtype=torch.int16).expand(Q * R, n).contiguous()      # every element paired: the most a map can ask for
            full = replays(lambda: hip.superposed_rmsd_mapped(qca, rca, qmap), args.reps)
            print(f'{Q} x {R} pairs of length {n}: align_sequences {fmt(al)} | align_traceback {fmt(tb)}, without ops {fmt(lean)}, traceback / align '
                  f'{tb[0] / al[0]:.2f} | superposed_rmsd_mapped {fmt(mapped)} on the traced maps ({pairs:.1f} aligned pairs a map), {fmt(full)} on identity '
                  f'maps ({n} pairs)', flush=True)
            del qmap


if __name__ == '__main__':
    main()
