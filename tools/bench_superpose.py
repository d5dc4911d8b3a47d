"""Device time of hip.superposed_rmsd and hip.cluster_shapes_grouped.

    python tools/bench_superpose.py [--shapes 1024x1024,4096x4096 --lengths 16,256 --cluster 4096,16384 --points 16 --reps 10]

Every measurement is a torch.cuda.graph of the call replayed --reps times between two events on the stream, reported as the median replay (smallest -
largest) and as pairs per second.  Q x R: every row n points, NULL masks (all points fitted and measured), with and without the transform outputs.
Clustering: one group of S structures of --points points, members of 32 shape families each rigidly displaced at random plus 0.1 A noise, at a cutoff of
1 A; the adjacency kernel evaluates S^2 pairs (each unordered pair twice, once per bit row), the greedy kernel follows in the same graph.  Coordinates are
random walks of 3.8 A steps."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ab_opt_amd import hip  # noqa: E402


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
    ap.add_argument('--shapes', default='1024x1024,4096x4096')
    ap.add_argument('--lengths', default='16,256')
    ap.add_argument('--cluster', default='4096,16384', help='structures per group')
    ap.add_argument('--points', type=int, default=16, help='points of a clustered structure')
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    fmt = lambda t, pairs: f'{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f}), {pairs / t[0] / 1e6:.1f} G pairs/s'
    g = torch.Generator(device=dev).manual_seed(1)
    walk = lambda k, m: (torch.nn.functional.normalize(torch.randn(k, m, 3, generator=g, device=dev), dim=2) * 3.8).cumsum(1).contiguous()
    for n in (int(v) for v in args.lengths.split(',')):
        for shape in args.shapes.split(','):
            Q, R = (int(v) for v in shape.split('x'))
            q, r = walk(Q, n), walk(R, n)
            plain = replays(lambda: hip.superposed_rmsd(q, r), args.reps)
            full = replays(lambda: hip.superposed_rmsd(q, r, want_transform=True), args.reps)
            print(f'{Q} x {R} pairs of {n} points: superposed_rmsd {fmt(plain, Q * R)} | with rot and trans {fmt(full, Q * R)}', flush=True)
    n = args.points
    for S in (int(v) for v in args.cluster.split(',')):
        fam = walk(32, n)
        which = torch.randint(0, 32, (S,), generator=g, device=dev)
        rot = hip.so3_exp(torch.randn(S, 3, generator=g, device=dev) * 1.5)
        x = (torch.einsum('sab,skb->ska', rot, fam[which]) + torch.randn(S, 1, 3, generator=g, device=dev) * 20.0 + torch.randn(S, n, 3, generator=g, device=dev) * 0.1).contiguous()
        t = replays(lambda: hip.cluster_shapes_grouped(x, S, 1.0), args.reps)
        count = int(hip.cluster_shapes_grouped(x, S, 1.0)['count'][0])
        print(f'{S} structures of {n} points: cluster_shapes_grouped {fmt(t, S * S)} (S^2 evaluations), {count} clusters', flush=True)


if __name__ == '__main__':
    main()
