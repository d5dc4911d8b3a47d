"""Device time of hip.relax_grouped beside the two hip.interface_geometry_grouped calls that sampler.relax_candidates adds to it.

    python tools/bench_relax.py [--shapes 16x8x256x5,100x100x256x5,1000x1x48x5,16x8x256x15 --iters 50 --moved 24]

Per shape G x S x L x A: the Python call on a preallocated output, by events, median of 10 calls (smallest - largest), with the caller's bound max_moved given
and with the default min(L, 256), which sizes the workgroup's LDS for the worst case; the two geometry calls; what the relax did to the summed energy terms.
Structures are the scorer benchmarks' generator made on the device (tools/bench_sasa.py): two CA random walks of 3.8 A steps 6 A apart, atoms normal(0.9 A)
around their CA; the moved residues are a run of --moved at the end of the first walk, and the links follow the walks.  Knobs: the defaults of hip.relax_grouped."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ab_opt_amd import hip  # noqa: E402


def make(G, S, L, A, moved, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    N, n1 = G * S, max(1, L // 3)
    step = torch.randn(N, L, 3, generator=g, device=dev)
    step = step * (3.8 / step.norm(dim=-1, keepdim=True))
    ca = torch.cat([step[:, :n1].cumsum(1), step[:, n1:].cumsum(1) + torch.tensor([6.0, 0.0, 0.0], device=dev)], 1)
    pos = ca[:, :, None, :] + torch.randn(N, L, A, 3, generator=g, device=dev) * (1.2 if A == 15 else 0.9)
    mask = torch.rand(N, L, A, generator=g, device=dev) < 0.9
    move = torch.zeros(G, L, dtype=torch.bool, device=dev)
    move[:, max(0, n1 - moved):n1] = True
    link = torch.ones(G, L, dtype=torch.bool, device=dev)
    link[:, n1 - 1] = False
    link[:, L - 1] = False
    return pos.contiguous(), mask.contiguous(), move, link


def events(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='16x8x256x5,100x100x256x5,1000x1x48x5,16x8x256x15')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--moved', type=int, default=24, help='moved residues per candidate')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for shape in args.shapes.split(','):
        G, S, L, A = (int(v) for v in shape.split('x'))
        pos, mask, move, link = make(G, S, L, A, args.moved, dev)
        out = torch.empty_like(pos)
        group = torch.where(move, 1, 2).int()
        n_moved = int(move[0].sum())
        bounded = events(lambda: hip.relax_grouped(pos, mask, move, link=link, iters=args.iters, out=out, max_moved=n_moved))
        default = events(lambda: hip.relax_grouped(pos, mask, move, link=link, iters=args.iters, out=out))
        geom = events(lambda: (hip.interface_geometry_grouped(pos, mask, group, link=link, bond_max=2.0),
                               hip.interface_geometry_grouped(out, mask, group, link=link, bond_max=2.0)))
        e = hip.relax_grouped(pos, mask, move, link=link, iters=args.iters, out=out, max_moved=n_moved)['energy'].double().sum(0)
        before = hip.interface_geometry_grouped(pos, mask, group, link=link, bond_max=2.0)
        after = hip.interface_geometry_grouped(out, mask, group, link=link, bond_max=2.0)
        fmt = lambda t: f'{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})'
        terms = ', '.join(f'{n} {float(a):.4g} -> {float(b):.4g}' for n, a, b in zip(('bond', 'ca', 'clash', 'tether'), e[0], e[1]))
        print(f'{G} x {S} x {L} x {A}, {n_moved} moved, iters = {args.iters}: relax_grouped with max_moved = {n_moved} {fmt(bounded)} | with the default bound '
              f'{fmt(default)} | two interface_geometry_grouped calls {fmt(geom)} | energy summed over the candidates: {terms} | clashes '
              f'{int(before["clash"].sum())} -> {int(after["clash"].sum())}, breaks {int(before["breaks"].sum())} -> {int(after["breaks"].sum())}', flush=True)


if __name__ == '__main__':
    main()
