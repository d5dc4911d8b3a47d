"""Device time of hip.surface_patches_grouped and hip.sequence_liabilities_grouped beside hip.sasa_grouped, the neighbouring call that
makes the area the patches are formed on, at the same shape.

    python tools/bench_developability.py [--shapes 16x8x256x5,100x100x256x5,1000x1x48x5 --radius 10 --run-min 5 --points 128 --probe 1.4]

Per shape G x S x L x A, by events, median of 10 calls (smallest - largest): the C entry of the patches on preallocated outputs and the Python call; the
liabilities with and without freq; sasa_grouped; and sampler.developability's chain on the same candidates.  Structures are the generator of tools/bench_sasa.py
with two thirds of the residues on side 1; sequences are uniform over the twenty types, a tenth of the positions are scored rows."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ab_opt_amd import hip, sampler  # noqa: E402


def make(G, S, L, A, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    N, n1 = G * S, max(1, -(-2 * L // 3))
    step = torch.randn(N, L, 3, generator=g, device=dev)
    step = step * (3.8 / step.norm(dim=-1, keepdim=True))
    ca = torch.cat([step[:, :n1].cumsum(1), step[:, n1:].cumsum(1) + torch.tensor([6.0, 0.0, 0.0], device=dev)], 1)
    pos = ca[:, :, None, :] + torch.randn(N, L, A, 3, generator=g, device=dev) * 0.9
    mask = torch.rand(N, L, A, generator=g, device=dev) < 0.9
    group = torch.full((G, L), 2, dtype=torch.int32, device=dev)
    group[:, :n1] = 1
    seqs = torch.randint(0, 20, (N, L), generator=g, device=dev, dtype=torch.uint8)
    rows = torch.rand(G, L, generator=g, device=dev) < 0.1
    return pos.contiguous(), mask.contiguous(), group, seqs, rows


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
    ap.add_argument('--shapes', default='16x8x256x5,100x100x256x5,1000x1x48x5')
    ap.add_argument('--radius', type=float, default=10.0)
    ap.add_argument('--run-min', type=int, default=5)
    ap.add_argument('--points', type=int, default=128)
    ap.add_argument('--probe', type=float, default=1.4)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    weight = hip.default_patch_weight(dev)
    for shape in args.shapes.split(','):
        G, S, L, A = (int(v) for v in shape.split('x'))
        pos, mask, group, seqs, rows = make(G, S, L, A, dev)
        N = G * S
        radii = sampler.slot_radii(A)
        sasa = events(lambda: hip.sasa_grouped(pos, mask, group, radii, probe=args.probe, points=args.points))
        area = hip.sasa_grouped(pos, mask, group, radii, probe=args.probe, points=args.points)['area'][..., 0].contiguous()
        patch = torch.empty(N, L, device=dev)
        nbr = torch.empty(N, L, dtype=torch.int32, device=dev)
        entry = lambda: hip._check(hip.lib().abopt_surface_patches_grouped(hip.ptr(pos), hip.ptr(mask), 0, hip.ptr(group), hip.ptr(area), hip.ptr(seqs), 0,
                                                                           hip.ptr(weight), args.radius, G, S, L, A, hip.ptr(patch), hip.ptr(nbr), hip.stream()))
        c_entry = events(entry)
        py_call = events(lambda: hip.surface_patches_grouped(pos, mask, group, area, seqs, radius=args.radius))
        liab = events(lambda: hip.sequence_liabilities_grouped(seqs, S, rows=rows, run_min=args.run_min))
        liab_freq = events(lambda: hip.sequence_liabilities_grouped(seqs, S, rows=rows, run_min=args.run_min, want_freq=True))
        batch = dict(fragment_type=torch.where(group == 1, 1, 3).long(), generate_flag=rows, chain_nb=(group != 1).long(),
                     res_nb=torch.arange(L, device=dev).expand(G, L).contiguous())
        chain = events(lambda: sampler.developability(batch, seqs, pos, mask, probe=args.probe, points=args.points, radius=args.radius, run_min=args.run_min))
        got = hip.surface_patches_grouped(pos, mask, group, area, seqs, radius=args.radius)
        part = got['nbr'] > 0
        lb = hip.sequence_liabilities_grouped(seqs, S, rows=rows, run_min=args.run_min)
        fmt = lambda t: f'{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})'
        print(f'{G} x {S} x {L} x {A}: patches C entry {fmt(c_entry)} | Python call {fmt(py_call)} | liabilities {fmt(liab)} | with freq {fmt(liab_freq)} | '
              f'sasa_grouped {fmt(sasa)} | sampler.developability {fmt(chain)} | {float(got["nbr"][part].float().mean()):.1f} neighbours per residue that takes part, '
              f'{float(lb["counts"][:, 7].float().mean()):.2f} flagged positions per design', flush=True)


if __name__ == '__main__':
    main()
