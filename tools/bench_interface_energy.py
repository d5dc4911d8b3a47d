"""Device time of hip.interface_energy_grouped beside hip.interface_geometry_grouped on the same inputs.

    python tools/bench_interface_energy.py [--shapes 1x64x256x5,16x8x256x5,1000x1x48x5,16x8x256x15]

Per shape G x S x L x A (the screen's: P = 64 poses of L = 256 as one group, 16 x 8 re-docks, 1000 single candidates of L = 48): the Python call, by events,
median of 10 calls (smallest - largest), without and with the placeholder pair table, and hip.interface_geometry_grouped with its default cutoffs; what the
scorer found, summed over the candidates.  Structures are the scorer benchmarks' generator made on the device (tools/bench_sasa.py): two CA random walks of
3.8 A steps 6 A apart, atoms normal(0.9 A) around their CA, the first third of the row side 1; types uniform over the twenty; the links follow the walks.
Random atoms around a CA are no backbone: the hydrogen-bond term runs (the 9 A rule passes as often as in a real interface) but what it finds means nothing."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ab_opt_amd import hip, model, sampler  # noqa: E402


def make(G, S, L, A, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    N, n1 = G * S, max(1, L // 3)
    step = torch.randn(N, L, 3, generator=g, device=dev)
    step = step * (3.8 / step.norm(dim=-1, keepdim=True))
    ca = torch.cat([step[:, :n1].cumsum(1), step[:, n1:].cumsum(1) + torch.tensor([6.0, 0.0, 0.0], device=dev)], 1)
    pos = ca[:, :, None, :] + torch.randn(N, L, A, 3, generator=g, device=dev) * (1.2 if A == 15 else 0.9)
    mask = torch.rand(N, L, A, generator=g, device=dev) < 0.9
    group = torch.full((G, L), 2, dtype=torch.int32, device=dev)
    group[:, :n1] = 1
    link = torch.ones(G, L, dtype=torch.bool, device=dev)
    link[:, n1 - 1] = False
    link[:, L - 1] = False
    seqs = torch.randint(0, 20, (N, L), generator=g, device=dev).to(torch.uint8)
    return pos.contiguous(), mask.contiguous(), group, link, seqs


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
    ap.add_argument('--shapes', default='1x64x256x5,16x8x256x5,1000x1x48x5,16x8x256x15')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    table = model.hydrophobic_contact_table().to(dev)
    for shape in args.shapes.split(','):
        G, S, L, A = (int(v) for v in shape.split('x'))
        pos, mask, group, link, seqs = make(G, S, L, A, dev)
        plain = events(lambda: hip.interface_energy_grouped(pos, mask, group, seqs, link=link))
        tabled = events(lambda: hip.interface_energy_grouped(pos, mask, group, seqs, pair_table=table, link=link))
        geom = events(lambda: hip.interface_geometry_grouped(pos, mask, group, link=link))
        s = sampler.energy_summary(hip.interface_energy_grouped(pos, mask, group, seqs, pair_table=table, link=link), group)
        fmt = lambda t: f'{t[0] * 1000:.1f} us ({t[1] * 1000:.1f}-{t[2] * 1000:.1f})'
        print(f'{G} x {S} x {L} x {A}: interface_energy_grouped {fmt(plain)} | with a pair table {fmt(tabled)} | interface_geometry_grouped {fmt(geom)} | '
              f'summed over the candidates: {int(s["hbonds"].sum())} hydrogen bonds, {int(s["salt_bridges"].sum())} salt bridges, {int(s["like_pairs"].sum())} '
              f'like-charge pairs, {int(s["pair_contacts"].sum())} contacts', flush=True)


if __name__ == '__main__':
    main()
