"""Device time of hip.backbone_conformation_grouped beside hip.interface_energy_grouped on the same inputs.

    python tools/bench_backbone.py [--shapes 1x64x256x5,16x8x256x5,1000x1x48x5,16x8x256x15]

Per shape G x S x L x A (those of tools/bench_interface_energy.py: P = 64 poses of L = 256 as one group, 16 x 8 re-docks, 1000 single candidates of L = 48):
the Python call, by events, median of 10 calls (smallest - largest), every row scored, with the default three regions; hip.interface_energy_grouped with its
default knobs beside it; what the scorer found, summed over the candidates.  Structures are that benchmark's generator: random atoms around a CA random walk
are no backbone -- the bond term runs as often as in a real chain, the torsions are uniform noise and what is found means nothing."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

from ab_opt_amd import hip  # noqa: E402
from bench_interface_energy import events, make  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='1x64x256x5,16x8x256x5,1000x1x48x5,16x8x256x15')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    col = {name: k for k, name in enumerate(hip.BACKBONE_COUNTS)}
    for shape in args.shapes.split(','):
        G, S, L, A = (int(v) for v in shape.split('x'))
        pos, mask, group, link, seqs = make(G, S, L, A, dev)
        rows = torch.ones(G, L, dtype=torch.bool, device=dev)
        conf = events(lambda: hip.backbone_conformation_grouped(pos, mask, rows, seqs=seqs, link=link))
        energy = events(lambda: hip.interface_energy_grouped(pos, mask, group, seqs, link=link))
        n = hip.backbone_conformation_grouped(pos, mask, rows, seqs=seqs, link=link)['count'].sum(0).cpu()
        fmt = lambda t: f'{t[0] * 1000:.1f} us ({t[1] * 1000:.1f}-{t[2] * 1000:.1f})'
        print(f'{G} x {S} x {L} x {A}: backbone_conformation_grouped {fmt(conf)} | interface_energy_grouped {fmt(energy)} | summed over the candidates: '
              f'{int(n[col["phipsi"]])} residues with phi and psi, {int(n[col["outliers"]])} outliers, {int(n[col["cis"]])} cis, {int(n[col["twisted"]])} twisted, '
              f'{int(n[col["hb_donor"]])} hydrogen bonds, states H/E/G/I/T/C ' + '/'.join(str(int(n[col[c]])) for c in 'HEGITC'), flush=True)


if __name__ == '__main__':
    main()
