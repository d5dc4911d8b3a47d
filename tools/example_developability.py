"""Dock a few poses of a synthetic complex with hash-filled weights, redesign the loop on each pose and print what every design is, chemically
(sampler.developability).

    python tools/example_developability.py [--poses 4 --designs 3 --steps 20 --contig 33-39 --rows generated|antibody --radius 10 --run-min 5 --points 128]

Per design: the sequence of the redesigned stretch, the liabilities that count against the design (a motif counts if one of its residues is a scored row, so a
sequon completed beside a framework Asn is listed), the net charge and mean hydropathy of the scored rows, and the exposed hydrophobic patches of the unbound
antibody: SAP-like sum, the largest patch and its residue, apolar and polar exposed area.  The weights are not a trained checkpoint and the complex is synthetic,
so the numbers show the call, nothing about antibodies.  The area is that of five backbone + CB slots: a coarse-grained patch score comparable between the
candidates of one complex, not a published SAP value; Kyte-Doolittle, 10 A and run_min = 5 are conventional values, not tuned ones."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ab_opt_amd import geometry, get_model, hip, sampler  # noqa: E402
from ab_opt_amd.model import AA_LETTERS, LIABILITY_NAMES, generate_mask_from_str  # noqa: E402
from ab_opt_amd.utils import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', type=int, default=4)
    ap.add_argument('--designs', type=int, default=3, help='designs per pose')
    ap.add_argument('--steps', type=int, default=20, help='T, the steps both models are built with')
    ap.add_argument('--contig', default='33-39', help='the redesigned stretch, 1-based and inclusive')
    ap.add_argument('--rows', choices=('generated', 'antibody'), default='generated', help='the rows the liabilities, charge and hydropathy are scored on')
    ap.add_argument('--radius', type=float, default=10.0)
    ap.add_argument('--run-min', type=int, default=5)
    ap.add_argument('--points', type=int, default=128)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    dock = synth.build_model(args.steps, 3, device=dev)
    design = synth.fill_module_(get_model(synth.AttrDict(synth.cfg_abdock(args.steps, resolution='backbone+CB'))).eval(), seed=4).to(dev)
    one = {k: v.to(dev) for k, v in synth.make_batch(1, synth.LAYOUT_128, seed=21).items()}
    P, S = args.poses, args.designs
    rep = lambda t, n: t.expand(n, *t.shape[1:]).contiguous()
    gen = one['generate_flag'][0]
    t1 = sampler.sample_replicated(dock, one, P, dict(sample_structure=True, sample_sequence=False, seed=args.seed, rng_offset=0))[0]
    g1 = rep(gen[None], P)
    pose_pos, pose_mask = geometry.reconstruct_backbone_partially(rep(one['pos_heavyatom'], P), hip.so3_exp(t1[0]), t1[1], torch.where(g1, t1[2], rep(one['aa'], P)),
                                                                  rep(one['chain_nb'], P), rep(one['res_nb'], P), rep(one['mask_heavyatom'], P), g1)
    dflag = gen & generate_mask_from_str(args.contig, gen)
    cx = [dict(one, pos_heavyatom=pose_pos[i:i + 1], mask_heavyatom=pose_mask[i:i + 1], generate_flag=dflag[None]) for i in range(P)]
    t2 = sampler.sample_grouped(design, cx, S, dict(sample_structure=False, sample_sequence=True, seed=args.seed + 1, rng_offset=0))[0]
    g2 = rep(dflag[None], P * S)
    seqs = torch.where(g2, t2[2], rep(one['aa'], P * S))
    pos, mask = geometry.reconstruct_backbone_partially(pose_pos.repeat_interleave(S, 0), hip.so3_exp(t2[0]), t2[1], seqs, rep(one['chain_nb'], P * S),
                                                        rep(one['res_nb'], P * S), pose_mask.repeat_interleave(S, 0), g2)
    batch = {k: rep(one[k], P) for k in ('fragment_type', 'chain_nb', 'res_nb')}
    batch['generate_flag'] = rep(dflag[None], P)
    res = sampler.developability(batch, seqs, pos, mask, rows=args.rows, radius=args.radius, run_min=args.run_min, points=args.points)
    host = {k: v.cpu() for k, v in res.items()}
    letters = AA_LETTERS + 'X' * 236
    where = dflag.nonzero()[:, 0].cpu().tolist()
    print(f"{P} poses x {S} designs of {seqs.shape[1]} residues, {len(where)} redesigned ({args.contig}), rows = {args.rows}, radius {args.radius} A, run_min {args.run_min}")
    print('pose design  stretch' + ' ' * max(1, len(where) - 6) + 'liabilities' + ' ' * 22 + 'charge  gravy     SAP   largest patch (residue)  apolar / polar area (A^2)')
    for c in range(P * S):
        stretch = ''.join(letters[int(seqs[c, r])] for r in where)
        found = ', '.join(f'{name} {int(host[name][c])}' for name in LIABILITY_NAMES if int(host[name][c])) or 'none'
        print(f"{c // S:4d} {c % S:6d}  {stretch}  {found:<32s} {int(host['net_charge'][c]):+5d}  {float(host['gravy'][c]):+6.2f}  {float(host['sap'][c]):7.0f}  "
              f"{float(host['patch_max'][c]):8.0f} ({int(host['patch_argmax'][c]) + 1:3d})           {float(host['apolar_area'][c]):6.0f} / {float(host['polar_area'][c]):<6.0f}")


if __name__ == '__main__':
    main()
