"""Dock a few poses of a synthetic complex with hash-filled weights, redesign the loop on each pose and print whether the generated backbone of every design is
a plausible polypeptide (sampler.backbone_conformation).

    python tools/example_backbone.py [--poses 4 --designs 3 --steps 20 --contig 33-39 --hb-cutoff -0.5 --rows generated]

Per design: the sequence of the redesigned stretch, its DSSP-LIKE states (H, E, G, I, T, C; '-' = not scored), the Ramachandran outliers among the scored
residues with phi and psi, cis and twisted peptides, and the longest C-N bond.  The states come from Kabsch & Sander's patterns on single hydrogen bonds: this is
NOT DSSP (no ladders or sheets, no B / E distinction, no bends, no helix trimming), and the three Ramachandran boxes are this library's coarse convention
(model.RAMA_REGIONS), not a published contour.  The weights are not a trained checkpoint and the complex is synthetic, so the numbers show the call, nothing
about antibodies."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ab_opt_amd import geometry, get_model, hip, sampler  # noqa: E402
from ab_opt_amd.model import AA_LETTERS, SS_LETTERS, generate_mask_from_str  # noqa: E402
from ab_opt_amd.utils import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', type=int, default=4)
    ap.add_argument('--designs', type=int, default=3, help='designs per pose')
    ap.add_argument('--steps', type=int, default=20, help='T, the steps both models are built with')
    ap.add_argument('--contig', default='33-39', help='the redesigned stretch, 1-based and inclusive')
    ap.add_argument('--hb-cutoff', type=float, default=-0.5)
    ap.add_argument('--rows', default='generated', choices=('generated', 'antibody'))
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
    batch = {k: rep(one[k], P) for k in ('fragment_type', 'chain_nb', 'res_nb', 'generate_flag')}
    res = sampler.backbone_conformation(batch, pos, mask, rows=args.rows, seqs=seqs, hb_cutoff=args.hb_cutoff)
    host = {k: v.cpu() for k, v in res.items()}
    letters = AA_LETTERS + 'X' * 236
    where = dflag.nonzero()[:, 0].cpu().tolist()
    shown = range(max(0, where[0] - 4), min(seqs.shape[1], where[-1] + 5)) if where else range(0)
    print(f"{P} poses x {S} designs of {seqs.shape[1]} residues, {len(where)} redesigned ({args.contig}), rows scored: {args.rows}, hb_cutoff {args.hb_cutoff} kcal/mol, "
          f"three coarse Ramachandran boxes (this library's convention)")
    print(f'pose design  stretch  states {shown.start + 1}-{shown.stop}' + ' ' * max(1, len(shown) - 12) + 'scored  phi+psi  outliers  cis  twisted  hbonds  max C-N')
    for c in range(P * S):
        stretch = ''.join(letters[int(seqs[c, r])] for r in where)
        states = ''.join(SS_LETTERS[int(host['state'][c, r])] if int(host['state'][c, r]) < len(SS_LETTERS) else '-' for r in shown)
        print(f"{c // S:4d} {c % S:6d}  {stretch}  {states}  {int(host['scored'][c]):6d} {int(host['count'][c, 1]):8d} {int(host['outliers'][c]):9d} {int(host['cis'][c]):4d} "
              f"{int(host['twisted'][c]):8d} {int(host['hbonds'][c]):7d}  {float(host['bond'][c, :, 0].max()):7.2f}")
    held = host['freq'].sum(0)
    print('residues in a helix_4 or a bridge in the most designs:',
          ', '.join(f'{int(r) + 1} ({int(held[r])})' for r in held.argsort(descending=True)[:8] if held[r] > 0) or 'none')


if __name__ == '__main__':
    main()
