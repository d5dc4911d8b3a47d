"""Dock a few poses of a synthetic complex with hash-filled weights, redesign the loop on each pose and print what the interface of every design is, chemically
(sampler.interface_energy).

    python tools/example_interface_energy.py [--poses 4 --designs 3 --steps 20 --contig 33-39 --hb-cutoff -0.5 --eps 4 --table]

Per design: the sequence of the redesigned stretch, the backbone hydrogen bonds, salt bridges and like-charge pairs across the interface (each counted once),
the contacts within pair_cutoff, and the three energies (antibody side; the kernel gives a pair's energy to both of its residues).  --table adds
model.hydrophobic_contact_table(), a PLACEHOLDER that counts hydrophobic contacts with a minus sign: no statistical potential is shipped.  The weights are not a
trained checkpoint and the complex is synthetic, so the numbers show the call, nothing about antibodies.  The score reads five backbone + CB slots -- no side
chains, no water, no screening: comparable between the candidates of one complex, NOT a binding free energy; every constant is a conventional value, not a
tuned one."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ab_opt_amd import geometry, get_model, hip, sampler  # noqa: E402
from ab_opt_amd.model import AA_LETTERS, generate_mask_from_str, hydrophobic_contact_table  # noqa: E402
from ab_opt_amd.utils import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', type=int, default=4)
    ap.add_argument('--designs', type=int, default=3, help='designs per pose')
    ap.add_argument('--steps', type=int, default=20, help='T, the steps both models are built with')
    ap.add_argument('--contig', default='33-39', help='the redesigned stretch, 1-based and inclusive')
    ap.add_argument('--hb-cutoff', type=float, default=-0.5)
    ap.add_argument('--eps', type=float, default=4.0)
    ap.add_argument('--table', action='store_true', help='add the placeholder hydrophobic contact table as the pair term')
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
    res = sampler.interface_energy(batch, seqs, pos, mask, pair_table=hydrophobic_contact_table() if args.table else None, hb_cutoff=args.hb_cutoff, eps=args.eps)
    host = {k: v.cpu() for k, v in res.items()}
    letters = AA_LETTERS + 'X' * 236
    where = dflag.nonzero()[:, 0].cpu().tolist()
    print(f"{P} poses x {S} designs of {seqs.shape[1]} residues, {len(where)} redesigned ({args.contig}), antibody against antigen, hb_cutoff {args.hb_cutoff} "
          f"kcal/mol, eps {args.eps} r, pair table {'hydrophobic placeholder' if args.table else 'off'}")
    print('pose design  stretch' + ' ' * max(1, len(where) - 6) + 'hbonds  salt  like  contacts      e_hb    e_elec    e_pair   e_total')
    for c in range(P * S):
        stretch = ''.join(letters[int(seqs[c, r])] for r in where)
        print(f"{c // S:4d} {c % S:6d}  {stretch}  {int(host['hbonds'][c]):6d} {int(host['salt_bridges'][c]):5d} {int(host['like_pairs'][c]):5d} "
              f"{int(host['pair_contacts'][c]):9d}  {float(host['e_hb'][c]):8.2f}  {float(host['e_elec'][c]):8.2f}  {float(host['e_pair'][c]):8.2f}  "
              f"{float(host['e_total'][c]):8.2f}")
    held = host['freq'].sum(0)
    print('residues holding a hydrogen bond or a salt bridge in the most designs:',
          ', '.join(f'{int(r) + 1} ({int(held[r])})' for r in held.argsort(descending=True)[:8] if held[r] > 0) or 'none')


if __name__ == '__main__':
    main()
