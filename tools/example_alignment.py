"""Redesign the loop of a synthetic complex with hash-filled weights and compare every design with the native loop with ONE RESIDUE REMOVED, placed in another
frame (sampler.aligned_rmsd): the aligned strings and three RMSDs side by side.

    python tools/example_alignment.py [--designs 6 --steps 20 --contig 33-39 --mismatch -1 --gap-open -4 --gap-extend -1]

Per design: the two gapped strings of THE alignment (model.alignment_strings), seqid and the number of aligned pairs, and
    aligned     sampler.aligned_rmsd: CA superposed on the aligned pairs and measured on them -- the frame does not enter;
    gapped      sampler.similarity: the reference's gapped CA RMSD without superposition -- it measures the displacement of the frame;
    by rank     sampler.superposed_rmsd: -1, because the two loops differ in length and it pairs by rank.
The designs keep the native backbone outside the redesigned stretch, so `aligned` is small where the alignment pairs the residues that correspond.  The weights
are not a trained checkpoint and the complex is synthetic, so the numbers show the calls, nothing about antibodies."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ab_opt_amd import geometry, get_model, hip, sampler  # noqa: E402
from ab_opt_amd.model import alignment_strings, generate_mask_from_str, identity_table  # noqa: E402
from ab_opt_amd.utils import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--designs', type=int, default=6)
    ap.add_argument('--steps', type=int, default=20, help='T, the steps the model is built with')
    ap.add_argument('--contig', default='33-39', help='the redesigned stretch, 1-based and inclusive')
    ap.add_argument('--mismatch', type=int, default=-1, help='the score of two different types; equal types score 2')
    ap.add_argument('--gap-open', type=int, default=-4)
    ap.add_argument('--gap-extend', type=int, default=-1)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    design = synth.fill_module_(get_model(synth.AttrDict(synth.cfg_abdock(args.steps, resolution='backbone+CB'))).eval(), seed=4).to(dev)
    one = {k: v.to(dev) for k, v in synth.make_batch(1, synth.LAYOUT_128, seed=21).items()}
    S = args.designs
    rep = lambda t, n: t.expand(n, *t.shape[1:]).contiguous()
    gen = one['generate_flag'][0]
    dflag = gen & generate_mask_from_str(args.contig, gen)
    t2 = sampler.sample_grouped(design, [dict(one, generate_flag=dflag[None])], S, dict(sample_structure=False, sample_sequence=True, seed=args.seed, rng_offset=0))[0]
    g2 = rep(dflag[None], S)
    seqs = torch.where(g2, t2[2], rep(one['aa'], S))
    pos, mask = geometry.reconstruct_backbone_partially(rep(one['pos_heavyatom'], S), hip.so3_exp(t2[0]), t2[1], seqs, rep(one['chain_nb'], S), rep(one['res_nb'], S),
                                                        rep(one['mask_heavyatom'], S), g2)
    where = gen.nonzero()[:, 0]
    n, mid = len(where), len(where) // 2
    keep = torch.cat([torch.arange(mid), torch.arange(mid + 1, n)]).to(dev)         # the native loop with its middle residue removed ...
    g = torch.Generator(device=dev).manual_seed(args.seed + 1)
    rot, shift = hip.so3_exp(torch.randn(1, 3, generator=g, device=dev) * 1.5)[0], torch.randn(3, generator=g, device=dev) * 20.0
    ref_seqs = one['aa'][0, where][keep][None]
    ref_ca = (one['pos_heavyatom'][0, where, 1][keep] @ rot.T + shift)[None]         # ... in another frame
    gaps = dict(table=identity_table(2, args.mismatch), gap_open=args.gap_open, gap_extend=args.gap_extend)
    al = sampler.aligned_rmsd(one, seqs, pos, mask, ref_seqs=ref_seqs, ref_ca=ref_ca, **gaps)
    gapped = sampler.similarity(one, seqs, pos, mask, ref_seqs=ref_seqs, ref_ca=ref_ca, **gaps)['rmsd']
    ranked = sampler.superposed_rmsd(one, pos, mask, ref_ca=ref_ca)['rmsd']
    print(f'{S} designs of a loop of {n} residues ({args.contig} redesigned) against the native loop without residue {mid}, moved by about '
          f'{float(shift.norm()):.0f} A; identity table 2 / {args.mismatch}, gaps {args.gap_open} / {args.gap_extend}')
    print('design  seqid  pairs  RMSD: aligned  gapped  by rank   the alignment (design over reference)')
    for c in range(S):
        sa, sb = alignment_strings(al['ops'][c, 0].cpu(), seqs[c].cpu(), ref_seqs[0].cpu(), qmask=(gen & mask[c, :, 1].bool()).cpu())
        print(f"{c:6d}  {float(al['seqid'][c, 0]):5.1f}  {int(al['n_pairs'][c, 0]):5d}  {float(al['rmsd'][c, 0]):13.2f}  {float(gapped[c, 0]):6.2f}  "
              f"{float(ranked[c, 0]):7.2f}   {sa}")
        print(' ' * 59 + sb)


if __name__ == '__main__':
    main()
