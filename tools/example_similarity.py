"""Redesign the loop of a synthetic complex with hash-filled weights and print how close every design is to the native loop and to a panel of loops of OTHER
lengths (sampler.similarity): the `seqid` and `rmsd` of the reference's eval stage.

    python tools/example_similarity.py [--designs 6 --steps 20 --contig 33-39 --mismatch -1 --gap-open -20 --gap-extend -1]

Per design: the redesigned loop, its identity to and gapped CA RMSD from the native loop (the reference's two numbers; no superposition, the designs keep the
native frame), and score / matches / columns against each loop of the panel -- the native loop with one residue removed, with one residue doubled, and
reversed.  End gaps are free, so two sequences whose best overlap scores below 0 are not aligned at all (score 0, no match, every residue a column): with a
mismatch of -2 that is the fate of most hash-filled designs, hence the milder default here.  The table is model.identity_table(2, --mismatch): no BLOSUM62
is shipped (model.substitution_table turns Biopython's into the kernel's table).  The weights are not a trained checkpoint and the complex is synthetic, so
the numbers show the call, nothing about antibodies."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ab_opt_amd import geometry, get_model, hip, sampler  # noqa: E402
from ab_opt_amd.model import AA_LETTERS, generate_mask_from_str, identity_table  # noqa: E402
from ab_opt_amd.utils import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--designs', type=int, default=6)
    ap.add_argument('--steps', type=int, default=20, help='T, the steps the model is built with')
    ap.add_argument('--contig', default='33-39', help='the redesigned stretch, 1-based and inclusive')
    ap.add_argument('--mismatch', type=int, default=-1, help='the score of two different types; equal types score 2')
    ap.add_argument('--gap-open', type=int, default=-20)
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
    gaps = dict(table=identity_table(2, args.mismatch), gap_open=args.gap_open, gap_extend=args.gap_extend)
    native = sampler.similarity(one, seqs, pos, mask, **gaps)                       # rows='generated': the whole loop, of which --contig was redesigned
    where = gen.nonzero()[:, 0]
    loop, ca = one['aa'][0, where], one['pos_heavyatom'][0, where, 1]
    n, mid = len(where), len(where) // 2
    names = ['one removed', 'one doubled', 'reversed']
    keep = [torch.cat([torch.arange(mid), torch.arange(mid + 1, n)]), torch.cat([torch.arange(mid + 1), torch.arange(mid, n)]), torch.arange(n - 1, -1, -1)]
    width = n + 1
    ref_seqs = torch.zeros(3, width, dtype=torch.long, device=dev)
    ref_ca = torch.zeros(3, width, 3, device=dev)
    ref_mask = torch.zeros(3, width, dtype=torch.bool, device=dev)
    for k, idx in enumerate(keep):
        ref_seqs[k, :len(idx)], ref_ca[k, :len(idx)], ref_mask[k, :len(idx)] = loop[idx.to(dev)], ca[idx.to(dev)], True
    panel = sampler.similarity(one, seqs, pos, mask, ref_seqs=ref_seqs, ref_ca=ref_ca, ref_mask=ref_mask, **gaps)
    host = {k: v.cpu() for k, v in native.items()}
    ph = {k: v.cpu() for k, v in panel.items()}
    letters = AA_LETTERS + 'X' * 236
    print(f"{S} designs of a loop of {n} residues ({args.contig} redesigned), identity table 2 / {args.mismatch}, gaps {args.gap_open} / {args.gap_extend}")
    print('design  loop' + ' ' * max(1, n - 2) + 'seqid   rmsd   | ' + ' | '.join(f'{x}: score matches/columns rmsd' for x in names))
    for c in range(S):
        text = ''.join(letters[int(seqs[c, r])] for r in where.tolist())
        cells = ' | '.join(f"{int(ph['score'][c, k]):4d} {int(ph['matches'][c, k]):3d}/{int(ph['columns'][c, k]):<3d} {float(ph['rmsd'][c, k]):6.2f}" for k in range(3))
        print(f"{c:6d}  {text}  {float(host['seqid'][c]):6.1f}  {float(host['rmsd'][c]):5.2f}   | {cells}")


if __name__ == '__main__':
    main()
