"""Dock a few poses of a synthetic complex with hash-filled weights, relax them on the device and print what the relax did, in the units the screen reports
(sampler.relax_candidates).

    python tools/example_relax.py [--poses 8 --steps 20 --move antibody|generated --iters 50 --clash-cutoff 3.0 --bond-max 2.0 --step 0.05 --max-shift 0.1
                                   --max-angle 0.05 --w-bond 1 --w-ca 1 --w-clash 1 --w-tether 0.05]

Per pose: the clashing atom pairs (generated residues against every other residue) and the broken peptide bonds before and after, and the four energy terms
before and after.  The weights are not a trained checkpoint and the complex is synthetic: almost every peptide bond of it is broken to begin with and the
hash-filled model leaves the docked loop some 20 A from its anchors, so the counts say what the descent does to a bad pose, nothing about antibodies.  The
defaults here are a gentle step (0.05, at most 0.1 A and 0.05 rad per iteration) with the whole antibody free to move: the summed clashes and breaks fall.
With --move generated and the library's defaults (--step 0.2 --max-shift 0.5 --max-angle 0.2) the bonds drag the loop back to its anchors, the breaks fall
and the clashes RISE on the way (DESIGN.md section 6.8 has the table).  What a relax does to DockQ, clashes or hit rates of a trained model is unmeasured."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ab_opt_amd import geometry, hip, sampler  # noqa: E402
from ab_opt_amd.utils import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', type=int, default=8)
    ap.add_argument('--steps', type=int, default=20, help='T, the steps the docking model is built with')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--move', choices=('generated', 'antibody'), default='antibody')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--clash-cutoff', type=float, default=3.0)
    ap.add_argument('--bond-max', type=float, default=2.0)
    ap.add_argument('--step', type=float, default=0.05)
    ap.add_argument('--max-shift', type=float, default=0.1)
    ap.add_argument('--max-angle', type=float, default=0.05)
    ap.add_argument('--w-bond', type=float, default=1.0)
    ap.add_argument('--w-ca', type=float, default=1.0)
    ap.add_argument('--w-clash', type=float, default=1.0)
    ap.add_argument('--w-tether', type=float, default=0.05)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    dock = synth.build_model(args.steps, 3, device=dev)
    one = {k: v.to(dev) for k, v in synth.make_batch(1, synth.LAYOUT_128, seed=21).items()}
    n = args.poses
    v, p, s = sampler.sample_replicated(dock, one, n, dict(sample_structure=True, sample_sequence=False, seed=args.seed, rng_offset=0))[0][:3]
    rep = lambda a: a[:1].expand(n, *a.shape[1:]).contiguous()
    gen = rep(one['generate_flag'])
    pos, mask = geometry.reconstruct_backbone_partially(rep(one['pos_heavyatom']), hip.so3_exp(v), p, torch.where(gen, s, rep(one['aa'])), rep(one['chain_nb']),
                                                        rep(one['res_nb']), rep(one['mask_heavyatom']), gen)
    res = sampler.relax_candidates(one, pos, mask, move=args.move, bond_max=args.bond_max, clash_cutoff=args.clash_cutoff, iters=args.iters, step=args.step,
                                   max_shift=args.max_shift, max_angle=args.max_angle, w_bond=args.w_bond, w_ca=args.w_ca, w_clash=args.w_clash,
                                   w_tether=args.w_tether)
    shift = (res['pos'] - pos).norm(dim=-1)
    shift = torch.where(mask, shift, torch.zeros_like(shift)).amax((1, 2))
    e = res['energy'].cpu()
    print(f"{n} poses of {one['aa'].shape[1]} residues, {int(one['generate_flag'].sum())} docked, move = {args.move}, {args.iters} iterations")
    print('pose  clashes       breaks        bond             ca               clash            tether     largest move (A)')
    for i in range(n):
        terms = '  '.join(f'{float(e[i, 0, k]):7.2f}->{float(e[i, 1, k]):<7.2f}' for k in range(4))
        print(f"{i:4d}  {int(res['clashes_before'][i]):4d} -> {int(res['clashes_after'][i]):<4d}  {int(res['breaks_before'][i]):4d} -> {int(res['breaks_after'][i]):<4d}  "
              f'{terms}  {float(shift[i]):.2f}')
    tot = lambda k: int(res[k].sum())
    print(f"all   {tot('clashes_before'):4d} -> {tot('clashes_after'):<4d}  {tot('breaks_before'):4d} -> {tot('breaks_after'):<4d}")


if __name__ == '__main__':
    main()
