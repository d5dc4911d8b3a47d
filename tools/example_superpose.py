"""Sample loop conformations on a synthetic complex with hash-filled weights, place each of them into the frames of several poses, and cluster the loops by
SHAPE across the poses (sampler.cluster_shapes, sampler.superposed_rmsd).

    python tools/example_superpose.py [--poses 3 --designs 4 --steps 10 --cutoff 1.5 --seed 0]

The structure model samples --designs loop conformations; every one of them is then placed, antibody and all, into --poses frames (pose 0 keeps the native
frame, the others are moved by a random rotation and translation that stands for where docking would have put them: the hash-filled model docks nothing
meaningful, and its conformations share nothing, so the copies are what there is to find).  Printed: the clusters `cluster_poses` finds (no superposition:
it cannot merge across frames) next to those of `cluster_shapes` (one cluster per conformation, one member per pose); every design's loop RMSD to the native
loop, fitted on the loop itself and fitted on the antibody's framework; and, for design 0 of pose 0 against its copy in pose 1, the unsuperposed rmsd of
`similarity` (the size of the displacement) next to the superposed one (rounding).  The weights are not a trained checkpoint and the complex is synthetic, so
the numbers show the calls, nothing about antibodies."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ab_opt_amd import geometry, hip, sampler, screen  # noqa: E402
from ab_opt_amd.utils import synth  # noqa: E402


def random_motion(g, shift, dev):
    """a random rotation (hip.so3_exp of a random vector) and a translation of about `shift` A per axis"""
    return hip.so3_exp(torch.randn(1, 3, generator=g, device=dev) * 1.5)[0], torch.randn(3, generator=g, device=dev) * shift


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', type=int, default=3)
    ap.add_argument('--designs', type=int, default=4, help='loop conformations per pose')
    ap.add_argument('--steps', type=int, default=10, help='T, the steps the model is built with')
    ap.add_argument('--cutoff', type=float, default=1.5, help='Angstrom, for both clusterings')
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    model = synth.build_model(args.steps, 3, device=dev)
    one = {k: v.to(dev) for k, v in synth.make_batch(1, synth.LAYOUT_128, seed=21).items()}
    P, S = args.poses, args.designs
    N = P * S
    rep = lambda t, n: t.expand(n, *t.shape[1:]).contiguous()
    gen = one['generate_flag'][0]
    t1 = sampler.sample_replicated(model, one, S, dict(sample_structure=True, sample_sequence=False, seed=args.seed, rng_offset=0))[0]
    g1 = rep(gen[None], S)
    pos, mask = geometry.reconstruct_backbone_partially(rep(one['pos_heavyatom'], S), hip.so3_exp(t1[0]), t1[1], torch.where(g1, t1[2], rep(one['aa'], S)),
                                                        rep(one['chain_nb'], S), rep(one['res_nb'], S), rep(one['mask_heavyatom'], S), g1)
    pos, mask = pos.repeat(P, 1, 1, 1), mask.repeat(P, 1, 1)        # design d of pose p is row p S + d
    antibody = screen.chain_groups(one['fragment_type'])[0] == 1
    g = torch.Generator(device=dev).manual_seed(args.seed + 1)
    for p in range(1, P):                                           # pose 0 keeps the native frame
        R, t = random_motion(g, 20.0, dev)
        rows = slice(p * S, (p + 1) * S)
        pos[rows, antibody] = pos[rows, antibody] @ R.T + t
    where = gen.nonzero()[:, 0]
    ca = pos[:, where, 1].contiguous()
    by_pose = sampler.cluster_poses(ca, args.cutoff)
    by_shape = sampler.cluster_shapes(ca, args.cutoff)
    own = sampler.superposed_rmsd(one, pos, mask, fit='generated')
    framework = sampler.superposed_rmsd(one, pos, mask, fit='context', score='generated')
    print(f'{S} loop conformations of {len(where)} residues, each in the frames of {P} poses: {N} structures; cutoff {args.cutoff} A')
    print(f"cluster_poses  (no superposition): {len(by_pose['centre'])} clusters, sizes {by_pose['size'].tolist()}")
    print(f"cluster_shapes (superposed)      : {len(by_shape['centre'])} clusters, sizes {by_shape['size'].tolist()}, centres {by_shape['centre'].tolist()}")
    print('design pose  shape cluster  pose cluster  loop RMSD to the native: fitted on the loop   fitted on the framework')
    for c in range(N):
        print(f"{c:6d} {c // S:4d}  {int(by_shape['label'][c]):13d}  {int(by_pose['label'][c]):12d}  {float(own['rmsd'][c]):43.2f}  {float(framework['rmsd'][c]):24.2f}")
    seqs = one['aa']
    ref = ca[S:S + 1] if P > 1 else ca[:1]                          # design 0 in the frame of pose 1
    plain = sampler.similarity(one, seqs, pos[:1], mask[:1], ref_ca=ref)['rmsd'][0, 0]
    fitted = sampler.superposed_rmsd(one, pos[:1], mask[:1], ref_ca=ref)['rmsd'][0, 0]
    print(f'design 0 of pose 0 against its copy in pose 1: similarity rmsd (no superposition) {float(plain):.2f} A, superposed rmsd {float(fitted):.2e} A')


if __name__ == '__main__':
    main()
