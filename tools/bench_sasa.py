"""Device time of hip.sasa_grouped beside the two things it can honestly be compared with on the same inputs: the plain torch statement
of the definition on the device, and hip.interface_geometry_grouped, the neighbouring call of the screen.

    python tools/bench_sasa.py [--shapes 16x8x256x5,100x100x256x5,1000x1x48x5,16x8x256x15 --points 128 --probe 1.4 --torch-candidates 200]

Per shape G x S x L x A: the C entry alone on preallocated outputs and the Python call, by events, median of 10 calls (smallest - largest); the torch statement
(one candidate at a time: a cdist of the candidate's M n test points against its M atoms) over --torch-candidates candidates (0: all), scaled to the shape, with its
peak memory; the share of atom pairs the bounding-sphere prune enters, computed on the host in float64 for the first candidate.  Structures are the tests'
generator made on the device: two CA random walks of 3.8 A steps 6 A apart, atoms normal(0.9 A) around their CA, a third of the residues on side 1."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ab_opt_amd import hip  # noqa: E402

RADII = (1.55, 1.70, 1.70, 1.52, 1.70)


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
    radius = torch.tensor([RADII[a] if a < 5 else 1.70 for a in range(A)], device=dev)
    return pos.contiguous(), mask.contiguous(), group, radius


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


def sasa_torch(pos, mask, group, radius, dirs, probe):
    """The definition for ONE candidate in plain torch, fp32 (cdist: not the definition's rounding) -> pts (4,)."""
    L, A = mask.shape
    part = mask & ((group == 1) | (group == 2))[:, None] & torch.isfinite(pos).all(-1) & (radius > 0) & (radius <= 16)
    c, R = pos[part], radius.expand(L, A)[part] + probe
    side = group[:, None].expand(L, A)[part]
    M, n = c.shape[0], dirs.shape[0]
    q = c[:, None, :] + R[:, None, None] * dirs[None]
    hid = (torch.cdist(q.view(M * n, 3), c, compute_mode='donot_use_mm_for_euclid_dist') < R[None]).view(M, n, M)
    hid[torch.arange(M), :, torch.arange(M)] = False
    same = side[:, None] == side[None, :]
    own = (hid & same[:, None, :]).any(-1)
    other = (hid & ~same[:, None, :]).any(-1)
    free, cplx = (~own).sum(1), (~own & ~other).sum(1)
    return torch.stack([free[side == 1].sum(), free[side == 2].sum(), cplx[side == 1].sum(), cplx[side == 2].sum()])


def prune_share(pos, mask, group, radius, probe):
    """Share of the (target atom, occluder atom) pairs of ONE candidate whose occluder residue the bounding-sphere test of csrc/sasa.hip lets in; float64, host."""
    pos, mask, group = pos.double().cpu().numpy(), mask.cpu().numpy(), group.cpu().numpy()
    L, A = mask.shape
    R = np.broadcast_to(radius.double().cpu().numpy(), (L, A)) + probe
    part = mask & np.isin(group, (1, 2))[:, None]
    cnt = part.sum(1)
    centre = (pos * part[..., None]).sum(1) / np.maximum(cnt, 1)[:, None]
    rb = np.where(part, np.linalg.norm(pos - centre[:, None], axis=-1) + R, -np.inf).max(1)
    res, slot = np.nonzero(part)
    D = np.linalg.norm(pos[res, slot][:, None, :] - centre[None], axis=-1)                  # (M, L)
    enter = (D <= (R[res, slot][:, None] + rb[None]) * (1 + 2.0 ** -16) + 0.01) & (cnt > 0)[None]
    return float((enter * cnt[None]).sum() / max(1, res.size * cnt.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='16x8x256x5,100x100x256x5,1000x1x48x5,16x8x256x15')
    ap.add_argument('--points', type=int, default=128)
    ap.add_argument('--probe', type=float, default=1.4)
    ap.add_argument('--torch-candidates', type=int, default=200, help='candidates the torch statement runs on (0: all); its time is scaled to the shape')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    n, probe = args.points, args.probe
    dirs = hip.sphere_points(n, dev)
    k = float(torch.tensor(4.0 * math.pi / n, dtype=torch.float64).float())
    for shape in args.shapes.split(','):
        G, S, L, A = (int(v) for v in shape.split('x'))
        pos, mask, group, radius = make(G, S, L, A, dev)
        N = G * S
        rad = radius.expand(G, L, A).contiguous()
        pts = torch.empty(N, 4, dtype=torch.int32, device=dev)
        area = torch.empty(N, L, 2, device=dev)
        ws = torch.empty(hip.lib().abopt_sasa_ws_bytes(G, S, L, A), dtype=torch.uint8, device=dev)
        entry = lambda: hip._check(hip.lib().abopt_sasa_grouped(hip.ptr(pos), hip.ptr(mask), 0, hip.ptr(group), hip.ptr(rad), hip.ptr(dirs), n, G, S, L, A, probe, k,
                                                                hip.ptr(pts), hip.ptr(area), hip.ptr(ws), ws.numel(), hip.stream()))
        c_entry = events(entry)
        py_call = events(lambda: hip.sasa_grouped(pos, mask, group, radius, probe=probe, points=n))
        neighbour = events(lambda: hip.interface_geometry_grouped(pos, mask, group))
        got = hip.sasa_grouped(pos, mask, group, radius, probe=probe, points=n)
        m = N if args.torch_candidates == 0 else min(N, args.torch_candidates)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ref = torch.stack([sasa_torch(pos[c], mask[c], group[c // S], radius, dirs, probe) for c in range(m)])
        b.record()
        torch.cuda.synchronize()
        t_torch = a.elapsed_time(b) * N / m
        peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        differ = int((ref != got['pts'][:m]).any(1).sum())
        total = int(mask.sum()) * n
        free, cplx = int(got['pts'][:, :2].sum()), int(got['pts'][:, 2:].sum())
        fmt = lambda t: f'{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})'
        print(f'{G} x {S} x {L} x {A}, n = {n}: C entry {fmt(c_entry)} | Python call {fmt(py_call)} | torch statement {t_torch:.1f} ms for all {N} '
              f'(ran {m}; {differ} of them differ from the kernel in some count), peak {peak:.0f} MB | interface_geometry_grouped {fmt(neighbour)} | '
              f'prune enters {100 * prune_share(pos[0], mask[0], group[0], radius, probe):.1f} % of the atom pairs | free-exposed {free / total:.3f} of the points, '
              f'{(free - cplx) / max(1, free):.3f} of those buried | mean BSA {float((got["area"][..., 0] - got["area"][..., 1]).sum(-1).mean()):.0f} A^2', flush=True)


if __name__ == '__main__':
    main()
