"""Device time of hip.align_sequences and hip.gapped_rmsd beside their numpy statements.

    python tools/bench_similarity.py [--shapes 128x1,128x1024,1000x1000 --lengths 16,256 --sample 6]

Per shape Q x R and length n (every row n residues, NULL masks): the Python call, by events, median of 10 calls (smallest - largest); for gapped_rmsd the
kernel launch plus the torch operations that form rmsd.  Beside them the numpy statements of tests/similarity_statement.py (align_pair, sd_pair: a row of
the table per numpy call) timed on --sample pairs and scaled to Q R pairs.  Sequences are uniform over the twenty types, the table is model.identity_table(),
gaps -20 / -1; coordinates are random walks of 3.8 A steps.  Every pair runs the whole n x n table: there is no band and no early exit to favour an input."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import similarity_statement as st  # noqa: E402
from ab_opt_amd import hip, model  # noqa: E402


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
    ap.add_argument('--shapes', default='128x1,128x1024,1000x1000')
    ap.add_argument('--lengths', default='16,256')
    ap.add_argument('--sample', type=int, default=6, help='pairs the numpy statements are timed on')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    table = model.identity_table()
    tdev = table.to(dev)
    fmt = lambda t: f'{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})'
    for n in (int(v) for v in args.lengths.split(',')):
        rng = np.random.default_rng(n)
        a, b = rng.integers(0, 20, (args.sample, n)), rng.integers(0, 20, (args.sample, n))
        ca, cb = (rng.normal(size=(2, args.sample, n, 3)).cumsum(2) * 2.2).astype(np.float32)
        t0 = time.perf_counter()
        for k in range(args.sample):
            st.align_pair(a[k], b[k], table.numpy(), -20, -1)
        t1 = time.perf_counter()
        for k in range(args.sample):
            st.sd_pair(ca[k], cb[k][:max(1, n // 2)])                # half the length: the widest band there is
        t2 = time.perf_counter()
        np_align, np_sd = (t1 - t0) / args.sample, (t2 - t1) / args.sample
        for shape in args.shapes.split(','):
            Q, R = (int(v) for v in shape.split('x'))
            g = torch.Generator(device=dev).manual_seed(Q * R + n)
            q, r = (torch.randint(0, 20, (k, n), generator=g, device=dev).to(torch.uint8) for k in (Q, R))
            walk = lambda k, m: (torch.randn(k, m, 3, generator=g, device=dev) * 2.2).cumsum(1).contiguous()
            qca, rca, rhalf = walk(Q, n), walk(R, n), walk(R, max(1, n // 2))
            al = events(lambda: hip.align_sequences(q, r, tdev, -20, -1))
            same = events(lambda: hip.gapped_rmsd(qca, rca))
            half = events(lambda: hip.gapped_rmsd(qca, rhalf))
            print(f'{Q} x {R} pairs of length {n}: align_sequences {fmt(al)} | gapped_rmsd, equal lengths {fmt(same)}, against half the length {fmt(half)} | '
                  f'numpy statements scaled from {args.sample} pairs: alignment {np_align * Q * R:.2f} s, sd against half the length {np_sd * Q * R:.2f} s', flush=True)


if __name__ == '__main__':
    main()
