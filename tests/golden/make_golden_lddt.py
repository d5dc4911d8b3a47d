#!/usr/bin/env python
"""Generate tests/golden/lddt_small.npz by running lddt() of the REFERENCE (AbDock/src/modules/common/plddt.py) on the CPU.

    python tests/golden/make_golden_lddt.py

Runs only where /root/reference exists (the build container), like make_golden.py; nothing here is imported by the tests, which read the .npz file.
Per L in {7, 65}: four CA random walks of 3.8 A steps as the true structures, each perturbed by normal(0.3 / 1 / 3 / 1 A) as the prediction, a mask [4, L, 1]
with some residues masked out, and the last two residues of every walk moved 60 A and 120 A away along x: farther than the cutoff of 15 A from everything, where the
reference returns eps / eps = 1.0 and this library -1.  The inputs meet the acceptance condition of tests/test_lddt.py (its `repair` moves the later residue of a
pair that sits within 1e-3 A of the cutoff or of a threshold by about 0.05 A) and are kept in the file with the reference's outputs, per residue and pooled.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
REF = '/root/reference'
sys.path.insert(0, os.path.join(REF, 'AbDock'))

from src.modules.common.plddt import lddt      # noqa: E402
import test_lddt                                # noqa: E402

CUTOFF = 15.0


def main():
    rng = np.random.default_rng(20240607)
    out = dict(cutoff=np.float32(CUTOFF))
    for L in (7, 65):
        ref, mod = np.zeros((4, L, 3), dtype=np.float32), np.zeros((4, L, 3), dtype=np.float32)
        mask = np.ones((4, L, 1), dtype=np.float32)
        for b in range(4):
            ca = test_lddt.walk(rng, L)
            ca[-2:, 0] += ca[:, 0].max() - ca[-2:, 0] + np.array([60.0, 120.0])
            pred = ca + rng.normal(size=(L, 3)) * (0.3, 1.0, 3.0, 1.0)[b]
            X = test_lddt.repair(np.stack([ca, pred]).astype(np.float32), rng, CUTOFF)
            assert not test_lddt.violations(X, CUTOFF)[0].any()
            ref[b], mod[b] = X
            mask[b, rng.permutation(L - 2)[:max(1, L // 10)], 0] = 0.0
        t = lambda a: torch.from_numpy(a)
        with torch.no_grad():
            res = lddt(t(mod), t(ref), t(mask), cutoff=CUTOFF, per_residue=True)
            pooled = lddt(t(mod), t(ref), t(mask), cutoff=CUTOFF, per_residue=False)
        assert res.shape == (4, L) and pooled.shape == (4,)
        out.update({f'ref_{L}': ref, f'model_{L}': mod, f'mask_{L}': mask, f'per_residue_{L}': res.numpy(), f'pooled_{L}': pooled.numpy()})
        print(f'L = {L}: pooled {pooled.numpy().round(4).tolist()}')
    np.savez_compressed(os.path.join(HERE, 'lddt_small.npz'), **out)
    print('wrote lddt_small.npz')


if __name__ == '__main__':
    main()
