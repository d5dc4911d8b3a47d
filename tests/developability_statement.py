"""The definitions of the developability scorers (include/abopt.h: abopt_sequence_liabilities_grouped, abopt_surface_patches_grouped)
restated in numpy, and the inputs of tests/test_developability.py.

`liabilities_np` is written from the table of classes with plain loops over anchors and windows -- no regular expression: the window rules (inside the sequence,
every step linked, every byte a type, one scored row) are what it pins.  It also tallies, per class, how many windows counted and how many were turned down for
each reason, so that a test can assert that its inputs reach every rule.  `patches_f32` mirrors the patch definition step by step in np.float32 -- the fused
distance is an exact fused multiply-add, see `fma32` -- and `patches_f64` is the same in float64 on the same fp32 inputs."""
import functools

import numpy as np

AA = 'ACDEFGHIKLMNPQRSTVWY'
KD10 = (18, 25, -35, -35, 28, -4, -32, 45, -39, 38, 19, -35, -16, -35, -45, -8, -7, 42, -9, -13)
NAMES = ('n_glyc', 'deamidation', 'isomerisation', 'cleavage', 'cys', 'met', 'hydrophobic_run')
REASONS = ('end', 'link', 'byte', 'row')
HYDROPHOBIC = frozenset(AA.index(c) for c in 'FILMVWY')
SHIFT = (900.0, -700.0, 500.0)


def encode(s):
    """'NGT' -> bytes; any other character is the byte 20 ('x'), 21 ('y') or 255 ('z')"""
    other = {'x': 20, 'y': 21, 'z': 255}
    return np.array([AA.index(c) if c in AA else other[c] for c in s], dtype=np.uint8)


# ------------------------------------------------------------------------------------------ liabilities
def patterns(run_min):
    """per class, one predicate per position of its window (on a byte < 20)"""
    is_ = lambda *cs: (lambda b, s=frozenset(AA.index(c) for c in cs): b in s)
    pats = [[is_('N'), lambda b: b != AA.index('P'), is_('S', 'T')], [is_('N'), is_('G', 'S')], [is_('D'), is_('G', 'S')], [is_('D'), is_('P')], [is_('C')],
            [is_('M')]]
    pats.append([lambda b: b in HYDROPHOBIC] * run_min if run_min else None)
    return pats


def liabilities_np(seqs, rows, link, run_min):
    """ONE group: seqs (S, n) bytes, rows (n,) or None (all scored), link (n,) or None (all bonded), run_min 0 or 2 .. 16.
    -> dict(flags (S, n) uint8, counts (S, 12) int64, hyd10 (S,) int64, freq (n,) int64, tally {(class, 'counted' | reason): windows})."""
    seqs = np.asarray(seqs)
    S, n = seqs.shape
    scored = np.ones(n, bool) if rows is None else np.asarray(rows).astype(bool)
    bonded = np.ones(n, bool) if link is None else np.asarray(link).astype(bool)
    flags, counts, hyd10 = np.zeros((S, n), np.uint8), np.zeros((S, 12), np.int64), np.zeros(S, np.int64)
    tally = {}
    pats = patterns(run_min)
    for s in range(S):
        x = [int(v) for v in seqs[s]]
        for k in range(n):
            f = 0
            for c, pat in enumerate(pats):
                if pat is None:
                    continue
                w = len(pat)
                have = [(j, x[k + j]) for j in range(w) if k + j < n]
                typed = [(j, b) for j, b in have if b < 20]
                if not typed or not all(pat[j](b) for j, b in typed):
                    continue                                                # not this motif, whatever the rules say
                if len(have) < w:
                    reason = 'end' if len(typed) == len(have) else None     # the motif runs past the end
                elif len(typed) < w:
                    reason = 'byte'                                         # a byte >= 20 inside it
                elif not all(bonded[k + j] for j in range(w - 1)):
                    reason = 'link'
                elif not any(scored[k + j] for j in range(w)):
                    reason = 'row'
                else:
                    reason = 'counted'
                    f |= 1 << c
                    counts[s, c] += 1
                if reason:
                    tally[(c, reason)] = tally.get((c, reason), 0) + 1
            flags[s, k] = f
            counts[s, 7] += f != 0
            if scored[k]:
                b = x[k]
                counts[s, 8] += b in (AA.index('K'), AA.index('R'))
                counts[s, 9] += b in (AA.index('D'), AA.index('E'))
                counts[s, 10] += b == AA.index('H')
                counts[s, 11] += b < 20
                hyd10[s] += KD10[b] if b < 20 else 0
    return dict(flags=flags, counts=counts, hyd10=hyd10, freq=(flags != 0).sum(0).astype(np.int64), tally=tally)


def liabilities_grouped_np(seqs, S, rows, link, run_min):
    """G groups: seqs (G*S, n), rows / link (G, n) or None -> flags, counts, hyd10 per design, freq (G, n), tally summed."""
    G = seqs.shape[0] // S
    outs = [liabilities_np(seqs[g * S:(g + 1) * S], None if rows is None else rows[g], None if link is None else link[g], run_min) for g in range(G)]
    tally = {}
    for o in outs:
        for key, v in o['tally'].items():
            tally[key] = tally.get(key, 0) + v
    return dict(flags=np.concatenate([o['flags'] for o in outs]), counts=np.concatenate([o['counts'] for o in outs]),
                hyd10=np.concatenate([o['hyd10'] for o in outs]), freq=np.stack([o['freq'] for o in outs]), tally=tally)


_EXAMPLE = {0: 'NAT', 1: 'NG', 2: 'DS', 3: 'DP', 4: 'C', 5: 'M'}


def liability_case(G, S, n, run_min, with_rows, with_link, seed=0):
    """Sequences with PLANTED motifs (130 random residues with N, G, S, T, D, P, C, M at triple weight held 0 `DP` and 0 runs of five).  For every class a window
    ending at position 64 and one ending at 65, one at the last possible anchor, one cut off by the end of the sequence, one across an unlinked step, one around
    a byte of 20, of 21 and of 255, one whose only scored row is its last residue, one with no scored row; N-P-S; hydrophobic runs of run_min - 1, run_min and
    run_min + 3 and one that reaches position n - 1.  A later plant may overwrite an earlier one (the sequences are short): the test asserts on the statement,
    over its whole table of cases, that every rule was reached.  -> dict(seqs (G*S, n) uint8, rows (G, n) bool or None, link (G, n) bool or None)."""
    rng = np.random.default_rng(1000 * seed + 131 * n + 17 * run_min + 5 * G + S + 2 * with_rows + with_link)
    N = G * S
    p = np.ones(20)
    p[[AA.index(c) for c in 'NGSTDPCM']] = 3.0
    seqs = rng.choice(20, size=(N, n), p=p / p.sum()).astype(np.uint8)
    rows = (rng.random((G, n)) < 0.7) if with_rows else None
    link = (rng.random((G, n)) < 0.95) if with_link else None
    examples = dict(_EXAMPLE)
    if run_min:
        examples[6] = ''.join('LIVFWYM'[j % 7] for j in range(run_min))
    turn = [0]

    def put(text, k, scored=None, unlink=None):
        """the bytes of `text` from position k of the next design (what falls outside the sequence is dropped); scored: the rows of the window, unlink: a step"""
        d = turn[0] % N
        turn[0] += 1
        b = encode(text)
        for j in range(len(b)):
            if 0 <= k + j < n:
                seqs[d, k + j] = b[j]
                if rows is not None:
                    rows[d // S, k + j] = True if scored is None else scored[j]
                if link is not None and j < len(b) - 1:
                    link[d // S, k + j] = j != unlink
        return d

    free = lambda w: int(rng.integers(0, max(1, n - w + 1)))
    for c, text in examples.items():
        w = len(text)
        if w > 1:
            put(text, free(w), unlink=int(rng.integers(w - 1)))
            for other in 'xyz':
                j = int(rng.integers(1, w))
                put(text[:j] + other + text[j + 1:], free(w))
        put(text, free(w), scored=[False] * (w - 1) + [True])
        put(text, free(w), scored=[False] * w)
        put(text, free(w))
    put('NPS', free(3))
    if run_min:
        for length in (run_min - 1, run_min, run_min + 3):
            put('A' + 'L' * length + 'A', free(length + 2))
    for c, text in examples.items():                                            # the fixed places last, so that they survive
        w = len(text)
        for end in (64, 65):
            put(text, end - w + 1)
        put(text, n - w)
        if w > 1:
            put(text, n - w + 1)
    if run_min:
        put('L' * (run_min + 2), n - run_min - 2)
    return dict(seqs=seqs, rows=rows, link=link)


# ------------------------------------------------------------------------------------------ patches
def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, exactly: the product of two fp32 numbers is exact in float64; the float64 sum with c is corrected to round-to-odd with the
    error term of TwoSum, after which the rounding to fp32 is the single rounding of the fused operation (53 >= 24 + 2 bits)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all='ignore'):
        p = a * b
        s = np.atleast_1d(p + c).copy()
        p, c = np.broadcast_to(p, s.shape), np.broadcast_to(c, s.shape)
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = s.view(np.int64)
        fix = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
        step = np.where((err > 0) == (s > 0), 1, -1)
        s = np.where(fix, (bits + step).view(np.float64), s)
        return s.astype(np.float32)


def _patches(dt, pos, mask, group, area, seqs, weight, radius, margins=False):
    """The definition for ONE candidate in the arithmetic `dt`: pos (L, A, 3), mask (L, A), group (L,), area (L,), seqs (L,) bytes, weight (21,), radius.
    -> dict(patch (L,) dt, nbr (L,) int64, part (L,) bool, near (L, L) bool [, margin (L, L): | |c_i - c_j| - radius | in float64, inf off the participating pairs])."""
    pos, area, weight = np.asarray(pos, dtype=np.float32), np.asarray(area, dtype=np.float32), np.asarray(weight, dtype=np.float32)
    mask, group = np.asarray(mask).astype(bool), np.asarray(group)
    L, A = mask.shape
    r = np.arange(L)
    slot = np.where(mask[:, 4], 4, 1) if A >= 5 else np.ones(L, dtype=np.int64)                 # CB if it is there, else CA
    c = pos[r, slot].astype(dt)
    w = weight[np.minimum(np.asarray(seqs).astype(np.int64), 20)]
    with np.errstate(invalid='ignore', over='ignore'):
        part = (group == 1) & mask[r, slot] & np.isfinite(pos[r, slot]).all(-1) & np.isfinite(area) & (area >= 0) & np.isfinite(w)
        h = w.astype(dt) * area.astype(dt)                                                      # one multiply
        dx, dy, dz = (c[:, None, e] - c[None, :, e] for e in range(3))
        d2 = fma32(dz, dz, fma32(dy, dy, dx * dx)) if dt == np.float32 else (dx * dx + dy * dy) + dz * dz
        thr = dt(np.float32(radius)) * dt(np.float32(radius))
        near = part[:, None] & part[None, :] & (d2 <= thr)
        acc = np.zeros(L, dtype=dt)
        for j in range(L):                                                                      # acc = acc + h_j in ascending j, for every target at once
            acc = np.where(near[:, j], acc + h[j], acc)
    out = dict(patch=acc, nbr=near.sum(1).astype(np.int64), part=part, near=near, h=h)
    if margins:
        with np.errstate(invalid='ignore'):
            d = np.sqrt(((pos[r, slot].astype(np.float64)[:, None] - pos[r, slot].astype(np.float64)[None]) ** 2).sum(-1))
        out['margin'] = np.where(part[:, None] & part[None, :], np.abs(d - float(np.float32(radius))), np.inf)
    return out


def patches_f32(pos, mask, group, area, seqs, weight, radius, **kw):
    return _patches(np.float32, pos, mask, group, area, seqs, weight, radius, **kw)


def patches_f64(pos, mask, group, area, seqs, weight, radius, **kw):
    return _patches(np.float64, pos, mask, group, area, seqs, weight, radius, **kw)


def default_weight():
    return np.array([v / 10.0 for v in KD10] + [0.0], dtype=np.float64).astype(np.float32)


def patches_grouped_f32(pos, mask, group, area, seqs, weight, radius, S):
    """patches_f32 over G groups of S candidates: mask (G*S or G, L, A), seqs (G*S or G, L) -> (patch (G*S, L) float32, nbr (G*S, L) int64, near share)."""
    N, L = pos.shape[:2]
    patch, nbr = np.zeros((N, L), np.float32), np.zeros((N, L), np.int64)
    pairs = near = 0
    for c in range(N):
        g = c // S
        one = patches_f32(pos[c], mask[c] if mask.shape[0] == N else mask[g], group[g], area[c], seqs[c] if seqs.shape[0] == N else seqs[g], weight, radius)
        patch[c], nbr[c] = one['patch'], one['nbr']
        pairs += int(one['part'].sum()) ** 2
        near += int(one['near'].sum())
    return patch, nbr, near / max(1, pairs)


@functools.lru_cache(maxsize=None)
def structure(G, S, L, A, far=False, seed=0):
    """Candidates of the surface tests, built once per shape and treated as read-only: per candidate two CA random walks of 3.8 A steps, the second 6 A along x
    from the first; the first ceil(2 L / 3) residues are side 1 (a third is too few neighbours); atoms normal(0.9 A) around their CA; area uniform in 0 .. 150 A^2;
    types uniform over the twenty.  From L = 7 on, at residues drawn without order: one without atoms, one without CA, one with CB masked out, two of group 0,
    one NaN coordinate in its centre, a NaN and a negative area, and the bytes 20, 21 and 255.  far: rotated and moved by SHIFT.
    -> dict(pos fp32 (G*S, L, A, 3), mask (G*S, L, A), group (G, L) int32, area fp32 (G*S, L), seqs uint8 (G*S, L))."""
    rng = np.random.default_rng(7000 * seed + 37 * L + 11 * A + 3 * G + S)
    N, n1 = G * S, max(1, -(-2 * L // 3))
    group = np.full((G, L), 2, dtype=np.int32)
    group[:, :n1] = 1
    pos = np.zeros((N, L, A, 3))
    mask = np.ones((N, L, A), dtype=bool)
    area = rng.uniform(0.0, 150.0, size=(N, L)).astype(np.float32)
    seqs = rng.integers(0, 20, size=(N, L)).astype(np.uint8)
    if L >= 7:
        for g in range(G):
            group[g, rng.permutation(n1)[:2]] = 0
    for c in range(N):
        first = np.arange(L) < n1
        step = rng.normal(size=(L, 3))
        step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
        ca = np.zeros((L, 3))
        for sel, origin in ((first, np.zeros(3)), (~first, np.array([6.0, 0.0, 0.0]))):
            ca[sel] = origin + np.cumsum(step[sel], 0)
        pos[c] = ca[:, None] + rng.normal(size=(L, A, 3)) * 0.9
    if far:
        rot = np.linalg.qr(np.random.default_rng(99).normal(size=(3, 3)))[0]
        pos = pos @ rot.T + np.array(SHIFT)
    pos = pos.astype(np.float32)
    if L >= 7:
        for c in range(N):
            r = rng.permutation(n1)                                             # the special residues lie on side 1, where they matter
            pick = lambda k: r[k % n1]
            mask[c, pick(0)] = False
            mask[c, pick(1), 1] = False
            if A >= 5:
                mask[c, pick(2), 4] = False
            centre = 4 if A >= 5 and mask[c, pick(3), 4] else 1
            pos[c, pick(3), centre, int(rng.integers(3))] = np.nan
            area[c, pick(4)] = np.nan
            area[c, pick(5)] = -1.0
            seqs[c, pick(6)], seqs[c, pick(7)], seqs[c, pick(8)] = 20, 21, 255
    return dict(pos=pos, mask=mask, group=group, area=area, seqs=seqs)
