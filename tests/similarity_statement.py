"""The definitions of include/abopt.h for abopt_align_sequences and abopt_gapped_rmsd, restated in numpy (used by tests/test_similarity.py
and tools/bench_similarity.py).

Alignment, integers only: `align_brute` enumerates every alignment of two tiny sequences and prices it by the words of the definition (gap runs, free ends);
`align_slow` is the three-state Gotoh recurrence on tuples (score, matches, -columns) with the lexicographic maximum, cell by cell; `align_pair` is the same
recurrence a row at a time, the tuples folded into one int64 and the horizontal state taken as a running maximum -- the one fast enough for 256 x 256.

Gapped RMSD: `sd_table` is the reference's recurrence as written (tools/eval/similarity.py: reslist_rmsd), cell by cell, in float32 with the fused distance of
the kernels (`fma32`) or in float64; `sd_pair` is the same on the band k = j - i, a row at a time, bit for bit equal to it in float32; `sd_brute` enumerates the
order-preserving placements, all of them or those whose last two residues are adjacent."""
import itertools

import numpy as np

from developability_statement import fma32

NEG = -(1 << 60)


# ------------------------------------------------------------------------------------------ alignment
def _sub(table, x, y):
    T = table.shape[0]
    return int(table[min(int(x), T - 1), min(int(y), T - 1)])


def align_brute(a, b, table, gap_open, gap_extend):
    """Every alignment of a and b -- every word over P (a pair), A (a_i against a gap), B (a gap against b_j) that spells both -- priced by the definition: a
    maximal run of A or of B that touches the first or the last column is free, any other run of k columns costs gap_open + (k - 1) gap_extend; a pair scores
    table[a_i][b_j] and is a match iff the raw bytes are equal.  -> (score, matches, columns) of the lexicographic maximum of (score, matches, -columns)."""
    n, m = len(a), len(b)
    best = None

    def walk(i, j, word):
        nonlocal best
        if i == n and j == m:
            score = matches = 0
            ia = ib = 0
            runs = [(k, len(list(g))) for k, g in itertools.groupby(word)]
            for r, (k, cnt) in enumerate(runs):
                if k == 'P':
                    for _ in range(cnt):
                        score += _sub(table, a[ia], b[ib])
                        matches += int(a[ia] == b[ib])
                        ia += 1
                        ib += 1
                else:
                    if r != 0 and r != len(runs) - 1:
                        score += gap_open + (cnt - 1) * gap_extend
                    if k == 'A':
                        ia += cnt
                    else:
                        ib += cnt
            cand = (score, matches, -len(word))
            if best is None or cand > best:
                best = cand
            return
        if i < n and j < m:
            walk(i + 1, j + 1, word + 'P')
        if i < n:
            walk(i + 1, j, word + 'A')
        if j < m:
            walk(i, j + 1, word + 'B')

    walk(0, 0, '')
    return best[0], best[1], -best[2]


def align_slow(a, b, table, gap_open, gap_extend):
    """The recurrence of include/abopt.h on tuples, cell by cell.  H[i][j]: the best alignment of a[:i] and b[:j]; X: the best that ends with a_i against a gap;
    Y: the best that ends with a gap against b_j.  The first row and column are free leading gaps; the answer is the best of the last row and column with the
    free trailing gap's columns counted."""
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return 0, 0, max(n, m)
    add = lambda t, s, k: (t[0] + s, t[1] + k, t[2] - 1)
    none = (NEG, 0, 0)
    H = [[None] * (m + 1) for _ in range(n + 1)]
    X = [[none] * (m + 1) for _ in range(n + 1)]
    Y = [[none] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        H[i][0] = (0, 0, -i)
    for j in range(m + 1):
        H[0][j] = (0, 0, -j)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            X[i][j] = max(add(H[i - 1][j], gap_open, 0), add(X[i - 1][j], gap_extend, 0))
            Y[i][j] = max(add(H[i][j - 1], gap_open, 0), add(Y[i][j - 1], gap_extend, 0))
            H[i][j] = max(add(H[i - 1][j - 1], _sub(table, a[i - 1], b[j - 1]), int(a[i - 1] == b[j - 1])), X[i][j], Y[i][j])
    cands = [(H[i][m][0], H[i][m][1], H[i][m][2] - (n - i)) for i in range(n + 1)] + [(H[n][j][0], H[n][j][1], H[n][j][2] - (m - j)) for j in range(m + 1)]
    s, k, c = max(cands)
    return s, k, -c


# (score, matches, -columns) as score 2^28 + matches 2^16 - columns: |score| < 2^25, matches <= 256 and columns <= 512, also after the shift by k gap_extend
# steps below (|k| <= 256), so the order of the int64 is the lexicographic one of the tuples
_S, _M = 1 << 28, 1 << 16


def _decode(v):
    v = int(v)
    c = (-v) & 0xffff
    v += c
    return v >> 28, (v >> 16) & 0xfff, c


def align_pair(a, b, table, gap_open, gap_extend):
    """align_slow a row at a time.  X and the diagonal need the row above only; Y[j] = max_{k<j} (G[k] + open + (j - 1 - k) extend) with G = max(diagonal, X)
    (G[0] = H[i][0]) is a running maximum -- equal to the cell-by-cell recurrence because gap_open <= gap_extend."""
    a, b, table = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(table, dtype=np.int64)
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return 0, 0, max(n, m)
    assert gap_open <= gap_extend <= 0
    T = table.shape[0]
    bi = np.minimum(b, T - 1)
    d_open, d_ext = gap_open * _S - 1, gap_extend * _S - 1
    j = np.arange(m + 1, dtype=np.int64)
    H = -j                                                           # row 0
    X = np.full(m + 1, NEG, dtype=np.int64)
    last = [H[m] - n]
    for i in range(1, n + 1):
        pair = table[min(int(a[i - 1]), T - 1), bi] * _S + (a[i - 1] == b) * _M - 1
        G = np.empty(m + 1, dtype=np.int64)
        Xn = np.full(m + 1, NEG, dtype=np.int64)
        Xn[1:] = np.maximum(H[1:] + d_open, X[1:] + d_ext)
        G[0] = -i
        G[1:] = np.maximum(H[:-1] + pair, Xn[1:])
        Z = np.maximum.accumulate(G - j * d_ext)
        Hn = G.copy()
        Hn[1:] = np.maximum(G[1:], Z[:-1] + d_open + j[:-1] * d_ext)
        H, X = Hn, Xn
        last.append(H[m] - (n - i))
    return _decode(max(max(last), int((H - (m - j)).max())))


def align_rows(q, qmask, r, rmask, table, gap_open, gap_extend):
    """Q rows against R rows like the entry point: a row's sequence is its mask-true bytes in order (mask None = all).  -> score, matches, columns (Q, R) int32.
    Equal sequences are aligned once."""
    seq = lambda rows, mask: [tuple(int(v) for v in (row if mask is None else row[np.asarray(mask[k]).astype(bool)])) for k, row in enumerate(np.asarray(rows))]
    qs, rs = seq(q, qmask), seq(r, rmask)
    out = np.zeros((3, len(qs), len(rs)), dtype=np.int32)
    memo = {}
    for x, a in enumerate(qs):
        for y, b in enumerate(rs):
            if (a, b) not in memo:
                memo[a, b] = align_pair(a, b, table, gap_open, gap_extend)
            out[:, x, y] = memo[a, b]
    return out[0], out[1], out[2]


# ------------------------------------------------------------------------------------------ gapped RMSD
def _d(s, l, dt):
    """d between s (..., 3) and l (..., 3): the kernels' fused chain on fp32 differences, or plain float64 on the same fp32 inputs"""
    s, l = np.asarray(s, dtype=np.float32), np.asarray(l, dtype=np.float32)
    if dt == np.float32:
        u = s - l
        return fma32(u[..., 2], u[..., 2], fma32(u[..., 1], u[..., 1], u[..., 0] * u[..., 0])).reshape(u.shape[:-1])
    u = s.astype(np.float64) - l.astype(np.float64)
    return (u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]


def _short_long(q, r):
    q, r = np.asarray(q, dtype=np.float32).reshape(-1, 3), np.asarray(r, dtype=np.float32).reshape(-1, 3)
    return (q, r) if len(q) <= len(r) else (r, q)                   # equal lengths: the query is the short list


def sd_table(q, r, dt=np.float32):
    """The reference's table, cell by cell: SD[M-1][j] = d(M-1, j); SD[i][j] = min(d(i, j) + SD[i+1][j+1], SD[i][j+1]) for j <= N - M + i, the cell right of
    the boundary diagonal reading +inf, so the diagonal is built by the same addition.  -> (min_j SD[0][j <= N - M], M); (-1, 0) if either list is empty."""
    s, l = _short_long(q, r)
    M, N = len(s), len(l)
    if M == 0:
        return dt(-1), 0
    SD = np.full((M, N + 1), np.inf, dtype=dt)
    for j in range(N):
        SD[M - 1, j] = _d(s[M - 1], l[j], dt)
    for i in range(M - 2, -1, -1):
        for j in range(N - M + i, -1, -1):
            SD[i, j] = min(dt(_d(s[i], l[j], dt) + SD[i + 1, j + 1]), SD[i, j + 1])
    return SD[0, :N - M + 1].min(), M


def sd_pair(q, r, dt=np.float32):
    """sd_table on the band T_i[k] = SD[i][i + k], k <= N - M, a row at a time: an addition and a running minimum from the right."""
    s, l = _short_long(q, r)
    M, N = len(s), len(l)
    if M == 0:
        return dt(-1), 0
    W = N - M + 1
    T = _d(s[M - 1][None], l[M - 1:M - 1 + W], dt).astype(dt)
    for i in range(M - 2, -1, -1):
        u = (_d(s[i][None], l[i:i + W], dt).astype(dt) + T).astype(dt)
        T = np.minimum.accumulate(u[::-1])[::-1]
    return T.min(), M


def sd_brute(q, r, adjacent_last, dt=np.float64):
    """The minimum over the order-preserving placements of the short list in the long one of the sum of d -- all of them, or (adjacent_last) those in which
    the last two residues of the short list are neighbours in the long one."""
    s, l = _short_long(q, r)
    M, N = len(s), len(l)
    best = np.inf
    for place in itertools.combinations(range(N), M):
        if adjacent_last and M >= 2 and place[-1] != place[-2] + 1:
            continue
        best = min(best, sum(float(_d(s[i], l[j], dt)) for i, j in enumerate(place)))
    return best


def sd_rows(qca, qmask, rca, rmask, dt=np.float32):
    """Q rows against R rows like the entry point -> sd (Q, R) dt, m (Q, R) int32"""
    pick = lambda rows, mask: [np.asarray(row, dtype=np.float32) if mask is None else np.asarray(row, dtype=np.float32)[np.asarray(mask[k]).astype(bool)]
                               for k, row in enumerate(np.asarray(rows))]
    qs, rs = pick(qca, qmask), pick(rca, rmask)
    sd, m = np.zeros((len(qs), len(rs)), dtype=dt), np.zeros((len(qs), len(rs)), dtype=np.int32)
    for x, a in enumerate(qs):
        for y, b in enumerate(rs):
            sd[x, y], m[x, y] = sd_pair(a, b, dt)
    return sd, m
