"""The definition of include/abopt.h for abopt_align_traceback and abopt_superposed_rmsd_mapped, restated in numpy (used by
tests/test_alignment_trace.py and tools/bench_alignment.py); importable without a device.

THE alignment of a and b: among the words over P (a pair), A (a residue of a against a gap), B (a gap against a residue of b) that spell both sequences and
attain the lexicographic maximum of (score, matches, -columns) -- priced as abopt_align_sequences prices them -- the word that is lexicographically least when
read from its LAST column to its first, with P < A < B.

`trace_brute` is that sentence: every word enumerated and priced by `price_word`, the optimal ones kept, the reverse-lexicographic least taken.  `trace_walk`
computes the same word from the three Gotoh tables by a backward walk that keeps a SET of states; `greedy_walk_word` is the single-state walk with a fixed
preference, which is wrong on ties (GREEDY_FAILS keeps the cases).  `trace_rows` lays the result out as the entry point does; `mapped_rows` is the float64
statement of the mapped superposition on the pairs of a map."""
import itertools

import numpy as np

import superpose_statement as sp

P, A, B = 1, 2, 3                       # the codes of `ops`; 0 pads a row beyond `columns`
LETTER = {P: 'P', A: 'A', B: 'B'}
NEG = -(1 << 60)
_S, _M = 1 << 32, 1 << 16              # the kernel's carrier: score 2^32 + matches 2^16 - columns


def _sub(table, x, y):
    T = table.shape[0]
    return int(table[min(int(x), T - 1), min(int(y), T - 1)])


def _decode(v):
    v = int(v)
    c = (-v) & 0xffff
    v += c
    return v >> 32, (v >> 16) & 0xffff, c


# ------------------------------------------------------------------------------------------ the definition, word by word
def price_word(word, a, b, table, gap_open, gap_extend):
    """(score, matches, -columns) of one word (a sequence of P, A, B codes): a maximal run of A or of B that touches the first or the last column is free, any
    other run of k columns costs gap_open + (k - 1) gap_extend; a pair scores table[a_i][b_j] and is a match iff the raw bytes are equal."""
    score = matches = ia = ib = 0
    runs = [(k, len(list(g))) for k, g in itertools.groupby(word)]
    for r, (k, cnt) in enumerate(runs):
        if k == P:
            for _ in range(cnt):
                score += _sub(table, a[ia], b[ib])
                matches += int(a[ia] == b[ib])
                ia += 1
                ib += 1
        else:
            if r != 0 and r != len(runs) - 1:
                score += gap_open + (cnt - 1) * gap_extend
            if k == A:
                ia += cnt
            else:
                ib += cnt
    assert ia == len(a) and ib == len(b)
    return score, matches, -len(word)


def all_words(n, m):
    """every word that spells n residues of a and m of b, as tuples of codes"""
    out = []

    def walk(i, j, word):
        if i == n and j == m:
            out.append(word)
            return
        if i < n and j < m:
            walk(i + 1, j + 1, word + (P,))
        if i < n:
            walk(i + 1, j, word + (A,))
        if j < m:
            walk(i, j + 1, word + (B,))

    walk(0, 0, ())
    return out


def trace_brute(a, b, table, gap_open, gap_extend):
    """-> (score, matches, columns, word, how many words are optimal): the definition by enumeration; tiny sequences only."""
    table = np.asarray(table)
    priced = [(price_word(w, a, b, table, gap_open, gap_extend), w) for w in all_words(len(a), len(b))]
    best = max(p for p, _ in priced)
    optimal = [w for p, w in priced if p == best]
    word = min(optimal, key=lambda w: w[::-1])
    return best[0], best[1], -best[2], word, len(optimal)


# ------------------------------------------------------------------------------------------ the tables
def gotoh_tables(a, b, table, gap_open, gap_extend):
    """H, X, Y (n + 1, m + 1) int64 in the carrier and the pair term E (E[i][j]: a_i against b_j), a row at a time as similarity_statement.align_pair does
    (Y as a running maximum, exact because gap_open <= gap_extend).  Row 0 and column 0 of H are the free leading runs; X and Y read NEG there."""
    a, b, table = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(table, dtype=np.int64)
    n, m = len(a), len(b)
    assert n >= 1 and m >= 1 and gap_open <= gap_extend <= 0
    T = table.shape[0]
    bi = np.minimum(b, T - 1)
    d_open, d_ext = gap_open * _S - 1, gap_extend * _S - 1
    j = np.arange(m + 1, dtype=np.int64)
    H = np.zeros((n + 1, m + 1), dtype=np.int64)
    X = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    Y = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    E = np.zeros((n + 1, m + 1), dtype=np.int64)
    H[0] = -j
    for i in range(1, n + 1):
        E[i, 1:] = table[min(int(a[i - 1]), T - 1), bi] * _S + (a[i - 1] == b) * _M - 1
        X[i, 1:] = np.maximum(H[i - 1, 1:] + d_open, X[i - 1, 1:] + d_ext)
        G = np.empty(m + 1, dtype=np.int64)
        G[0] = -i
        G[1:] = np.maximum(H[i - 1, :-1] + E[i, 1:], X[i, 1:])
        Z = np.maximum.accumulate(G - j * d_ext)
        Y[i, 1:] = Z[:-1] + d_open + j[:-1] * d_ext
        H[i, 0] = -i
        H[i, 1:] = np.maximum(G[1:], Y[i, 1:])
    return H, X, Y, E, d_open, d_ext


def _optimum(H, n, m):
    col = H[:, m] - (n - np.arange(n + 1))                          # a free trailing run of A behind (i, m)
    row = H[n, :] - (m - np.arange(m + 1))                          # a free trailing run of B behind (n, j)
    best = max(int(col.max()), int(row.max()))
    return best, col == best, row == best


# ------------------------------------------------------------------------------------------ the walk
def trace_walk(a, b, table, gap_open, gap_extend):
    """-> (score, matches, columns, word): the alignment by the backward walk over sets of states.  After a suffix of the word is fixed the cell (i, j) is fixed;
    the set holds the states there from which the suffix completes an optimal word: 'H' (any ending), 'X' (ends with an A), 'Y' (ends with a B), 'TA' / 'TB'
    (inside the free trailing run of A / of B, which goes on).  A step closes the set under the ties X = H and Y = H, emits the least letter any state can
    emit over a tight edge, and moves to the tight predecessors for that letter."""
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return 0, 0, max(n, m), (A,) * n + (B,) * m
    H, X, Y, E, d_open, d_ext = gotoh_tables(a, b, table, gap_open, gap_extend)
    best, qa, qb = _optimum(H, n, m)
    first = lambda q, stop: next((k for k in range(stop) if q[k]), stop)
    mina, minb = first(qa, n), first(qb, m)                        # the first row (column) a trailing run may start behind
    i, j = n, m
    S = set()
    if qa[n]:
        S.add('H')
    if mina < n:
        S.add('TA')
    if minb < m:
        S.add('TB')
    word = []
    for _ in range(n + m):                                           # bounded: a letter consumes a residue
        if i == 0 and j == 0:
            break
        if 'H' in S and i >= 1 and j >= 1:
            if X[i, j] == H[i, j]:
                S.add('X')
            if Y[i, j] == H[i, j]:
                S.add('Y')
        opts = {P: set(), A: set(), B: set()}
        if 'H' in S:
            if i >= 1 and j >= 1:
                if H[i - 1, j - 1] + E[i, j] == H[i, j]:
                    opts[P].add('H')
            elif i >= 1:
                opts[A].add('H')                                     # column 0: the free leading run of A
            else:
                opts[B].add('H')                                     # row 0: the free leading run of B
        if 'X' in S:
            if H[i - 1, j] + d_open == X[i, j]:
                opts[A].add('H')
            if X[i - 1, j] + d_ext == X[i, j]:
                opts[A].add('X')
        if 'Y' in S:
            if H[i, j - 1] + d_open == Y[i, j]:
                opts[B].add('H')
            if Y[i, j - 1] + d_ext == Y[i, j]:
                opts[B].add('Y')
        if 'TA' in S:
            if qa[i - 1]:
                opts[A].add('H')
            if mina < i - 1:
                opts[A].add('TA')
        if 'TB' in S:
            if qb[j - 1]:
                opts[B].add('H')
            if minb < j - 1:
                opts[B].add('TB')
        letter = next(k for k in (P, A, B) if opts[k])
        word.append(letter)
        S = opts[letter]
        i -= letter != B
        j -= letter != A
    assert i == 0 and j == 0
    s, k, c = _decode(best)
    assert c == len(word)
    return s, k, c, tuple(word[::-1])


def greedy_walk_word(a, b, table, gap_open, gap_extend, x_first='H'):
    """The single-state walk: one state, a fixed preference (P, then A, then B; from a gap state with both edges tight, the predecessor `x_first`).  It follows
    tight edges only, so its word is optimal -- but not always THE alignment."""
    n, m = len(a), len(b)
    H, X, Y, E, d_open, d_ext = gotoh_tables(a, b, table, gap_open, gap_extend)
    best, qa, qb = _optimum(H, n, m)
    i, j, word = n, m, []
    if qa[n]:
        state = 'H'
    elif qa[:n].any():
        k = max(k for k in range(n) if qa[k])
        word, i, state = [A] * (n - k), k, 'H'
    else:
        k = max(k for k in range(m) if qb[k])
        word, j, state = [B] * (m - k), k, 'H'
    while i > 0 or j > 0:
        if state == 'H':
            if i == 0:
                word.append(B); j -= 1
            elif j == 0:
                word.append(A); i -= 1
            elif H[i - 1, j - 1] + E[i, j] == H[i, j]:
                word.append(P); i -= 1; j -= 1
            else:
                state = 'X' if X[i, j] == H[i, j] else 'Y'
        elif state == 'X':
            open_, ext = H[i - 1, j] + d_open == X[i, j], X[i - 1, j] + d_ext == X[i, j]
            state = 'H' if (open_ and (x_first == 'H' or not ext)) else 'X'
            word.append(A); i -= 1
        else:
            open_, ext = H[i, j - 1] + d_open == Y[i, j], Y[i, j - 1] + d_ext == Y[i, j]
            state = 'H' if (open_ and (x_first == 'H' or not ext)) else 'Y'
            word.append(B); j -= 1
    return tuple(word[::-1])


# (a, b, table, gap_open, gap_extend, x_first): the single-state walk with that preference gives another optimal word than the definition.  Found by a search
# over random tiny pairs and kept, one per preference; the test re-derives both words.  In the first, from X with both edges tight the H route next offers
# only B while the X route offers A.
GREEDY_FAILS = [((0, 0, 1, 1, 1), (0, 1, 0), ((2, -2), (-2, 2)), -1, 0, 'H'),
                ((1, 0, 1, 0), (0, 1), ((-2, -2), (2, -1)), -1, 0, 'H'),
                ((1, 1, 0, 0), (1, 0), ((1, 0), (0, 1)), 0, 0, 'X')]


# ------------------------------------------------------------------------------------------ the entry point's layout
def maps_of(word, ka, kb, na, nb):
    """ops row (na + nb) uint8, qmap (na) and rmap (nb) int16 of a word; ka / kb: the element index of every residue of a / b (the mask-true elements)."""
    ops = np.zeros(na + nb, dtype=np.uint8)
    ops[:len(word)] = word
    qmap, rmap = np.full(na, -1, dtype=np.int16), np.full(nb, -1, dtype=np.int16)
    i = j = 0
    for w in word:
        if w == P:
            qmap[ka[i]], rmap[kb[j]] = kb[j], ka[i]
        i += w != B
        j += w != A
    return ops, qmap, rmap


def trace_rows(q, qmask, r, rmask, table, gap_open, gap_extend, pairs=None):
    """Like the entry point: q (Q, na), r (R, nb) bytes, masks bool or None, pairs (P, 2) or None (all Q R, row-major).  -> dict of score, matches, columns (P)
    int32, ops (P, na + nb) uint8, qmap (P, na), rmap (P, nb) int16.  A pair outside the panels: 0, 0, 0, ops 0, maps -1.  Equal sequences are traced once."""
    q, r = np.asarray(q), np.asarray(r)
    (Q, na), (R, nb) = q.shape, r.shape
    if pairs is None:
        pairs = np.stack(np.meshgrid(np.arange(Q), np.arange(R), indexing='ij'), -1).reshape(-1, 2)
    pairs = np.asarray(pairs).reshape(-1, 2)
    n = len(pairs)
    out = dict(score=np.zeros(n, np.int32), matches=np.zeros(n, np.int32), columns=np.zeros(n, np.int32), ops=np.zeros((n, na + nb), np.uint8),
               qmap=np.full((n, na), -1, np.int16), rmap=np.full((n, nb), -1, np.int16))
    idx = lambda mask, row, width: np.arange(width) if mask is None else np.nonzero(np.asarray(mask[row]).astype(bool))[0]
    memo = {}
    for p, (x, y) in enumerate(pairs):
        if not (0 <= x < Q and 0 <= y < R):
            continue
        ka, kb = idx(qmask, x, na), idx(rmask, y, nb)
        a, b = tuple(int(v) for v in q[x][ka]), tuple(int(v) for v in r[y][kb])
        if (a, b) not in memo:
            memo[a, b] = trace_walk(a, b, table, gap_open, gap_extend)
        s, k, c, word = memo[a, b]
        out['score'][p], out['matches'][p], out['columns'][p] = s, k, c
        out['ops'][p], out['qmap'][p], out['rmap'][p] = maps_of(word, ka, kb, na, nb)
    return out


def alignment_strings_of(word, a, b, letters):
    """the two gapped strings of a word over the sequences a and b"""
    sa, sb, i, j = [], [], 0, 0
    for w in word:
        sa.append(letters[a[i]] if w != B else '-')
        sb.append(letters[b[j]] if w != A else '-')
        i += w != B
        j += w != A
    return ''.join(sa), ''.join(sb)


# ------------------------------------------------------------------------------------------ the mapped superposition
def mapped_lists(qmap_row, nb, qfit, rfit, qscore, rscore):
    """The fit pairs and the score pairs of one map row: (k, j = qmap[k]) in ascending k with 0 <= j < nb and both masks true (None = all; a score mask that is
    None is that side's fit mask).  -> ((kf, jf), (ks, js)) index arrays."""
    qmap_row = np.asarray(qmap_row).astype(np.int64)
    na = len(qmap_row)
    on = lambda m, width: np.ones(width, bool) if m is None else np.asarray(m).astype(bool)
    qf, rf = on(qfit, na), on(rfit, nb)
    qs, rs = (qf if qscore is None else on(qscore, na)), (rf if rscore is None else on(rscore, nb))
    ok = (qmap_row >= 0) & (qmap_row < nb)
    j = np.where(ok, qmap_row, 0)
    fit = ok & qf & rf[j]
    score = ok & qs & rs[j]
    kf, ks = np.nonzero(fit)[0], np.nonzero(score)[0]
    return (kf, qmap_row[kf]), (ks, qmap_row[ks])


def mapped_pair(x, y, qmap_row, qfit=None, rfit=None, qscore=None, rscore=None, fit=sp.kabsch):
    """One query row x (na, 3) against one reference row y (nb, 3) under a map, float64 -> dict(rmsd, n_fit, n_score, rot, trans, gap) like
    superpose_statement.pair; not scored (fewer than 3 fit pairs, or no score pair): -1, 0, 0, the identity, 0."""
    (kf, jf), (ks, js) = mapped_lists(qmap_row, len(y), qfit, rfit, qscore, rscore)
    if len(kf) < 3 or len(ks) == 0:
        return dict(rmsd=-1.0, n_fit=0, n_score=0, rot=np.eye(3), trans=np.zeros(3), gap=np.inf)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    R, t = fit(x[kf], y[jf])
    return dict(rmsd=sp.rmsd_under(R, t, x[ks], y[js]), n_fit=len(kf), n_score=len(ks), rot=R, trans=t, gap=sp.key_matrix_gap(y[jf], x[kf]))


def mapped_rows(q, r, qmap, pairs=None, qfit=None, rfit=None, qscore=None, rscore=None):
    """Like the entry point -> dict of arrays over the P pairs: rmsd, gap float64, n_fit, n_score int32, rot (P, 3, 3), trans (P, 3)."""
    Q, R = len(q), len(r)
    if pairs is None:
        pairs = np.stack(np.meshgrid(np.arange(Q), np.arange(R), indexing='ij'), -1).reshape(-1, 2)
    pairs = np.asarray(pairs).reshape(-1, 2)
    n = len(pairs)
    out = dict(rmsd=np.full(n, -1.0), gap=np.full(n, np.inf), n_fit=np.zeros(n, np.int32), n_score=np.zeros(n, np.int32), rot=np.tile(np.eye(3), (n, 1, 1)),
               trans=np.zeros((n, 3)))
    row = lambda m, i: None if m is None else m[i]
    for p, (x, y) in enumerate(pairs):
        if not (0 <= x < Q and 0 <= y < R):
            continue
        for k, v in mapped_pair(q[x], r[y], qmap[p], row(qfit, x), row(rfit, y), row(qscore, x), row(rscore, y)).items():
            out[k][p] = v
    return out
