"""abopt_align_traceback and abopt_superposed_rmsd_mapped (csrc/align_trace.hip): the definition of THE alignment by enumeration against
the state-set walk of tests/alignment_trace_statement.py on the CPU; the device against the walk -- every output as integers -- and the mapped superposition
against abopt_superposed_rmsd on the gathered pairs, bit for bit, and against float64 on the GPU.

The float64 bound is the contract of DESIGN.md sections 6.7 and 6.12: |rmsd - rmsd64| <= 2^-23 rmsd64 + 1e-6 A, on inputs whose key-matrix eigen-gap exceeds
1e-3 (the rotation is well determined) with at least 3 fit pairs in every scored pair; the case builders assert both and walk seeds until they hold."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import alignment_trace_statement as at
import scorer_harness as harness
import screen_workers
import similarity_statement as st
import superpose_statement as sp
from ab_opt_amd import hip, model, sampler
from scorer_harness import DEV

P_, A_, B_ = at.P, at.A, at.B
REL, ABS = 2.0 ** -23, 1e-6
INT_FIELDS = ('score', 'matches', 'columns', 'ops', 'qmap', 'rmap')


# ------------------------------------------------------------------------------------------ CPU: the definition
def test_traceback_statement_equals_brute_force():
    """The state-set walk against the definition -- every word enumerated and priced, the optimal ones kept, the reverse-lexicographic least taken -- on 2400
    random pairs of length 0 .. 5 over two or three letters plus a byte >= T, gaps with open <= extend <= 0, 0 / 0 and open = extend among them.  More than a
    fifth of the pairs have more than one optimal word, so the test cannot pass on tie-free inputs."""
    rng = np.random.default_rng(31)
    gaps = [(0, 0), (-1, -1), (-2, -1), (-1, 0), (-3, -3), (-2, 0), (-4, -2)]
    several = 0
    N = 2400
    for _ in range(N):
        T = int(rng.integers(2, 4))
        a = tuple(int(v) for v in rng.integers(0, T + 1, rng.integers(0, 6)))
        b = tuple(int(v) for v in rng.integers(0, T + 1, rng.integers(0, 6)))
        table = np.eye(T, dtype=np.int32) if rng.random() < 0.5 else rng.integers(-2, 3, (T, T)).astype(np.int32)
        go, ge = gaps[int(rng.integers(len(gaps)))]
        s, k, c, word, optimal = at.trace_brute(a, b, table, go, ge)
        assert at.trace_walk(a, b, table, go, ge) == (s, k, c, word), (a, b, table, go, ge)
        if a and b:
            assert (s, k, c) == st.align_brute(a, b, table, go, ge)
        several += optimal > 1
    print(f'{several} of {N} pairs have more than one optimal word')
    assert 5 * several >= N


def test_walk_agrees_with_align_pair_on_long_sequences():
    """(score, matches, columns) of the walk equal align_pair's on lengths up to 256, and the word it returns has that price and spells both sequences."""
    rng = np.random.default_rng(32)
    for n, m, letters in ((256, 256, 21), (255, 64, 2), (3, 256, 4), (256, 1, 2), (65, 63, 3), (128, 129, 25)):
        a, b = rng.integers(0, letters, n), rng.integers(0, letters, m)
        table = rng.integers(-4, 6, (min(letters, 21), min(letters, 21))).astype(np.int32)
        for go, ge in ((-3, -1), (0, 0), (-2, -2)):
            s, k, c, word = at.trace_walk(a, b, table, go, ge)
            assert (s, k, c) == st.align_pair(a, b, table, go, ge), (n, m, letters, go, ge)
            assert at.price_word(word, a, b, table, go, ge) == (s, k, -c)


def test_a_single_state_walk_is_not_the_definition():
    """Why the walk keeps a set: on the kept cases the greedy walk (P, then A, then B; a fixed predecessor from a gap state with both edges tight) returns an
    optimal word that is NOT the reverse-lexicographic least one, for either preference."""
    assert {f[5] for f in at.GREEDY_FAILS} == {'H', 'X'}
    for a, b, table, go, ge, first in at.GREEDY_FAILS:
        table = np.array(table, dtype=np.int32)
        s, k, c, word, optimal = at.trace_brute(a, b, table, go, ge)
        greedy = at.greedy_walk_word(a, b, table, go, ge, first)
        assert optimal > 1 and at.price_word(greedy, a, b, table, go, ge) == (s, k, -c), (a, b)
        assert greedy != word and greedy[::-1] > word[::-1] and at.trace_walk(a, b, table, go, ge)[3] == word, (a, b, greedy, word)


HAND = [0, 7, 3, 3, 12, 19, 5, 9, 9, 1, 15, 2, 8, 4, 16, 17, 6, 11, 13, 10, 18, 14, 0, 3]


def _hand_cases():
    """(name, a, b, gap_open, gap_extend, the word) on model.identity_table()"""
    a, n = HAND, len(HAND)
    other = 6                                                        # a residue unlike its neighbours wherever it is inserted below
    return [('identical', a, a, -20, -1, (P_,) * n),
            ('inserted in the middle', a, a[:12] + [other] + a[12:], -20, -1, (P_,) * 12 + (B_,) + (P_,) * 12),
            ('inserted at the start', a, [other] + a, -20, -1, (B_,) + (P_,) * n),
            ('inserted at the end', a, a + [other], -20, -1, (P_,) * n + (B_,)),
            ('deleted in the middle', a, a[:12] + a[13:], -20, -1, (P_,) * 12 + (A_,) + (P_,) * 11),
            ('nothing worth pairing', [0, 1], [2, 3, 4], -20, -1, (B_,) * 3 + (A_,) * 2),
            ('an empty query', [], a[:5], -20, -1, (B_,) * 5),
            ('an empty reference', a[:5], [], -20, -1, (A_,) * 5),
            ('both empty', [], [], -20, -1, ()),
            # an A-run next to a B-run: with gaps that cost nothing a's middle residue and b's two middle residues pair with nothing (a mismatch is -2); the
            # three orders of the runs are co-optimal, and read from the last column the A comes first
            ('an A-run next to a B-run', [0, 1, 5, 2, 3], [0, 1, 6, 7, 2, 3], 0, 0, (P_, P_, B_, B_, A_, P_, P_))]


def test_hand_cases_and_alignment_strings():
    t = model.identity_table().numpy()
    for name, a, b, go, ge, word in _hand_cases():
        s, k, c, got = at.trace_walk(a, b, t, go, ge)
        assert got == word, (name, got)
        if len(a) <= 6 and len(b) <= 6:
            assert at.trace_brute(a, b, t, go, ge)[:4] == (s, k, c, word), name
        na, nb = max(len(a), 1), max(len(b), 1)
        ops, qmap, rmap = at.maps_of(word, np.arange(len(a)), np.arange(len(b)), na, nb)
        qrow, rrow = np.array(list(a) + [0] * (na - len(a))), np.array(list(b) + [0] * (nb - len(b)))
        qm, rm = np.arange(na) < len(a), np.arange(nb) < len(b)
        sa, sb = model.alignment_strings(torch.from_numpy(ops), torch.from_numpy(qrow), torch.from_numpy(rrow), torch.from_numpy(qm), torch.from_numpy(rm))
        assert (sa, sb) == at.alignment_strings_of(word, a, b, model.AA_LETTERS) and len(sa) == len(sb) == c, name
        assert sa.replace('-', '') == ''.join(model.AA_LETTERS[v] for v in a) and sb.replace('-', '') == ''.join(model.AA_LETTERS[v] for v in b), name
    ops = at.maps_of((P_, B_, P_), np.arange(2), np.arange(3), 2, 3)[0]
    assert model.alignment_strings(ops, [0, 1], [0, 25, 1]) == ('A-C', 'AXC')                    # a type outside AA_LETTERS prints X
    with pytest.raises(ValueError, match='does not spell'):
        model.alignment_strings(ops, [0, 1, 2], [0, 25, 1])
    with pytest.raises(ValueError, match='a mask of'):
        model.alignment_strings(ops, [0, 1], [0, 25, 1], qmask=[True])


def _consistent(out, q, qmask, r, rmask, pairs, table=None):
    """ops spells both sequences; qmap and rmap are mutually inverse and strictly increasing along the pairs; the 1s of ops are the pairs of the maps, its
    matching 1s are `matches` and its nonzero entries `columns`."""
    Q, R = len(q), len(r)
    for p, (x, y) in enumerate(pairs):
        ops, qmap, rmap = out['ops'][p], out['qmap'][p].astype(int), out['rmap'][p].astype(int)
        if not (0 <= x < Q and 0 <= y < R):
            assert not ops.any() and (qmap == -1).all() and (rmap == -1).all() and out['columns'][p] == out['score'][p] == out['matches'][p] == 0
            continue
        ka = np.arange(q.shape[1]) if qmask is None else np.nonzero(qmask[x])[0]
        kb = np.arange(r.shape[1]) if rmask is None else np.nonzero(rmask[y])[0]
        c = int(out['columns'][p])
        word = ops[:c]
        assert c == np.count_nonzero(ops) and (word > 0).all() and (word != B_).sum() == len(ka) and (word != A_).sum() == len(kb), p
        i = np.cumsum(word != B_) - 1
        j = np.cumsum(word != A_) - 1
        pk, pj = ka[i[word == P_]], kb[j[word == P_]]               # the paired elements, by spelling the word
        paired = np.nonzero(qmap >= 0)[0]
        assert np.array_equal(paired, pk) and np.array_equal(qmap[paired], pj) and (np.diff(pj) > 0).all(), p
        back = np.nonzero(rmap >= 0)[0]
        assert np.array_equal(back, pj) and np.array_equal(rmap[back], pk), p
        assert int(out['matches'][p]) == int((q[x][pk] == r[y][pj]).sum()), p


def test_statement_outputs_are_consistent():
    c = trace_case('ties-no-gap-cost')
    _consistent(c['want'], c['q'], c['qmask'], c['r'], c['rmask'], c['all_pairs'])
    c = trace_case('listed-flat-gaps')
    _consistent(c['want'], c['q'], c['qmask'], c['r'], c['rmask'], c['pairs'])
    assert ((c['pairs'] < 0) | (c['pairs'] >= [len(c['q']), len(c['r'])])).any(1).sum() >= 2        # pairs outside the panels are among them


def test_bad_arguments_are_refused_before_any_launch():
    """Every ValueError of the two wrappers and of sampler.aligned_rmsd on CPU tensors, and the return codes of the two C entries on dummy pointers that are
    never dereferenced -- ABOPT_EUNSUPPORTED for a row of 257 among them."""
    q, r, t = torch.zeros(3, 9, dtype=torch.uint8), torch.zeros(2, 12, dtype=torch.int64), model.identity_table()
    tb = hip.align_traceback
    with pytest.raises(ValueError, match=r'q .* must be integer \(rows, n\)'):
        tb(q.float(), r, t, -2, -1)
    with pytest.raises(ValueError, match='r has 257 elements per row, expected 1 .. 256'):
        tb(q, torch.zeros(2, 257, dtype=torch.uint8), t, -2, -1)
    with pytest.raises(ValueError, match=r'mask of q .* must be \(rows, n\)'):
        tb(q, r, t, -2, -1, qmask=torch.ones(3, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match=r'table .* must be integer of shape \(T, T\)'):
        tb(q, r, t.float(), -2, -1)
    with pytest.raises(ValueError, match='gap_open <= gap_extend <= 0'):
        tb(q, r, t, -1, -2)
    with pytest.raises(ValueError, match='must be an integer'):
        tb(q, r, t, -1.5, -1)
    for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 2), torch.zeros(4, 2, dtype=torch.bool)):
        with pytest.raises(ValueError, match=r'pairs .* must be integer of shape \(P, 2\)'):
            tb(q, r, t, -2, -1, pairs=bad)
    with pytest.raises(ValueError, match='HIP device only'):
        tb(q, r, t, -2, -1, pairs=torch.zeros(4, 2, dtype=torch.int64))
    x, y, qmap = torch.zeros(3, 9, 3), torch.zeros(2, 12, 3, dtype=torch.float64), torch.zeros(6, 9, dtype=torch.int16)
    sm = hip.superposed_rmsd_mapped
    with pytest.raises(ValueError, match=r'q .* must be floating point \(rows, n, 3\)'):
        sm(x[:, :, :2], y, qmap)
    with pytest.raises(ValueError, match='r has 300 elements per row'):
        sm(x, torch.zeros(2, 300, 3), qmap)
    with pytest.raises(ValueError, match=r'mask of r .* must be'):
        sm(x, y, qmap, rfit=torch.ones(2, 9, dtype=torch.bool))
    with pytest.raises(ValueError, match=r'qscore .* must be \(rows, n\)'):
        sm(x, y, qmap, qscore=torch.ones(3, 8, dtype=torch.bool))
    for bad in (qmap[:5], qmap[:, :8], qmap.float(), qmap[0]):
        with pytest.raises(ValueError, match=r'qmap .* must be integer of shape \(P, na\)'):
            sm(x, y, bad)
    with pytest.raises(ValueError, match=r'qmap .* must be integer of shape \(P, na\) = \(4, 9\)'):
        sm(x, y, qmap, pairs=torch.zeros(4, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match=r'pairs .* must be integer of shape \(P, 2\)'):
        sm(x, y, qmap, pairs=torch.zeros(6, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match='HIP device only'):
        sm(x, y, qmap)
    batch = dict(aa=torch.zeros(1, 9, dtype=torch.long), generate_flag=torch.zeros(1, 9, dtype=torch.bool), fragment_type=torch.ones(1, 9, dtype=torch.long))
    pos, mask = torch.zeros(1, 9, 4, 3), torch.ones(1, 9, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match='rows must be'):
        sampler.aligned_rmsd(batch, q[:1], pos, mask, rows='designed')
    with pytest.raises(ValueError, match=r'expected seqs \(G\*S, L\)'):
        sampler.aligned_rmsd(batch, q[:1], pos[:, :, :1], mask[:, :, :1])
    with pytest.raises(ValueError, match='need both ref_seqs'):
        sampler.aligned_rmsd(batch, q[:1], pos, mask, ref_seqs=q)
    with pytest.raises(ValueError, match='ref_mask selects'):
        sampler.aligned_rmsd(batch, q[:1], pos, mask, ref_mask=torch.ones(1, 9, dtype=torch.bool))
    with pytest.raises(ValueError, match=r'expected ref_seqs \(R, nb\) and ref_ca \(R, nb, 3\)'):
        sampler.aligned_rmsd(batch, q[:1], pos, mask, ref_seqs=q, ref_ca=torch.zeros(3, 8, 3))

    L_ = hip.lib()
    dummy = (ctypes.c_char * 16)()
    a = ctypes.c_void_p(ctypes.addressof(dummy))

    def trace(Q=3, R=2, na=9, nb=12, T=21, go=-2, ge=-1, q=a, table=a, columns=a, pairs=None, P=0):
        return L_.abopt_align_traceback(q, None, a, None, table, T, go, ge, pairs, P, Q, R, na, nb, a, a, columns, None, None, None, None)

    def mapped(Q=3, R=2, na=9, nb=12, q=a, qmap=a, n_score=a, pairs=None, P=0):
        return L_.abopt_superposed_rmsd_mapped(q, a, qmap, pairs, P, None, None, None, None, Q, R, na, nb, a, a, n_score, None, None, None)
    for fn in (trace, mapped):
        for kw, rc, word in ((dict(na=257), 3, '256'), (dict(nb=257), 3, '256'), (dict(na=0), 1, 'bad dims'), (dict(Q=-1), 1, 'bad dims'),
                             (dict(Q=65536, R=65536), 1, 'bad dims'), (dict(Q=0, na=257), 3, '256'), (dict(pairs=a, P=-1), 1, 'bad dims')):
            assert fn(**kw) == rc and word in L_.abopt_last_error().decode(), (fn.__name__, kw, L_.abopt_last_error().decode())
        assert fn(Q=0) == 0 and fn(R=0, q=None) == 0 and fn(pairs=a, P=0) == 0 and fn(pairs=a, P=0, q=None) == 0       # the no-ops, ahead of the pointer checks
    for kw, word in ((dict(T=0), 'T=0'), (dict(T=33), 'T=33'), (dict(go=1, ge=1), 'gap_open'), (dict(go=-1, ge=-2), 'gap_open'), (dict(q=None), 'NULL'),
                     (dict(table=None), 'NULL'), (dict(columns=None), 'NULL'), (dict(pairs=a, P=4, q=None), 'NULL')):
        assert trace(**kw) == 1 and word in L_.abopt_last_error().decode(), (kw, L_.abopt_last_error().decode())
    for kw in (dict(q=None), dict(qmap=None), dict(n_score=None), dict(pairs=a, P=4, q=None)):
        assert mapped(**kw) == 1 and 'NULL' in L_.abopt_last_error().decode(), kw
    assert trace(Q=0, T=0) == 1                                      # the value checks precede the no-op


def test_binding_and_header_agree_on_the_new_entries():
    from test_abi import parse_header, signature_mismatches
    protos = parse_header()[0]
    assert {'abopt_align_traceback', 'abopt_superposed_rmsd_mapped'} <= set(protos) and set(hip.EXPORTS) == set(protos)
    assert signature_mismatches(hip._SIGNATURES, protos) == {}
    assert hip.ABI_VERSION == 59 and hip.lib().abopt_abi_version() == 59
    assert len(protos['abopt_align_traceback'][1]) == 21 and len(protos['abopt_superposed_rmsd_mapped'][1]) == 19


# ------------------------------------------------------------------------------------------ the traceback cases
LENS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256]         # a lane's four columns, the 64-lane ballot of compact_ranks, the row's end; 0 = an all-false row
# tag -> (rows: (query lengths, reference lengths) on rows of 256 with masks that are no prefixes, or (na, nb) = NULL masks; letters; table; gap_open;
#         gap_extend; pairs listed)
TRACE_CASES = {'ties-no-gap-cost': ((LENS, LENS[::-1]), 2, 'identity2', 0, 0, False),
               'listed-flat-gaps': ((LENS[1:] + [2], LENS), 2, 'identity2', -1, -1, True),
               'bytes-past-T': (([1, 5, 64, 65, 256, 200], [3, 4, 63, 255, 256, 0, 130]), 25, 'asymmetric21', -11, -1, False),
               'null-masks-wide-r': ((65, 256), 21, 'asymmetric21', -4, -2, True),
               'null-masks-wide-q': ((256, 63), 2, 'identity2', -1, 0, False),
               'null-masks-narrow': ((5, 3), 3, 'asymmetric3', -2, -1, False)}


def _masks(rng, lengths, width):
    m = np.zeros((len(lengths), width), dtype=bool)
    for k, n in enumerate(lengths):
        m[k, rng.choice(width, n, replace=False)] = True
        if 0 < n < width and m[k, :n].all():
            m[k, n - 1], m[k, width - 1] = False, True
    return m


@functools.lru_cache(maxsize=None)
def trace_case(tag):
    """the inputs of a case and what the statement gives on them, computed once"""
    rows, letters, tab, go, ge, listed = TRACE_CASES[tag]
    rng = np.random.default_rng(sum(map(ord, tag)))
    if isinstance(rows[0], int):
        na, nb, Q, R = rows[0], rows[1], 3, 2
        qmask = rmask = None
    else:
        na = nb = 256
        Q, R = len(rows[0]), len(rows[1])
        qmask, rmask = _masks(rng, rows[0], na), _masks(rng, rows[1], nb)
    table = {'identity2': np.array([[1, 0], [0, 1]]), 'asymmetric21': rng.integers(-6, 9, (21, 21)), 'asymmetric3': rng.integers(-3, 4, (3, 3))}[tab].astype(np.int32)
    c = dict(tag=tag, q=rng.integers(0, letters, (Q, na)).astype(np.uint8), r=rng.integers(0, letters, (R, nb)).astype(np.uint8), qmask=qmask, rmask=rmask,
             table=table, gap_open=go, gap_extend=ge)
    c['all_pairs'] = np.stack(np.meshgrid(np.arange(Q), np.arange(R), indexing='ij'), -1).reshape(-1, 2).astype(np.int32)
    c['pairs'] = None
    if listed:                                                       # scrambled, a pair repeated, pairs outside the panels on either side
        pairs = c['all_pairs'][rng.permutation(Q * R)][:max(Q * R * 2 // 3, 4)]
        c['pairs'] = np.concatenate([pairs[:3], [[Q, 0]], pairs, [[0, -1]], pairs[:1], [[-3, R + 7]]]).astype(np.int32)
    c['want'] = at.trace_rows(c['q'], qmask, c['r'], rmask, table, go, ge, c['pairs'])
    return c


def _dev(c, *names):
    return [None if c[n] is None else torch.from_numpy(np.ascontiguousarray(c[n])).to(DEV) for n in names]


def _trace(c, **kw):
    q, r, qmask, rmask, table, pairs = _dev(c, 'q', 'r', 'qmask', 'rmask', 'table', 'pairs')
    return hip.align_traceback(q, r, table, c['gap_open'], c['gap_extend'], qmask=qmask, rmask=rmask, pairs=pairs, want_rmap=True, **kw)


def test_case_statements_agree_with_align_rows():
    """On the CPU: the three integers of the traced cases are those of similarity_statement.align_rows, pair by pair."""
    for tag in ('ties-no-gap-cost', 'null-masks-narrow', 'null-masks-wide-q'):
        c = trace_case(tag)
        want = st.align_rows(c['q'], c['qmask'], c['r'], c['rmask'], c['table'], c['gap_open'], c['gap_extend'])
        for name, w in zip(('score', 'matches', 'columns'), want):
            assert np.array_equal(c['want'][name], w.reshape(-1)), (tag, name)


# ------------------------------------------------------------------------------------------ the mapped cases
@functools.lru_cache(maxsize=None)
def mapped_case():
    """Q = 5 designs and R = 4 references cut from one loop of 30 with deletions, insertions and substitutions, every row in a frame of its own, on rows of 40
    and 37 elements with masks that are no prefixes; fit and score masks on both sides.  The maps are the statement's.  Conditions (asserted; seeds are walked
    until they hold): every pair has at least 3 fit pairs and an eigen-gap above 1e-3, with and without the masks; at least one score set differs from its fit
    set on either side."""
    for seed in range(40, 60):
        rng = np.random.default_rng(seed)
        n0, Q, R, na, nb = 30, 5, 4, 40, 37
        base_seq, base_ca = rng.integers(0, 20, n0), sp._walk(rng, n0)

        def variant(width, drop, add):
            keep = np.sort(rng.choice(n0, n0 - drop, replace=False))
            seq, ca = list(base_seq[keep]), list(base_ca[keep] + rng.normal(size=(len(keep), 3)) * 0.4)
            for _ in range(add):
                k = int(rng.integers(1, len(seq)))
                seq.insert(k, int(rng.integers(0, 20)))
                ca.insert(k, (ca[k - 1] + ca[k]) / 2 + rng.normal(size=3))
            for k in rng.choice(len(seq), 2, replace=False):
                seq[k] = int(rng.integers(0, 20))
            rot, shift = sp.random_motion(rng, 40.0)
            mask = _masks(rng, [len(seq)], width)[0]
            row_seq, row_ca = rng.integers(0, 20, width), rng.normal(size=(width, 3)) * 30
            row_seq[mask], row_ca[mask] = seq, np.array(ca) @ rot.T + shift
            return row_seq.astype(np.uint8), row_ca.astype(np.float32), mask
        qs = [variant(na, int(rng.integers(0, 3)), int(rng.integers(0, 2))) for _ in range(Q)]
        rs = [variant(nb, int(rng.integers(0, 2)), int(rng.integers(0, 3))) for _ in range(R)]
        c = dict(q=np.stack([v[0] for v in qs]), qca=np.stack([v[1] for v in qs]), qmask=np.stack([v[2] for v in qs]), r=np.stack([v[0] for v in rs]),
                 rca=np.stack([v[1] for v in rs]), rmask=np.stack([v[2] for v in rs]), table=model.identity_table().numpy(), gap_open=-4, gap_extend=-1,
                 pairs=None, seeds_tried=seed - 40)
        c.update(qfit=rng.random((Q, na)) < 0.8, rfit=rng.random((R, nb)) < 0.85, qscore=rng.random((Q, na)) < 0.6, rscore=rng.random((R, nb)) < 0.7)
        c['want'] = at.trace_rows(c['q'], c['qmask'], c['r'], c['rmask'], c['table'], -4, -1)
        c['plain'] = at.mapped_rows(c['qca'], c['rca'], c['want']['qmap'])
        c['masked'] = at.mapped_rows(c['qca'], c['rca'], c['want']['qmap'], qfit=c['qfit'], rfit=c['rfit'], qscore=c['qscore'], rscore=c['rscore'])
        if all(w['n_fit'].min() >= 3 and w['gap'].min() > sp.GAP for w in (c['plain'], c['masked'])) and (c['masked']['n_fit'] != c['masked']['n_score']).any():
            return c
    raise AssertionError('no seed satisfies the conditions of mapped_case')


def test_mapped_case_conditions_hold_on_the_first_seed():
    """The conditions the float64 comparison rests on, checked here without a device: the first seed holds, every pair is scored with an eigen-gap above 1e-3 and
    at least 3 fit pairs, the lengths differ across pairs (so the rank entry alone could not score them), and the statement's RMSD after the fit is far below
    the unsuperposed deviation."""
    c = mapped_case()
    assert c['seeds_tried'] == 0
    for w in (c['plain'], c['masked']):
        assert w['n_fit'].min() >= 3 and w['gap'].min() > sp.GAP and (w['rmsd'] > 0).all() and w['rmsd'].max() < 3.0
    nq, nr = c['qmask'].sum(1), c['rmask'].sum(1)
    assert (nq[:, None] != nr[None]).sum() >= 10 and len(set(c['want']['columns'].tolist())) > 3
    assert (c['plain']['n_fit'] == (c['want']['qmap'] >= 0).sum(1)).all() and (c['plain']['n_fit'] < np.minimum(nq[:, None], nr[None]).reshape(-1) + 1).all()


def _gathered(c, p, masks):
    """pair p of the mapped case as two rows of equal count for the rank entry: the union of its fit and score pairs in ascending k, and which of them are
    fit / score pairs (None, None without masks)."""
    x, y = divmod(p, len(c['r']))
    m = {k: c[k][x if k[0] == 'q' else y] for k in ('qfit', 'rfit', 'qscore', 'rscore')} if masks else {}
    (kf, jf), (ks, js) = at.mapped_lists(c['want']['qmap'][p], c['rca'].shape[1], m.get('qfit'), m.get('rfit'), m.get('qscore'), m.get('rscore'))
    k = np.union1d(kf, ks)
    j = c['want']['qmap'][p][k].astype(int)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
    rows = t(c['qca'][x][k][None]), t(c['rca'][y][j][None])
    return rows + ((t(np.isin(k, kf)[None]), t(np.isin(k, ks)[None])) if masks else (None, None))


def _close(got, want64, tag):
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    err = np.abs(got - want64)
    print(f'{tag}: largest |rmsd - rmsd64| = {err.max():.3e} (bound at that pair {(REL * want64 + ABS)[err.argmax()]:.3e})')
    assert (err <= REL * want64 + ABS).all(), tag


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize('tag', list(TRACE_CASES))
def test_device_traceback_equals_the_statement(tag):
    """Every output equal as integers: lengths 0, 1, 3, 4, 5, 63, 64, 65, 255, 256 crossed with shorter and longer partners, masks that are no prefixes,
    all-false rows and NULL masks, two letters on an identity table with gaps 0 / 0 and -1 / -1 (tie-dense), 25 letters on a table of 21, asymmetric tables;
    pairs NULL, and a scrambled list with a repeated pair and pairs outside the panels.  score, matches and columns equal hip.align_sequences on the same
    rows, exactly."""
    c = trace_case(tag)
    got = _trace(c)
    for name in INT_FIELDS:
        g = got[name].cpu().numpy()
        assert g.dtype == c['want'][name].dtype and g.shape == c['want'][name].shape, (tag, name)
        assert np.array_equal(g, c['want'][name]), (tag, name, np.nonzero((g != c['want'][name]).reshape(len(g), -1).any(1))[0][:8])
    q, r, qmask, rmask, table = _dev(c, 'q', 'r', 'qmask', 'rmask', 'table')
    al = hip.align_sequences(q, r, table, c['gap_open'], c['gap_extend'], qmask=qmask, rmask=rmask)
    pairs = c['all_pairs'] if c['pairs'] is None else c['pairs']
    inside = ((pairs >= 0) & (pairs < [len(c['q']), len(c['r'])])).all(1)
    idx = torch.from_numpy(pairs[inside].astype(np.int64)).to(DEV)
    for name in ('score', 'matches', 'columns'):
        assert torch.equal(got[name][torch.from_numpy(inside).to(DEV)], al[name][idx[:, 0], idx[:, 1]]), (tag, name)
    lean = _trace(c, want_ops=False)                                 # the optional outputs left out: the others are the same
    assert 'ops' not in lean and all(torch.equal(lean[k], got[k]) for k in lean)


@pytest.mark.gpu
def test_mapped_superposition_equals_the_rank_entry_bit_for_bit():
    """The traced maps of the mapped case equal the statement's; then, pair by pair, rmsd, rot and trans of the mapped entry equal on their int32 views what
    hip.superposed_rmsd gives on the pairs gathered into rows of equal count -- with NULL masks, and with fit != score masks on both sides -- and the rmsd is
    within 2^-23 relative + 1e-6 A of the float64 Kabsch on the same pairs."""
    c = mapped_case()
    got = _trace(c)
    for name in INT_FIELDS:
        assert np.array_equal(got[name].cpu().numpy(), c['want'][name]), name
    qca, rca, qfit, rfit, qscore, rscore = _dev(c, 'qca', 'rca', 'qfit', 'rfit', 'qscore', 'rscore')
    bits = lambda t: t.reshape(-1).contiguous().view(torch.int32)
    for masks, want in ((False, c['plain']), (True, c['masked'])):
        kw = dict(qfit=qfit, rfit=rfit, qscore=qscore, rscore=rscore) if masks else {}
        out = hip.superposed_rmsd_mapped(qca, rca, got['qmap'], want_transform=True, **kw)
        assert np.array_equal(out['n_fit'].cpu().numpy(), want['n_fit']) and np.array_equal(out['n_score'].cpu().numpy(), want['n_score'])
        for p in range(len(want['rmsd'])):
            x, y, f, s = _gathered(c, p, masks)
            one = hip.superposed_rmsd(x, y, qfit=f, rfit=f, qscore=s, rscore=s, want_transform=True)
            assert int(one['n_fit']) == want['n_fit'][p] and int(one['n_score']) == want['n_score'][p]
            for name in ('rmsd', 'rot', 'trans'):
                assert torch.equal(bits(out[name][p]).reshape(-1), bits(one[name]).reshape(-1)), (masks, p, name)
        _close(out['rmsd'].cpu().numpy(), want['rmsd'], f'masks={masks}')


def _planted(seed):
    """A random-walk loop of 12 and a copy with one residue inserted behind residue 6, its sequence differing at the insertion only, moved by a random rotation
    and about 100 A -> (copy's types (1, 13), copy's CA, the loop's types (1, 12), the loop's CA)"""
    rng = np.random.default_rng(seed)
    seq = rng.permutation(20)[:13]                                   # 13 distinct types: the inserted one is unlike every residue of the loop
    ca = sp._walk(rng, 12)
    rot, _ = sp.random_motion(rng)
    shift = rng.normal(size=3)
    shift *= 100.0 / np.linalg.norm(shift)
    longer = np.concatenate([ca[:6], [(ca[5] + ca[6]) / 2 + [0.0, 3.0, 0.0]], ca[6:]])
    return (np.concatenate([seq[:6], seq[12:], seq[6:12]])[None].astype(np.uint8), (longer @ rot.T + shift)[None].astype(np.float32),
            seq[None, :12].astype(np.uint8), ca[None].astype(np.float32))


@pytest.mark.gpu
def test_a_planted_insertion_is_found_in_any_frame():
    """qmap skips exactly the inserted residue; the mapped RMSD is that of a zero deviation -- within the float64 contract of what the fp32 rounding of the moved
    coordinates leaves --, while hip.gapped_rmsd exceeds 1 A and hip.superposed_rmsd, whose counts differ, answers -1."""
    q, qca, r, rca = _planted(61)
    t = lambda v: torch.from_numpy(v).to(DEV)
    tb = hip.align_traceback(t(q), t(r), model.identity_table(), -4, -1, want_rmap=True)
    want = np.concatenate([np.arange(6), [-1], np.arange(6, 12)])
    assert tb['qmap'].cpu().numpy().tolist() == [want.tolist()] and tb['rmap'].cpu().numpy().tolist() == [[0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12]]
    assert tb['ops'][0, :13].tolist() == [1] * 6 + [2] + [1] * 6 and (tb['score'].item(), tb['matches'].item(), tb['columns'].item()) == (20, 12, 13)
    assert model.alignment_strings(tb['ops'][0].cpu(), q[0], r[0])[1].index('-') == 6
    out = hip.superposed_rmsd_mapped(t(qca), t(rca), tb['qmap'])
    zero = at.mapped_pair(qca[0], rca[0], want)['rmsd']              # float64 on the fp32 inputs: the rounding of coordinates near 100 A, about 1e-5 A
    print(f'planted insertion: rmsd {out["rmsd"].item():.3e}, float64 {zero:.3e}')
    assert zero < 1e-4 and out['n_fit'].item() == 12 and abs(out['rmsd'].item() - zero) <= REL * zero + ABS
    assert hip.gapped_rmsd(t(qca), t(rca))['rmsd'].item() > 1.0
    assert hip.superposed_rmsd(t(qca), t(rca))['rmsd'].item() == -1.0


@functools.lru_cache(maxsize=None)
def own_map_case():
    """A caller's own pairing: maps with entries outside [0, nb), not monotone, some reference elements named twice; masks on both sides; a listed pair outside
    the panels.  Seeds are walked until every scored pair has an eigen-gap above 1e-3; some pairs are not scored."""
    for seed in range(70, 90):
        rng = np.random.default_rng(seed)
        Q, R, na, nb = 4, 3, 23, 17
        pairs = np.concatenate([rng.integers(0, [Q, R], (14, 2)), [[Q, 1]], [[1, -1]]]).astype(np.int32)
        qmap = rng.integers(-6, nb + 6, (len(pairs), na)).astype(np.int16)
        qmap[3] = -1                                                 # no pair at all
        qmap[4, 2:] = nb                                             # two pairs at most
        qmap[5] = 32767
        c = dict(qca=(rng.normal(size=(Q, na, 3)) * 8).astype(np.float32), rca=(rng.normal(size=(R, nb, 3)) * 8).astype(np.float32), qmap=qmap, pairs=pairs,
                 qfit=rng.random((Q, na)) < 0.8, rfit=rng.random((R, nb)) < 0.8, qscore=rng.random((Q, na)) < 0.5, rscore=None, seeds_tried=seed - 70)
        c['want'] = at.mapped_rows(c['qca'], c['rca'], qmap, pairs, c['qfit'], c['rfit'], c['qscore'], None)
        scored = c['want']['n_fit'] > 0
        if scored.sum() >= 8 and (~scored).sum() >= 5 and c['want']['gap'][scored].min() > sp.GAP:
            return c
    raise AssertionError('no seed satisfies the conditions of own_map_case')


def test_own_map_case_conditions_hold():
    c = own_map_case()
    assert c['seeds_tried'] <= 3 and (np.diff(c['qmap'][0].astype(int)) < 0).any() and (c['qmap'] >= 17).any() and (c['qmap'] < -1).any()


@pytest.mark.gpu
def test_entries_outside_the_reference_row_are_never_pairs():
    """Out-of-range and non-monotone qmap entries: the counts equal the statement's exactly and the rmsd is within the float64 contract; pairs that are not
    scored read -1, 0, 0, the identity, 0; and the raw entry writes its P results and nothing behind them."""
    c = own_map_case()
    qca, rca, qmap, pairs, qfit, rfit, qscore = _dev(c, 'qca', 'rca', 'qmap', 'pairs', 'qfit', 'rfit', 'qscore')
    out = hip.superposed_rmsd_mapped(qca, rca, qmap, pairs=pairs, qfit=qfit, rfit=rfit, qscore=qscore, want_transform=True)
    want = c['want']
    assert np.array_equal(out['n_fit'].cpu().numpy(), want['n_fit']) and np.array_equal(out['n_score'].cpu().numpy(), want['n_score'])
    scored = want['n_fit'] > 0
    rmsd = out['rmsd'].cpu().numpy()
    _close(rmsd[scored], want['rmsd'][scored], 'own maps')
    off = torch.from_numpy(~scored).to(DEV)
    assert (rmsd[~scored] == -1).all() and bool((out['rot'][off] == torch.eye(3, device=DEV)).all()) and bool((out['trans'][off] == 0).all())
    P, pad = len(c['pairs']), 64
    f = {k: torch.full(((P + pad) * w,), 7.0, device=DEV) for k, w in (('rmsd', 1), ('rot', 9), ('trans', 3))}
    i = {k: torch.full((P + pad,), 7, dtype=torch.int32, device=DEV) for k in ('n_fit', 'n_score')}
    fl = lambda t: hip._as_flags(t)
    rc = hip.lib().abopt_superposed_rmsd_mapped(hip.ptr(qca), hip.ptr(rca), hip.ptr(qmap), hip.ptr(pairs), P, hip.ptr(fl(qfit)), hip.ptr(fl(qscore)),
                                                hip.ptr(fl(rfit)), None, 4, 3, 23, 17, hip.ptr(f['rmsd']), hip.ptr(i['n_fit']), hip.ptr(i['n_score']),
                                                hip.ptr(f['rot']), hip.ptr(f['trans']), hip.stream())
    torch.cuda.synchronize()
    assert rc == 0
    for k, w in (('rmsd', 1), ('rot', 9), ('trans', 3)):
        assert torch.equal(f[k][:P * w], out[k].reshape(-1)) and bool((f[k][P * w:] == 7).all()), k
    for k in i:
        assert torch.equal(i[k][:P], out[k]) and bool((i[k][P:] == 7).all()), k


def _small(seed, Q=5, R=7, na=9, nb=12):
    rng = np.random.default_rng(seed)
    t = lambda x: torch.from_numpy(x).to(DEV)
    return dict(q=t(rng.integers(0, 3, (Q, na)).astype(np.uint8)), r=t(rng.integers(0, 3, (R, nb)).astype(np.uint8)), qmask=t(rng.random((Q, na)) < 0.8),
                rmask=t(rng.random((R, nb)) < 0.8), qca=t((rng.normal(size=(Q, na, 3)) * 4).astype(np.float32)),
                rca=t((rng.normal(size=(R, nb, 3)) * 4).astype(np.float32)))


def _both(table, pairs=None):
    def call(q, r, qmask, rmask, qca, rca):
        tb = hip.align_traceback(q, r, table, -1, 0, qmask=qmask, rmask=rmask, pairs=pairs, want_rmap=True)
        return dict(tb, **hip.superposed_rmsd_mapped(qca, rca, tb['qmap'], pairs=pairs, qfit=qmask, want_transform=True))
    return call


@pytest.mark.gpu
def test_a_call_equals_its_single_pair_calls():
    """All pairs in one call, each pair in a call of its own (one row a side), and each pair listed alone against the whole panels: the same bytes."""
    t = _small(62)
    table = torch.tensor([[2, -1, 0], [-1, 2, -2], [0, -1, 1]], dtype=torch.int32, device=DEV)
    whole = _both(table)(**t)
    assert int((whole['rmsd'] >= 0).sum()) >= 20
    for x in range(5):
        for y in range(7):
            want = {k: v[x * 7 + y:x * 7 + y + 1] for k, v in whole.items()}
            harness.assert_same_results(_both(table)(**{k: v[x:x + 1] if k.startswith('q') else v[y:y + 1] for k, v in t.items()}), want, (x, y))
            harness.assert_same_results(_both(table, torch.tensor([[x, y]], dtype=torch.int32, device=DEV))(**t), want, (x, y, 'listed'))


@pytest.mark.gpu
def test_calls_are_capturable():
    """Both calls recorded with torch.cuda.graph and replayed on OTHER inputs copied into the static tensors give what the eager calls give on them."""
    table = torch.tensor([[2, -1, 0], [-1, 2, -2], [0, -1, 1]], dtype=torch.int32, device=DEV)
    pairs = torch.tensor([[4, 6], [0, 0], [2, 3], [2, 3], [1, 5]], dtype=torch.int32, device=DEV)
    for call in (_both(table), _both(table, pairs)):
        t, other = _small(63), _small(64)
        eager = {k: v.clone() for k, v in call(**t).items()}
        first, held = harness.capture_replays_on_other_inputs(call, t, other)
        harness.assert_same_results(first, eager, 'the first replay against the eager call')
        assert not torch.equal(held['qmap'], first['qmap']) and not torch.equal(held['rmsd'], first['rmsd'])


@pytest.mark.gpu
def test_empty_calls_and_unsupported_width():
    q, r, t = torch.zeros(0, 9, dtype=torch.uint8, device=DEV), torch.zeros(4, 5, dtype=torch.uint8, device=DEV), model.identity_table()
    none = torch.zeros(0, 2, dtype=torch.int32, device=DEV)
    out = hip.align_traceback(q, r, t, -2, -1, want_rmap=True)
    assert tuple(out['score'].shape) == (0,) and tuple(out['qmap'].shape) == (0, 9) and tuple(out['ops'].shape) == (0, 14) and tuple(out['rmap'].shape) == (0, 5)
    assert tuple(hip.align_traceback(r, q, t, -2, -1)['qmap'].shape) == (0, 5) and tuple(hip.align_traceback(r, r, t, -2, -1, pairs=none)['columns'].shape) == (0,)
    z = lambda *s: torch.zeros(*s, device=DEV)
    out = hip.superposed_rmsd_mapped(z(0, 9, 3), z(4, 5, 3), torch.zeros(0, 9, dtype=torch.int16, device=DEV), want_transform=True)
    assert tuple(out['rmsd'].shape) == (0,) and tuple(out['rot'].shape) == (0, 3, 3)
    assert tuple(hip.superposed_rmsd_mapped(z(4, 5, 3), z(4, 5, 3), torch.zeros(0, 5, dtype=torch.int16, device=DEV), pairs=none)['n_fit'].shape) == (0,)
    # pairs listed against an empty panel: every one lies outside it
    some = torch.tensor([[0, 0], [1, 2]], dtype=torch.int32, device=DEV)
    out = hip.align_traceback(q, r, t, -2, -1, pairs=some)
    assert out['columns'].tolist() == [0, 0] and bool((out['qmap'] == -1).all()) and not bool(out['ops'].any())
    wide = torch.zeros(2, 257, dtype=torch.uint8, device=DEV)
    wide3 = torch.zeros(2, 257, 3, device=DEV)
    i32 = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    f32 = torch.full((4,), 7.0, device=DEV)
    maps = torch.full((4, 257), 7, dtype=torch.int16, device=DEV)
    tab = t.to(DEV)
    L_ = hip.lib()
    rc = L_.abopt_align_traceback(hip.ptr(wide), None, hip.ptr(wide), None, hip.ptr(tab), 21, -2, -1, None, 0, 2, 2, 257, 257, hip.ptr(i32), hip.ptr(i32), hip.ptr(i32),
                                  None, hip.ptr(maps), None, hip.stream())
    rc2 = L_.abopt_superposed_rmsd_mapped(hip.ptr(wide3), hip.ptr(wide3), hip.ptr(maps), None, 0, None, None, None, None, 2, 2, 257, 257, hip.ptr(f32), hip.ptr(i32),
                                          hip.ptr(i32), None, None, hip.stream())
    torch.cuda.synchronize()
    assert rc == 3 and rc2 == 3 and bool((i32 == 7).all()) and bool((f32 == 7).all()) and bool((maps == 7).all())       # ABOPT_EUNSUPPORTED, nothing launched


@pytest.mark.gpu
def test_folded_grid():
    """Q R just past the 2^22 workgroups of one grid row (four pairs each) at length 3: the pairs of the second row equal the statement, like all the others.
    The rows are drawn from eight distinct ones per side, so the statement is 64 pairs."""
    rng = np.random.default_rng(65)
    Q, R, n = 4097, 4096, 3
    assert Q * R > 4 << 22
    base = dict(q=rng.integers(0, 2, (8, n)).astype(np.uint8), r=rng.integers(0, 2, (8, n)).astype(np.uint8), qmask=rng.random((8, n)) < 0.8,
                rmask=rng.random((8, n)) < 0.8)
    table = np.array([[1, 0], [0, 1]], dtype=np.int32)
    want = at.trace_rows(base['q'], base['qmask'], base['r'], base['rmask'], table, -1, -1)
    iq, ir = torch.from_numpy(rng.integers(0, 8, Q)).to(DEV), torch.from_numpy(rng.integers(0, 8, R)).to(DEV)
    d = {k: torch.from_numpy(v).to(DEV)[iq if k.startswith('q') else ir].contiguous() for k, v in base.items()}
    got = hip.align_traceback(d['q'], d['r'], torch.from_numpy(table).to(DEV), -1, -1, qmask=d['qmask'], rmask=d['rmask'], want_rmap=True)
    which = (iq[:, None] * 8 + ir[None]).reshape(-1)
    for name in INT_FIELDS:
        assert torch.equal(got[name], torch.from_numpy(want[name]).to(DEV)[which]), name


@pytest.mark.gpu
def test_sampler_aligned_rmsd_on_the_screen_complex():
    """The native against itself: seqid 100, the identity map on the generated residues, rmsd 0 within the contract; a reference one residue longer (residue 5
    doubled, as in test_similarity.py): one gap column, every residue paired, rmsd 0 still -- in another frame."""
    one = screen_workers.complex_(DEV)
    res = sampler.aligned_rmsd(one, one['aa'], one['pos_heavyatom'], one['mask_heavyatom'], want_transform=True)
    gen = one['generate_flag'][0].bool()
    n, L = int(gen.sum()), gen.shape[0]
    assert n >= 8 and L <= 256 and set(res) == {'seqid', 'score', 'matches', 'columns', 'n_pairs', 'rmsd', 'qmap', 'ops', 'rot', 'trans'}
    assert res['seqid'].tolist() == [100.0] and res['matches'].tolist() == [n] == res['columns'].tolist() == res['n_pairs'].tolist()
    ident = torch.where(gen, torch.arange(L, device=DEV), torch.full((L,), -1, device=DEV)).to(torch.int16)
    assert torch.equal(res['qmap'][0], ident) and res['ops'][0, :n].tolist() == [1] * n and not bool(res['ops'][0, n:].any())
    assert 0.0 <= res['rmsd'].item() <= ABS
    cols = torch.nonzero(gen)[:, 0]
    loop, ca = one['aa'][:1, cols], one['pos_heavyatom'][0, cols, 1]
    longer = torch.cat([loop[:, :6], loop[:, 5:]], 1)
    rot, shift = sp.random_motion(np.random.default_rng(66), 30.0)
    far = torch.cat([ca[:6], ca[5:]]).double() @ torch.from_numpy(rot).to(DEV).T + torch.from_numpy(shift).to(DEV)
    res = sampler.aligned_rmsd(one, one['aa'], one['pos_heavyatom'], one['mask_heavyatom'], ref_seqs=longer, ref_ca=far.float()[None], gap_open=-4, gap_extend=-1)
    assert tuple(res['rmsd'].shape) == (1, 1) and res['columns'].tolist() == [[n + 1]] and res['matches'].tolist() == [[n]] == res['n_pairs'].tolist()
    assert res['score'].tolist() == [[2 * n - 4]] and res['seqid'].item() == pytest.approx(100.0 * n / (n + 1), rel=1e-6)
    paired = res['qmap'][0, 0][cols].cpu().numpy().astype(int)
    x, y = ca.cpu().numpy(), far.float().cpu().numpy()
    zero = at.mapped_pair(x, y, paired)['rmsd']
    assert (np.diff(paired) >= 1).all() and sorted(set(range(n + 1)) - set(paired.tolist())) in ([5], [6]) and zero < 1e-4
    assert abs(res['rmsd'].item() - zero) <= REL * zero + ABS
