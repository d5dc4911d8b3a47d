"""abopt_align_sequences and abopt_gapped_rmsd (csrc/similarity.hip): the numpy statements of tests/similarity_statement.py against brute
force on the CPU, the device against the statements -- the three integers exactly, sd bit for bit -- on the GPU.

The float32 bound (test_float32_statement_agrees_with_float64).  With u = 2^-24: a difference of two fp32 coordinates is rounded once, so its square carries
2 u; the product and the two fmaf of the distance add one rounding each, all terms being non-negative: d is within 5 u of the exact value on the fp32 inputs.
A placement's sum adds its M non-negative terms one by one, M - 1 roundings: within (M + 4) u, plus second-order terms.  Rounding is monotone, so the
recurrence's result is the least of the placements' fp32 sums, and the least of numbers that are each within a relative eps of their exact values is within eps
of the least exact value.  The float64 statement's own error is 2^-29 times smaller.  Bound: |sd32 - sd64| <= (M + 8) 2^-24 sd64."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import scorer_harness as harness
import screen_workers
import similarity_statement as st
from ab_opt_amd import hip, model, sampler, screen
from scorer_harness import DEV

LENS_A = ([1, 3, 5, 64, 127, 129, 256], [2, 4, 63, 65, 128, 255])           # query lengths, reference lengths: 42 pairs, shorter and longer queries
LENS_B = ([2, 4, 63, 65, 128, 255, 256, 0], [1, 3, 5, 64, 127, 129, 256, 0])   # 64 pairs, equal lengths and an all-false row on either side
# (tag, lengths or None = NULL masks on rows of widths (na, nb), letters, T, symmetric table, gap_open, gap_extend)
CASES = [('ties', LENS_A, 2, 2, True, -3, -1),
         ('ties-flat-gaps', LENS_B, 2, 2, False, -2, -2),
         ('free-extension', LENS_B, 21, 21, True, -5, 0),
         ('bytes-past-T', LENS_A, 25, 21, False, -11, -1),
         ('no-gap-cost', LENS_A, 3, 3, True, 0, 0),
         ('null-masks-wide-r', (65, 256), 21, 21, False, -4, -2),
         ('null-masks-wide-q', (256, 63), 2, 2, True, -1, -1)]


def _table(rng, T, symmetric, lo=-6, hi=9):
    t = rng.integers(lo, hi, (T, T))
    return (np.triu(t) + np.triu(t, 1).T if symmetric else t).astype(np.int32)


def _masks(rng, lengths, width):
    """one row per length: that many true bytes at random places (not a prefix unless the row is full or empty)"""
    m = np.zeros((len(lengths), width), dtype=bool)
    for k, n in enumerate(lengths):
        m[k, rng.choice(width, n, replace=False)] = True
    return m


@functools.lru_cache(maxsize=None)
def case(tag):
    """inputs of a case and what the statements give on them, computed once"""
    _, lens, letters, T, symmetric, go, ge = next(c for c in CASES if c[0] == tag)
    rng = np.random.default_rng(sum(map(ord, tag)))
    if isinstance(lens[0], int):
        na, nb, Q, R = lens[0], lens[1], 3, 2
        qmask = rmask = None
    else:
        na = nb = 256
        Q, R = len(lens[0]), len(lens[1])
        qmask, rmask = _masks(rng, lens[0], na), _masks(rng, lens[1], nb)
    c = dict(q=rng.integers(0, letters, (Q, na)).astype(np.uint8), r=rng.integers(0, letters, (R, nb)).astype(np.uint8), qmask=qmask, rmask=rmask,
             table=_table(rng, T, symmetric), gap_open=go, gap_extend=ge,
             qca=(rng.normal(size=(Q, na, 3)) * 6).astype(np.float32), rca=(rng.normal(size=(R, nb, 3)) * 6).astype(np.float32))
    c['want'] = st.align_rows(c['q'], qmask, c['r'], rmask, c['table'], go, ge)
    c['want_sd'] = st.sd_rows(c['qca'], qmask, c['rca'], rmask)
    return c


def _dev(c, *names):
    return [None if c[n] is None else torch.from_numpy(c[n]).to(DEV) for n in names]


# ------------------------------------------------------------------------------------------ CPU: the statements
def test_alignment_statement_equals_brute_force():
    """The recurrence, cell by cell on tuples and a row at a time on int64, against the enumeration of every alignment: 300 random pairs of length <= 5 over two
    or three letters (ties everywhere), random tables, every gap_open <= gap_extend <= 0 in reach -- among them equal gaps and a free extension."""
    rng = np.random.default_rng(7)
    tied = 0
    for _ in range(300):
        letters = int(rng.integers(2, 4))
        a, b = rng.integers(0, letters, rng.integers(1, 6)), rng.integers(0, letters, rng.integers(1, 6))
        table = _table(rng, int(rng.integers(1, letters + 1)), bool(rng.integers(2)), -3, 4)
        go = -int(rng.integers(0, 6))
        ge = -int(rng.integers(0, -go + 1))
        want = st.align_brute(a, b, table, go, ge)
        assert st.align_slow(a, b, table, go, ge) == want == st.align_pair(a, b, table, go, ge), (a, b, table, go, ge)
        tied += want[2] != max(len(a), len(b))
    assert tied > 50                                                 # the optimum is often not the plain overlap: gaps inside and overhangs are exercised


def test_alignment_rows_agree_with_cells_on_longer_sequences():
    rng = np.random.default_rng(8)
    for n, m, letters in ((40, 70, 2), (64, 65, 21), (90, 33, 4), (1, 80, 2), (77, 1, 3)):
        a, b = rng.integers(0, letters + 2, n), rng.integers(0, letters + 2, m)
        table = _table(rng, letters, False)
        for go, ge in ((-7, -1), (-2, -2), (-4, 0), (0, 0)):
            assert st.align_pair(a, b, table, go, ge) == st.align_slow(a, b, table, go, ge), (n, m, letters, go, ge)


def test_alignment_hand_cases():
    t = model.identity_table().numpy()
    assert t.shape == (21, 21) and t.dtype == np.int32 and t[3, 3] == 2 and t[3, 4] == -2 and t[20, 20] == 2
    al = lambda a, b, go=-20, ge=-1: st.align_pair(a, b, t, go, ge)
    a = [0, 7, 3, 3, 12, 19, 5, 9, 9, 1, 15, 2, 8, 4, 16, 17, 6, 11, 13, 10, 18, 14, 0, 3]
    assert al(a, a) == (2 * len(a), len(a), len(a))                  # identical: every column a match
    ins = a[:12] + [6] + a[12:]                                      # one residue inserted in the middle: one paid gap column
    assert al(a, ins) == al(ins, a) == (2 * len(a) - 20, len(a), len(a) + 1)
    assert al(a, a[12:]) == (24, 12, 24) and al(a[:12], a) == (24, 12, 24)          # an overhang at either end is free, and counts in columns
    assert al(a[4:16], a) == al(a, a[4:16]) == (24, 12, 24)                         # ... at both ends
    assert al([], a) == al(a, []) == (0, 0, len(a)) and al([], []) == (0, 0, 0)     # an empty side
    assert al([0, 1], [2, 3]) == (0, 0, 4)                           # nothing worth pairing: two free runs, one at either end
    assert al([30, 40], [30, 40]) == (4, 2, 2) and al([30], [40]) == (2, 0, 1)      # bytes >= T read entry T - 1; a match is decided on the raw bytes
    assert st.align_pair(a, ins, t, -20, -20) == (2 * len(a) - 20, len(a), len(a) + 1)


def test_rmsd_statement_is_the_adjacent_last_minimum():
    """sd_table (the reference's recurrence, cell by cell) == sd_pair (the band form) in float32 bit for bit and in float64; both equal the brute-force minimum
    over the placements whose last two residues are adjacent, and differ from the minimum over all placements on a chosen input."""
    rng = np.random.default_rng(9)
    differs = 0
    for _ in range(200):
        q, r = (rng.normal(size=(rng.integers(1, 7), 3)) * 3).astype(np.float32), (rng.normal(size=(rng.integers(1, 7), 3)) * 3).astype(np.float32)
        t32, p32, t64, p64 = st.sd_table(q, r), st.sd_pair(q, r), st.sd_table(q, r, np.float64), st.sd_pair(q, r, np.float64)
        assert t32[1] == p32[1] == min(len(q), len(r)) and t32[0].dtype == np.float32 and t32[0].tobytes() == p32[0].tobytes()
        adjacent, free = st.sd_brute(q, r, True), st.sd_brute(q, r, False)
        assert t64[0] == p64[0] and abs(t64[0] - adjacent) <= 1e-12 * adjacent
        differs += free < adjacent * (1 - 1e-9)
    assert differs > 10
    # the chosen input: s = (0, 10) on a line, l = (0, 5, 10).  Placing s on l[0], l[2] costs 0 but is not adjacent-last: the recurrence gives 25 (l[1], l[2])
    line = lambda *x: np.array([[v, 0, 0] for v in x], dtype=np.float32)
    s, l = line(0, 10), line(0, 5, 10)
    assert st.sd_brute(s, l, False) == 0 and st.sd_brute(s, l, True) == 25
    assert st.sd_table(s, l) == (25, 2) == st.sd_table(l, s) and st.sd_pair(s, l) == (25, 2)
    assert st.sd_table(s, s) == (0, 2) and st.sd_pair(line(), s) == (-1, 0) and st.sd_table(s, line()) == (-1, 0)
    assert st.sd_pair(line(7), l) == (4, 1)                          # M = 1: the nearest residue


def test_float32_statement_agrees_with_float64():
    """|sd32 - sd64| <= (M + 8) 2^-24 sd64, the bound derived at the top of this file, on lists of every length class of the GPU cases."""
    rng = np.random.default_rng(10)
    worst = 0.0
    for nq, nr in ((1, 1), (5, 64), (63, 65), (128, 129), (127, 256), (256, 255), (256, 256), (2, 256), (200, 40)):
        q, r = (rng.normal(size=(nq, 3)) * 6).astype(np.float32), (rng.normal(size=(nr, 3)) * 6).astype(np.float32)
        (s32, M), (s64, _) = st.sd_pair(q, r), st.sd_pair(q, r, np.float64)
        rel = abs(float(s32) - s64) / s64
        worst = max(worst, rel / ((M + 8) * 2.0 ** -24))
        assert rel <= (M + 8) * 2.0 ** -24, (nq, nr, rel)
    print(f'largest |sd32 - sd64| / sd64 as a fraction of the bound: {worst:.3f}')


def test_tables():
    t = model.identity_table(5, -4)
    assert t.dtype == torch.int32 and tuple(t.shape) == (21, 21) and int(t.diagonal().min()) == 5 and int((t - torch.diag(t.diagonal())).max()) == 0 \
        and int(t.min()) == -4
    for bad in (dict(match=1.5), dict(mismatch=40000), dict(match=True)):
        with pytest.raises(ValueError, match='identity_table'):
            model.identity_table(**bad)
    # an alphabet in another order, with halves, lacking W and Y, with a letter the library has not (B) and with X
    letters = 'XBVTSRQPNMLKIHGFEDCA'
    rng = np.random.default_rng(11)
    m = rng.integers(-8, 9, (20, 20)) / 2.0
    t = model.substitution_table(letters, m, scale=2)
    assert t.dtype == torch.int32 and tuple(t.shape) == (21, 21)
    low = int(2 * min(m[i, j] for i in range(20) for j in range(20) if letters[i] != 'B' and letters[j] != 'B'))
    for i, a in enumerate(model.AA_LETTERS + 'X'):
        for j, b in enumerate(model.AA_LETTERS + 'X'):
            want = low if a in 'WY' or b in 'WY' else int(2 * m[letters.index(a), letters.index(b)])
            assert int(t[i, j]) == want, (a, b)
    assert torch.equal(model.substitution_table(letters.lower(), m, scale=2), t)
    assert int(model.substitution_table('AC', [[1, 0], [0, 1]], scale=3)[20, 20]) == 0          # no X: "no type" takes the minimum
    with pytest.raises(ValueError, match='integer'):
        model.substitution_table(letters, m, scale=1)
    with pytest.raises(ValueError, match='repeats'):
        model.substitution_table('AAC', np.zeros((3, 3)))
    with pytest.raises(ValueError, match='does not fit'):
        model.substitution_table('ACD', np.zeros((2, 2)))
    with pytest.raises(ValueError, match='32767'):
        model.substitution_table('AC', [[1, 0], [0, 1]], scale=40000)
    with pytest.raises(ValueError, match='none of'):
        model.substitution_table('BZ', np.zeros((2, 2)))


def test_bad_arguments_are_refused_before_any_launch():
    """Every ValueError of the two wrappers on CPU tensors (nothing has touched a device), the refusal of a CPU tensor once everything else is valid, and the
    return codes of the C entries on dummy pointers that are never dereferenced -- ABOPT_EUNSUPPORTED for a row of 257 among them."""
    q, r, t = torch.zeros(3, 9, dtype=torch.uint8), torch.zeros(2, 12, dtype=torch.int64), model.identity_table()
    al = hip.align_sequences
    for bad in (q[0], q.float(), torch.zeros(3, 9, 1, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r'q .* must be integer \(rows, n\)'):
            al(bad, r, t, -2, -1)
    with pytest.raises(ValueError, match=r'r .* must be integer'):
        al(q, r.double(), t, -2, -1)
    with pytest.raises(ValueError, match='r has 257 elements per row, expected 1 .. 256'):
        al(q, torch.zeros(2, 257, dtype=torch.uint8), t, -2, -1)
    with pytest.raises(ValueError, match='q has 0 elements per row'):
        al(q[:, :0], r, t, -2, -1)
    with pytest.raises(ValueError, match=r'mask of q .* must be \(rows, n\)'):
        al(q, r, t, -2, -1, qmask=torch.ones(3, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match=r'mask of r .* must be \(rows, n\)'):
        al(q, r, t, -2, -1, rmask=torch.ones(3, 12, dtype=torch.bool))
    for bad in (t[0], t[:, :20], t.float(), torch.zeros(33, 33, dtype=torch.int32), torch.zeros(0, 0, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r'table .* must be integer of shape \(T, T\)'):
            al(q, r, bad, -2, -1)
    for go, ge in ((1, 0), (-2, 1), (-1, -2), (-40000, -1)):
        with pytest.raises(ValueError, match='gap_open <= gap_extend <= 0'):
            al(q, r, t, go, ge)
    for go, ge in ((-1.5, -1), (-2, -0.5), (True, 0)):
        with pytest.raises(ValueError, match='must be an integer'):
            al(q, r, t, go, ge)
    with pytest.raises(ValueError, match='HIP device only'):                            # everything valid: the CPU tensor is refused before anything is allocated
        al(q, r, t, -2, -1, qmask=torch.ones(3, 9, dtype=torch.bool))
    qca, rca = torch.zeros(3, 9, 3), torch.zeros(2, 12, 3, dtype=torch.float64)
    gr = hip.gapped_rmsd
    for bad in (qca[0], qca[:, :, :2], qca.long()):
        with pytest.raises(ValueError, match=r'qca .* must be floating point \(rows, n, 3\)'):
            gr(bad, rca)
    with pytest.raises(ValueError, match='rca has 300 elements per row'):
        gr(qca, torch.zeros(2, 300, 3))
    with pytest.raises(ValueError, match=r'mask of rca .* must be'):
        gr(qca, rca, rmask=torch.ones(2, 9, dtype=torch.bool))
    with pytest.raises(ValueError, match='HIP device only'):
        gr(qca, rca, qmask=torch.ones(3, 9, dtype=torch.bool))
    batch = dict(aa=torch.zeros(1, 9, dtype=torch.long), generate_flag=torch.zeros(1, 9, dtype=torch.bool), fragment_type=torch.ones(1, 9, dtype=torch.long))
    with pytest.raises(ValueError, match='rows must be'):
        sampler.similarity(batch, q[:1], torch.zeros(1, 9, 4, 3), torch.ones(1, 9, 4, dtype=torch.bool), rows='designed')
    with pytest.raises(ValueError, match=r'expected seqs \(G\*S, L\)'):
        sampler.similarity(batch, q[:1], torch.zeros(1, 9, 1, 3), torch.ones(1, 9, 1, dtype=torch.bool))

    L_ = hip.lib()
    dummy = (ctypes.c_char * 16)()
    a = ctypes.c_void_p(ctypes.addressof(dummy))

    def align(Q=3, R=2, na=9, nb=12, T=21, go=-2, ge=-1, q=a, table=a, columns=a):
        return L_.abopt_align_sequences(q, None, a, None, table, T, go, ge, Q, R, na, nb, a, a, columns, None)

    def rmsd(Q=3, R=2, na=9, nb=12, qca=a, m=a):
        return L_.abopt_gapped_rmsd(qca, None, a, None, Q, R, na, nb, a, m, None)
    for fn in (align, rmsd):
        for kw, rc, word in ((dict(na=257), 3, '256'), (dict(nb=257), 3, '256'), (dict(na=0), 1, 'bad dims'), (dict(Q=-1), 1, 'bad dims'),
                             (dict(Q=65536, R=65536), 1, 'bad dims'), (dict(Q=0, na=257), 3, '256')):
            assert fn(**kw) == rc and word in L_.abopt_last_error().decode(), (fn.__name__, kw, L_.abopt_last_error().decode())
    for kw, word in ((dict(T=0), 'T=0'), (dict(T=33), 'T=33'), (dict(go=1, ge=1), 'gap_open'), (dict(go=-1, ge=-2), 'gap_open'), (dict(go=-32768), 'gap_open'),
                     (dict(q=None), 'NULL'), (dict(table=None), 'NULL'), (dict(columns=None), 'NULL')):
        assert align(**kw) == 1 and word in L_.abopt_last_error().decode(), (kw, L_.abopt_last_error().decode())
    for kw in (dict(qca=None), dict(m=None)):
        assert rmsd(**kw) == 1 and 'NULL' in L_.abopt_last_error().decode()
    assert align(Q=0) == 0 and align(R=0, q=None) == 0 and rmsd(Q=0, qca=None) == 0 and rmsd(R=0) == 0      # no-ops, between the value checks and the pointer checks
    assert align(Q=0, T=0) == 1


def test_binding_and_header_agree_on_the_new_entries():
    """The export list still equals the header (tests/test_abi.py checks every signature; this names the two new ones), and the ABI is still 59."""
    from test_abi import parse_header, signature_mismatches
    protos = parse_header()[0]
    assert {'abopt_align_sequences', 'abopt_gapped_rmsd'} <= set(protos) and set(hip.EXPORTS) == set(protos)
    assert signature_mismatches(hip._SIGNATURES, protos) == {}
    assert hip.ABI_VERSION == 59 and hip.lib().abopt_abi_version() == 59
    assert len(protos['abopt_align_sequences'][1]) == 16 and len(protos['abopt_gapped_rmsd'][1]) == 11


def _designs(one, S, seed):
    """S copies of a complex's sequence with 0 .. 2 substitutions each among its generated residues -> (seqs (S, L), the generated columns)"""
    rng = np.random.default_rng(seed)
    aa = one['aa'][0].cpu().numpy()
    cols = np.nonzero(one['generate_flag'][0].cpu().numpy())[0]
    seqs = np.repeat(aa[None], S, 0)
    for s in range(1, S):
        for c in rng.choice(cols, rng.integers(1, 3), replace=False):
            seqs[s, c] = (seqs[s, c] + 1 + rng.integers(19)) % 20
    return seqs, cols


def test_near_identical_designs_align_without_gaps():
    """What the GPU test of sampler.similarity relies on, by the statement: designs of one length that differ in a few substitutions align column on column, so
    matches is the length minus the Hamming distance."""
    from ab_opt_amd.utils import synth
    one = synth.make_batch(1, synth.LAYOUT_128, seed=21)
    seqs, cols = _designs(one, 6, 3)
    loops = seqs[:, cols]
    score, matches, columns = st.align_rows(loops, None, loops, None, model.identity_table().numpy(), -20, -1)
    ham = (loops[:, None] != loops[None]).sum(-1)
    assert ham.max() >= 2 and np.array_equal(matches, len(cols) - ham) and (columns == len(cols)).all() and np.array_equal(score, 2 * len(cols) - 4 * ham)


# ------------------------------------------------------------------------------------------ GPU
def _align(c):
    q, r, qmask, rmask, table = _dev(c, 'q', 'r', 'qmask', 'rmask', 'table')
    return hip.align_sequences(q, r, table, c['gap_open'], c['gap_extend'], qmask=qmask, rmask=rmask)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', [c[0] for c in CASES])
def test_device_equals_the_statements(tag):
    """score, matches, columns exactly and sd bit for bit, on every length class crossed with shorter and longer partners, masks that are no prefixes, all-false
    rows and NULL masks, two and 21 letters, bytes >= T, symmetric and asymmetric tables, gap_extend == gap_open and gap_extend == 0."""
    c = case(tag)
    got = _align(c)
    for name, want in zip(('score', 'matches', 'columns'), c['want']):
        assert got[name].dtype == torch.int32 and np.array_equal(got[name].cpu().numpy(), want), (tag, name)
    qca, rca, qmask, rmask = _dev(c, 'qca', 'rca', 'qmask', 'rmask')
    out = hip.gapped_rmsd(qca, rca, qmask=qmask, rmask=rmask)
    sd, m = c['want_sd']
    assert np.array_equal(out['m'].cpu().numpy(), m), tag
    assert np.array_equal(out['sd'].cpu().numpy().view(np.int32), sd.view(np.int32)), tag
    with np.errstate(invalid='ignore'):
        rmsd = np.where(m > 0, np.sqrt(sd / np.maximum(m, 1).astype(np.float32)), np.float32(-1))
    assert np.allclose(out['rmsd'].cpu().numpy(), rmsd.astype(np.float32), rtol=1e-6, atol=0), tag


def _small(seed, Q=5, R=7, na=9, nb=12):
    rng = np.random.default_rng(seed)
    t = lambda x: torch.from_numpy(x).to(DEV)
    return dict(q=t(rng.integers(0, 4, (Q, na)).astype(np.uint8)), r=t(rng.integers(0, 4, (R, nb)).astype(np.uint8)), qmask=t(rng.random((Q, na)) < 0.7),
                rmask=t(rng.random((R, nb)) < 0.7), qca=t((rng.normal(size=(Q, na, 3)) * 4).astype(np.float32)),
                rca=t((rng.normal(size=(R, nb, 3)) * 4).astype(np.float32)))


def _both(table):
    def call(q, r, qmask, rmask, qca, rca):
        return dict(hip.align_sequences(q, r, table, -3, -1, qmask=qmask, rmask=rmask), **hip.gapped_rmsd(qca, rca, qmask=qmask, rmask=rmask))
    return call


@pytest.mark.gpu
def test_a_call_equals_its_single_pair_calls():
    t = _small(12)
    call = _both(torch.from_numpy(_table(np.random.default_rng(12), 4, False)).to(DEV))
    whole = call(**t)
    for x in range(5):
        for y in range(7):
            one = call(**{k: v[x:x + 1] if k.startswith('q') else v[y:y + 1] for k, v in t.items()})
            harness.assert_same_results(one, {k: v[x:x + 1, y:y + 1] for k, v in whole.items()}, (x, y))


@pytest.mark.gpu
def test_folded_grid():
    """Q R just past the 2^22 workgroups of one grid row (four pairs each): the pairs of the second row equal the statement, like all the others.  The rows are
    drawn from eight distinct ones per side, so the statement is 64 pairs."""
    rng = np.random.default_rng(13)
    Q, R, n = 4097, 4096, 3
    assert Q * R > 4 << 22
    base = dict(q=rng.integers(0, 2, (8, n)).astype(np.uint8), r=rng.integers(0, 2, (8, n)).astype(np.uint8), qmask=rng.random((8, n)) < 0.8,
                rmask=rng.random((8, n)) < 0.8, qca=(rng.normal(size=(8, n, 3)) * 3).astype(np.float32), rca=(rng.normal(size=(8, n, 3)) * 3).astype(np.float32))
    table = _table(rng, 2, False)
    iq, ir = torch.from_numpy(rng.integers(0, 8, Q)).to(DEV), torch.from_numpy(rng.integers(0, 8, R)).to(DEV)
    d = {k: torch.from_numpy(v).to(DEV)[iq if k.startswith('q') else ir].contiguous() for k, v in base.items()}
    want = dict(zip(('score', 'matches', 'columns'), st.align_rows(base['q'], base['qmask'], base['r'], base['rmask'], table, -2, -1)))
    want['sd'], want['m'] = st.sd_rows(base['qca'], base['qmask'], base['rca'], base['rmask'])
    got = dict(hip.align_sequences(d['q'], d['r'], torch.from_numpy(table).to(DEV), -2, -1, qmask=d['qmask'], rmask=d['rmask']),
               **hip.gapped_rmsd(d['qca'], d['rca'], qmask=d['qmask'], rmask=d['rmask']))
    for name, w in want.items():
        assert torch.equal(got[name], torch.from_numpy(w).to(DEV)[iq][:, ir]), name


@pytest.mark.gpu
def test_calls_are_capturable():
    """Both calls recorded with torch.cuda.graph and replayed on OTHER inputs copied into the static tensors give what the eager calls give on them."""
    call = _both(torch.from_numpy(_table(np.random.default_rng(14), 4, True)).to(DEV))
    t, other = _small(14), _small(15)
    eager = {k: v.clone() for k, v in call(**t).items()}
    first, held = harness.capture_replays_on_other_inputs(call, t, other)
    harness.assert_same_results(first, eager, 'the first replay against the eager call')
    assert not torch.equal(held['score'], first['score']) and not torch.equal(held['sd'], first['sd'])


@pytest.mark.gpu
def test_empty_calls_and_unsupported_width():
    q, r, t = torch.zeros(0, 9, dtype=torch.uint8, device=DEV), torch.zeros(4, 5, dtype=torch.uint8, device=DEV), model.identity_table()
    assert tuple(hip.align_sequences(q, r, t, -2, -1)['score'].shape) == (0, 4) and tuple(hip.align_sequences(r, q, t, -2, -1)['columns'].shape) == (4, 0)
    assert tuple(hip.gapped_rmsd(torch.zeros(0, 9, 3, device=DEV), torch.zeros(4, 5, 3, device=DEV))['rmsd'].shape) == (0, 4)
    wide = torch.zeros(2, 257, dtype=torch.uint8, device=DEV)
    out = torch.full((2, 2), 7, dtype=torch.int32, device=DEV)
    tab = t.to(DEV)
    rc = hip.lib().abopt_align_sequences(hip.ptr(wide), None, hip.ptr(wide), None, hip.ptr(tab), 21, -2, -1, 2, 2, 257, 257, hip.ptr(out), hip.ptr(out), hip.ptr(out),
                                         hip.stream())
    torch.cuda.synchronize()
    assert rc == 3 and bool((out == 7).all())                        # ABOPT_EUNSUPPORTED, and nothing was launched


@pytest.mark.gpu
def test_sampler_similarity_on_the_screen_complex():
    """With defaults the native against itself has seqid 100 and rmsd 0; designs of the loop's length give the Hamming counts of cluster_sequences; a reference
    of another length and rows='antibody' run through the same call."""
    one = screen_workers.complex_(DEV)
    res = sampler.similarity(one, one['aa'], one['pos_heavyatom'], one['mask_heavyatom'])
    n = int(one['generate_flag'].sum())
    assert n >= 8 and set(res) == {'seqid', 'score', 'matches', 'columns', 'rmsd', 'sd', 'm'}
    assert res['seqid'].tolist() == [100.0] and res['rmsd'].tolist() == [0.0] and res['matches'].tolist() == [n] == res['columns'].tolist() == res['m'].tolist()
    S = 6
    seqs, cols = _designs(one, S, 3)
    seqs = torch.from_numpy(seqs).to(DEV)
    pos, mask = one['pos_heavyatom'].expand(S, -1, -1, -1), one['mask_heavyatom'].expand(S, -1, -1)
    loops = seqs[:, torch.from_numpy(cols).to(DEV)]
    res = sampler.similarity(one, seqs, pos, mask, ref_seqs=loops)
    dist = hip.cluster_sequences_grouped(loops, S, 0, want_dist=True)['dist'][0]
    assert int(dist.max()) >= 2 and torch.equal(res['matches'], n - dist) and bool((res['columns'] == n).all()) and set(res) == {'seqid', 'score', 'matches', 'columns'}
    assert torch.equal(res['seqid'], 100.0 * res['matches'].float() / torch.full_like(res['seqid'], n))    # a tensor: a division, not a reciprocal
    own = sampler.similarity(one, seqs, pos, mask)
    assert torch.equal(own['matches'], res['matches'][:, 0]) and bool((own['rmsd'] == 0).all()) and bool((own['m'] == n).all())
    # a reference loop one residue longer (residue 5 doubled): one paid gap column in the sequence, and a placement of the native loop that costs nothing
    ca = one['pos_heavyatom'][0, torch.from_numpy(cols).to(DEV), 1]
    longer = torch.cat([loops[:1, :6], loops[:1, 5:]], 1)
    ref_ca = torch.cat([ca[:6], ca[5:]])[None]
    res = sampler.similarity(one, seqs[:1], pos[:1], mask[:1], ref_seqs=longer, ref_ca=ref_ca, gap_open=-4, gap_extend=-1)
    assert res['columns'].tolist() == [[n + 1]] and res['matches'].tolist() == [[n]] and res['score'].tolist() == [[2 * n - 4]]
    assert res['m'].tolist() == [[n]] and res['rmsd'].tolist() == [[0.0]]
    whole = sampler.similarity(one, seqs, pos, mask, rows='antibody')
    ab = int((screen.chain_groups(one['fragment_type']) == 1).sum())
    assert ab > n and bool((whole['columns'] == ab).all()) and torch.equal(whole['matches'], ab - dist[:, 0]) and bool((whole['m'] == ab).all())
