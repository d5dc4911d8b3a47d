"""Developability: abopt_sequence_liabilities_grouped / abopt_surface_patches_grouped, their bindings (hip.sequence_liabilities_grouped,
hip.surface_patches_grouped, hip.check_run_min, hip.default_patch_weight), sampler.sequence_liabilities / sampler.developability and the tables of
ab_opt_amd.model.

The definitions are restated in tests/developability_statement.py.  Every output of the liabilities is an integer and the device has to EQUAL liabilities_np; the
patches are fp32 formed in a stated order and the device has to equal patches_f32 on the int32 view.  Random sequences do not hold every motif, so the generator
plants them, and the tests first assert on the statement that every class was counted and was turned down for every reason that applies to it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import developability_statement as st
import scorer_harness as harness
import screen_workers
from ab_opt_amd import hip, model, sampler, screen
from scorer_harness import DEV

# (G, S, n, run_min, rows given, link given): every (G, S) of {(1, 1), (3, 2), (2, 5)}, n of {1, 2, 3, 7, 63, 64, 65, 130, 257}, run_min of {0, 2, 5, 16}, rows and
# link each NULL and given
LIAB_CASES = [(1, 1, 1, 0, False, False), (3, 2, 1, 5, True, True), (2, 5, 2, 2, True, False), (1, 1, 2, 16, False, True), (3, 2, 3, 2, True, True),
              (2, 5, 3, 5, False, False), (1, 1, 7, 5, True, True), (3, 2, 7, 2, False, True), (2, 5, 7, 16, True, False), (1, 1, 63, 5, True, True),
              (3, 2, 63, 16, False, False), (2, 5, 64, 5, True, True), (1, 1, 64, 2, False, True), (3, 2, 65, 5, True, False), (2, 5, 65, 16, True, True),
              (1, 1, 130, 5, True, True), (3, 2, 130, 0, True, True), (2, 5, 130, 16, False, True), (1, 1, 257, 16, True, True), (3, 2, 257, 5, True, True),
              (2, 5, 257, 2, False, False)]
# (G, S, L, A): L of {1, 2, 7, 63, 64, 65, 130, 300} and A of {2, 5, 15}
PATCH_CASES = [(1, 1, 1, 2), (3, 2, 2, 5), (2, 5, 7, 5), (1, 1, 7, 15), (3, 2, 63, 5), (1, 1, 64, 2), (2, 5, 65, 5), (1, 1, 65, 15), (3, 2, 130, 2), (1, 1, 130, 5),
               (1, 1, 300, 5), (2, 3, 300, 15)]
FAR_CASES = [(3, 2, 2, 5), (2, 5, 7, 5), (3, 2, 63, 5), (1, 1, 65, 15), (1, 1, 130, 5), (1, 1, 300, 5)]
RADII = (0.0, 4.5, 10.0, 1000.0)


def custom_weight():
    """a table of another scale with a NaN entry (L takes no part), a negative one and a weight for "no type\""""
    w = st.default_weight() * np.float32(0.37)
    w[st.AA.index('L')] = np.nan
    w[st.AA.index('G')] = -2.25
    w[20] = 2.5
    return w


# ------------------------------------------------------------------------------------------ the statements, computed once
@functools.lru_cache(maxsize=None)
def liab(G, S, n, run_min, with_rows, with_link):
    c = st.liability_case(G, S, n, run_min, with_rows, with_link)
    return dict(c, want=st.liabilities_grouped_np(c['seqs'], S, c['rows'], c['link'], run_min))


def assert_every_rule_is_reached():
    """over the whole table: every class counted at least once, and turned down at least once for each reason that applies to it (the one-residue classes can
    neither run past the end nor hold a link or a byte >= 20)"""
    tally = {}
    for case in LIAB_CASES:
        for key, v in liab(*case)['want']['tally'].items():
            tally[key] = tally.get(key, 0) + v
    for c, name in enumerate(st.NAMES):
        assert tally.get((c, 'counted'), 0) > 0, (name, 'never counted')
        for reason in (('row',) if c in (4, 5) else st.REASONS):
            assert tally.get((c, reason), 0) > 0, (name, 'never turned down for', reason)
    return tally


@functools.lru_cache(maxsize=None)
def patch_want(G, S, L, A, radius, shared=False, custom=False, far=False):
    s = st.structure(G, S, L, A, far)
    seqs = s['seqs'][::S] if shared else s['seqs']
    return st.patches_grouped_f32(s['pos'], s['mask'], s['group'], s['area'], seqs, custom_weight() if custom else st.default_weight(), radius, S)


def patch_inputs(G, S, L, A, far=False):
    s = st.structure(G, S, L, A, far)
    return {k: torch.from_numpy(s[k]).to(DEV) for k in ('pos', 'mask', 'group', 'area', 'seqs')}


def _bits(res):
    """patch as its int32 bit pattern: torch.equal on it is bit for bit"""
    return dict(patch=res['patch'].view(torch.int32), nbr=res['nbr'])


def _assert_patches(got, want, tag):
    patch, nbr = want[0], want[1]
    assert got['patch'].dtype == torch.float32 and got['nbr'].dtype == torch.int32
    g_nbr = got['nbr'].cpu().numpy().astype(np.int64)
    assert np.array_equal(g_nbr, nbr), (tag, np.argwhere(g_nbr != nbr)[:4])
    g_patch = got['patch'].cpu().numpy()
    bad = np.argwhere(g_patch.view(np.int32) != patch.view(np.int32))
    assert not len(bad), (tag, bad[:4], g_patch[tuple(bad[0])], patch[tuple(bad[0])])


def _assert_liabilities(got, want, tag, freq=True):
    assert got['flags'].dtype == torch.uint8 and got['counts'].dtype == torch.int32 and got['hyd10'].dtype == torch.int32
    for name in ('flags', 'counts', 'hyd10') + (('freq',) if freq else ()):
        g = got[name].cpu().numpy().astype(np.int64)
        assert g.shape == want[name].shape and np.array_equal(g, want[name].astype(np.int64)), (tag, name, np.argwhere(g != want[name])[:4])


def _run_liab(c, S, run_min, want_freq=True):
    t = {k: None if c[k] is None else torch.from_numpy(c[k]).to(DEV) for k in ('seqs', 'rows', 'link')}
    return hip.sequence_liabilities_grouped(t['seqs'], S, rows=t['rows'], link=t['link'], run_min=run_min, want_freq=want_freq)


# ------------------------------------------------------------------------------------------ CPU
def test_liability_statement_on_hand_written_sequences():
    """Short strings with the flags written out by hand (bit 0 n_glyc, 1 deamidation, 2 isomerisation, 3 cleavage, 4 cys, 5 met, 6 hydrophobic run)."""
    cases = [('NGT', None, None, 5, [3, 0, 0]),                       # N-G-T: a sequon and N-G
             ('NPS', None, None, 5, [0, 0, 0]),                       # a proline in the middle: no sequon; N-P is nothing
             ('NAS', None, None, 5, [1, 0, 0]),
             ('NGS', None, None, 5, [3, 0, 0]),
             ('NNS', None, None, 5, [1, 2, 0]),                       # N-N-S is a sequon at 0; N-S deamidates at 1 and has no third residue
             ('NS', None, None, 5, [2, 0]),                           # no room for a sequon
             ('DGDSDP', None, None, 5, [4, 0, 4, 0, 8, 0]),
             ('ACM', None, None, 5, [0, 16, 32]),
             ('LLLL', None, None, 5, [0, 0, 0, 0]),
             ('LLLLL', None, None, 5, [64, 0, 0, 0, 0]),
             ('LLLLLL', None, None, 5, [64, 64, 0, 0, 0, 0]),         # every anchor of a window, not only the first of the run
             ('LIVMF', None, None, 5, [64, 0, 0, 32, 0]),
             ('LIVMF', None, None, 0, [0, 0, 0, 32, 0]),              # the class is off
             ('AFWA', None, None, 2, [0, 64, 0, 0]),
             ('NxT', None, None, 5, [0, 0, 0]),                       # a byte of 20 inside the window
             ('NAz', None, None, 5, [0, 0, 0]),                       # ... of 255
             ('NAT', None, [1, 0, 0], 5, [0, 0, 0]),                  # an unlinked step inside the window
             ('NAT', None, [1, 1, 0], 5, [1, 0, 0]),                  # the last entry of link is ignored
             ('NAT', [0, 0, 1], None, 5, [1, 0, 0]),                  # the only scored row is the last residue: a liability of the design
             ('NAT', [0, 0, 0], None, 5, [0, 0, 0]),
             ('DGNG', [0, 0, 1, 0], None, 5, [0, 0, 2, 0]),
             ('CM', [0, 1], None, 5, [0, 32])]
    for text, rows, link, run_min, flags in cases:
        got = st.liabilities_np(st.encode(text)[None], rows, link, run_min)
        assert got['flags'][0].tolist() == flags, (text, rows, link, run_min, got['flags'][0].tolist())
        assert got['counts'][0, 7] == sum(f != 0 for f in flags) and got['freq'].tolist() == [int(f != 0) for f in flags]
        for b in range(7):
            assert got['counts'][0, b] == sum((f >> b) & 1 for f in flags)
    got = st.liabilities_np(st.encode('KRDEHxA')[None], [1, 1, 1, 1, 1, 1, 0], None, 5)
    assert got['counts'][0, 8:].tolist() == [2, 2, 1, 5] and got['hyd10'][0] == -39 - 45 - 35 - 35 - 32
    two = st.liabilities_np(np.stack([st.encode('NGT'), st.encode('AAC')]), None, None, 5)
    assert two['freq'].tolist() == [1, 0, 1] and two['counts'][:, :7].tolist() == [[1, 1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0]]


def test_planted_motifs_reach_every_rule():
    tally = assert_every_rule_is_reached()
    print({f'{st.NAMES[c]}/{r}': v for (c, r), v in sorted(tally.items())})


def test_fused_multiply_add_of_the_statement_is_exact():
    """fma32 against exact rational arithmetic, on operands chosen so that the float64 sum itself is often inexact (a product of 48 bits beside an addend far below)."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = (rng.normal(size=4000) * 10.0 ** rng.integers(-3, 4, 4000)).astype(np.float32)
    b = (rng.normal(size=4000) * 10.0 ** rng.integers(-3, 4, 4000)).astype(np.float32)
    c = (rng.normal(size=4000) * 10.0 ** rng.integers(-12, 4, 4000)).astype(np.float32)
    c[:500] = (-a[:500].astype(np.float64) * b[:500].astype(np.float64)).astype(np.float32)       # cancellation
    got = st.fma32(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    for k in range(4000):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        err = abs(exact - Fraction(float(got[k])))
        others = [abs(exact - Fraction(float(np.nextafter(got[k], np.float32(side))))) for side in (np.inf, -np.inf)]
        assert err <= min(others), (k, a[k], b[k], c[k], got[k])
        assert err < min(others) or (got[k].view(np.int32) & 1) == 0, (k, 'a tie goes to even')
    print(f'the float64 shortcut differs from the exact fma on {(naive != got).sum()} of 4000 operands')
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 lies exactly half way between two fp32 numbers; an addend of +-2^-60 decides the rounding, and a float64 sum loses it
    x, tiny = np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -60)
    assert st.fma32(x, x, tiny)[0] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23) and st.fma32(x, x, -tiny)[0] == np.float32(1 + 2.0 ** -11)
    assert np.float32(np.float64(x) * np.float64(x) + np.float64(tiny)) == np.float32(1 + 2.0 ** -11)          # the shortcut gets the first one wrong


@pytest.mark.parametrize('L,A', [(7, 5), (65, 15), (130, 5)])
def test_float32_patch_statement_agrees_with_float64(L, A):
    """The two statements give the same neighbours on every pair whose float64 margin | |c_i - c_j| - radius | is at least 2^-18 (max |coordinate| + radius): 64
    ulps of the largest magnitude entering a difference.  How many pairs lie inside the margin, near and far from the origin, is printed."""
    for far in (False, True):
        s = st.structure(1, 1, L, A, far)
        for radius in (4.5, 10.0):
            args = (s['pos'][0], s['mask'][0], s['group'][0], s['area'][0], s['seqs'][0], st.default_weight(), radius)
            a, b = st.patches_f32(*args), st.patches_f64(*args, margins=True)
            bound = 2.0 ** -18 * (np.nanmax(np.abs(s['pos'][0][s['mask'][0]])) + radius)
            safe = b['margin'] >= bound
            pairs = np.isfinite(b['margin'])
            differ = a['near'] != b['near']
            print(f'L={L} A={A} radius={radius} far={far}: {pairs.sum()} pairs, {(pairs & ~safe).sum()} within {bound:.2e} A of the radius, {differ.sum()} verdicts differ')
            assert np.array_equal(a['part'], b['part']) and not (differ & safe).any()
            assert pairs.sum() == int(a['part'].sum()) ** 2 and (safe | ~pairs).mean() > 0.9
            # where the neighbours are the same, the fp32 sum is the float64 one to the bound of a recursive sum of n terms, each product rounded once
            keep = ~(differ.any(1))
            budget = (b['nbr'] + 1) * 2.0 ** -24 * np.where(b['near'], np.abs(b['h'])[None, :], 0.0).sum(1) * 1.01
            assert (np.abs(a['patch'].astype(np.float64) - b['patch']) <= budget)[keep].all()


def test_bad_arguments_are_refused_before_any_launch():
    """Every ValueError of the two wrappers and of the sampler's forms on CPU tensors (so nothing has touched a device), the refusal of a CPU tensor once
    everything else is valid, and ABOPT_EINVAL of the two C entries on dummy pointers that are never dereferenced."""
    assert hip.check_run_min('x', 0) == 0 and hip.check_run_min('x', 2) == 2 and hip.check_run_min('x', 16.0) == 16
    for bad in (1, -1, 17, 2.5, True):
        with pytest.raises(ValueError, match='run_min'):
            hip.check_run_min('run_min', bad)
    seqs = torch.zeros(6, 9, dtype=torch.int64)
    with pytest.raises(ValueError, match='run_min'):
        hip.sequence_liabilities_grouped(seqs, 3, run_min=1)
    with pytest.raises(ValueError, match='whole groups'):
        hip.sequence_liabilities_grouped(seqs, 4)
    with pytest.raises(ValueError, match='whole groups'):
        hip.sequence_liabilities_grouped(seqs.float(), 3)
    with pytest.raises(ValueError, match=r'rows \(6, 9\) must be \(G, n\)'):
        hip.sequence_liabilities_grouped(seqs, 3, rows=torch.ones(6, 9, dtype=torch.bool))
    with pytest.raises(ValueError, match=r'link \(2, 8\) must be \(G, n\)'):
        hip.sequence_liabilities_grouped(seqs, 3, link=torch.ones(2, 8, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='HIP device only'):
        hip.sequence_liabilities_grouped(seqs, 3, rows=torch.ones(2, 9, dtype=torch.bool))
    with pytest.raises(ValueError, match=r'expected \(S, n\)'):
        sampler.sequence_liabilities(seqs[0])
    with pytest.raises(ValueError, match=r'rows \(2, 9\) must be \(n,\)'):
        sampler.sequence_liabilities(seqs, rows=torch.ones(2, 9, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='HIP device only'):
        sampler.sequence_liabilities(seqs)

    pos, mask, group = torch.zeros(4, 6, 5, 3), torch.ones(4, 6, 5, dtype=torch.bool), torch.ones(2, 6, dtype=torch.int32)
    area, sq = torch.ones(4, 6), torch.zeros(4, 6, dtype=torch.uint8)
    call = hip.surface_patches_grouped
    with pytest.raises(ValueError, match='whole groups'):
        call(pos[:3], mask[:3], group, area[:3], sq[:3])
    with pytest.raises(ValueError, match='1 .. 15'):
        call(torch.zeros(4, 6, 16, 3), torch.ones(4, 6, 16, dtype=torch.bool), group, area, sq)
    with pytest.raises(ValueError, match='slot 1 is CA'):
        call(pos[:, :, :1], mask[:, :, :1], group, area, sq)
    with pytest.raises(ValueError, match='neither per candidate nor per group'):
        call(pos, mask[:3], group, area, sq)
    with pytest.raises(ValueError, match='area'):
        call(pos, mask, group, area[:2], sq)
    with pytest.raises(ValueError, match='area'):
        call(pos, mask, group, area.long(), sq)
    with pytest.raises(ValueError, match='seqs'):
        call(pos, mask, group, area, sq[:3])
    with pytest.raises(ValueError, match='seqs'):
        call(pos, mask, group, area, sq.float())
    with pytest.raises(ValueError, match='weight'):
        call(pos, mask, group, area, sq, weight=torch.zeros(20))
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='radius'):
            call(pos, mask, group, area, sq, radius=bad)
    with pytest.raises(RuntimeError, match='HIP device only'):                          # everything valid: the CPU tensor is refused before anything is allocated
        call(pos, mask, group, area, sq[:2])
    batch = dict(fragment_type=torch.ones(2, 6, dtype=torch.long), generate_flag=torch.zeros(2, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match='rows'):
        sampler.developability(batch, sq, pos, mask, rows='designed')

    L_ = hip.lib()
    dummy = (ctypes.c_char * 16)()
    a = ctypes.c_void_p(ctypes.addressof(dummy))
    liab_c = lambda G=2, S=3, n=9, run_min=5, seqs=a, flags=a, counts=a: L_.abopt_sequence_liabilities_grouped(seqs, None, None, run_min, G, S, n, flags, counts, None, None)
    for kw, word in ((dict(run_min=1), 'run_min'), (dict(run_min=17), 'run_min'), (dict(run_min=-2), 'run_min'), (dict(S=0), 'bad dims'), (dict(n=0), 'bad dims'),
                     (dict(G=-1), 'bad dims'), (dict(G=2, S=32768, n=32768), 'bad dims'), (dict(G=65536, S=1, n=1), '65535'), (dict(seqs=None), 'NULL'),
                     (dict(flags=None), 'NULL'), (dict(counts=None), 'NULL')):
        assert liab_c(**kw) == 1 and word in L_.abopt_last_error().decode(), (kw, L_.abopt_last_error().decode())
    assert liab_c(G=0) == 0 and liab_c(G=0, seqs=None) == 0                            # a no-op
    patch_c = lambda G=2, S=3, L=9, A=5, radius=10.0, pos=a, nbr=a: L_.abopt_surface_patches_grouped(pos, a, 0, a, a, a, 0, a, radius, G, S, L, A, a, nbr, None)
    for kw, word in ((dict(A=1), 'CA'), (dict(A=16), '16'), (dict(L=0), 'bad dims'), (dict(G=-1), 'bad dims'), (dict(S=-1), 'bad dims'), (dict(radius=-1.0), 'radius'),
                     (dict(radius=float('nan')), 'radius'), (dict(radius=float('inf')), 'radius'), (dict(G=65536, S=1), '65535'), (dict(pos=None), 'NULL'),
                     (dict(nbr=None), 'NULL')):
        assert patch_c(**kw) == 1 and word in L_.abopt_last_error().decode(), (kw, L_.abopt_last_error().decode())
    assert patch_c(G=0) == 0 and patch_c(S=0) == 0 and patch_c(G=0, pos=None) == 0     # no-ops, between the value checks and the pointer checks
    assert patch_c(G=0, radius=-1.0) == 1


def test_names_and_hydropathy_table():
    assert model.LIABILITY_NAMES == ('n_glyc', 'deamidation', 'isomerisation', 'cleavage', 'cys', 'met', 'hydrophobic_run') == st.NAMES
    tenths = [18, 25, -35, -35, 28, -4, -32, 45, -39, 38, 19, -35, -16, -35, -45, -8, -7, 42, -9, -13]
    assert list(model.KD_HYDROPATHY_TENTHS) == tenths and model.AA_LETTERS == st.AA
    assert list(model.KD_HYDROPATHY) == [t / 10.0 for t in tenths]
    assert dict(zip(model.AA_LETTERS, model.KD_HYDROPATHY))['I'] == 4.5 and dict(zip(model.AA_LETTERS, model.KD_HYDROPATHY))['R'] == -4.5
    w = hip.default_patch_weight()
    assert w.dtype == torch.float32 and w.shape == (21,) and not w.is_cuda and hip.default_patch_weight() is w
    assert np.array_equal(w.numpy(), np.array([t / 10.0 for t in tenths] + [0.0]).astype(np.float32)) and np.array_equal(w.numpy(), st.default_weight())


# ------------------------------------------------------------------------------------------ GPU: the liabilities
@pytest.mark.gpu
def test_liabilities_equal_the_statement():
    """flags, counts, hyd10 and freq as integers against liabilities_np over the whole table: the group layouts, the 64-position marks and the 256-position tile of
    the kernel (n = 257), every run_min, rows and link each NULL and given; and without freq the same flags and counts."""
    assert_every_rule_is_reached()                                                      # on the statement, before any device call
    for case in LIAB_CASES:
        G, S, n, run_min, _, _ = case
        c = liab(*case)
        _assert_liabilities(_run_liab(c, S, run_min), c['want'], case)
        got = _run_liab(c, S, run_min, want_freq=False)
        assert 'freq' not in got
        _assert_liabilities(got, c['want'], case, freq=False)
    c = liab(2, 5, 130, 16, False, True)                                                # any integer dtype, values outside 0 .. 255 saturate to "no type"
    wide = torch.from_numpy(c['seqs'].astype(np.int64)).to(DEV)
    wide = torch.where(wide == 255, 100000, wide)
    got = hip.sequence_liabilities_grouped(wide, 5, link=torch.from_numpy(c['link']).to(DEV), run_min=16, want_freq=True)
    _assert_liabilities(got, c['want'], 'int64 sequences')
    empty = hip.sequence_liabilities_grouped(wide[:0], 5, want_freq=True)
    assert empty['flags'].shape == (0, 130) and empty['counts'].shape == (0, 12) and empty['hyd10'].shape == (0,) and empty['freq'].shape == (0, 130)


@pytest.mark.gpu
def test_sequence_liabilities_summary():
    """sampler.sequence_liabilities: the single-group form with the named counts, net_charge and gravy (one float64 division; NaN where nothing is scored)."""
    c = liab(1, 1, 130, 5, True, True)
    seqs = np.concatenate([c['seqs'], liab(1, 1, 130, 5, True, True)['seqs'][:, ::-1]])
    rows, link = c['rows'][0], c['link'][0]
    want = st.liabilities_np(seqs, rows, link, 5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    got = sampler.sequence_liabilities(t(seqs).long(), rows=t(rows), link=t(link), run_min=5)
    assert np.array_equal(got['flags'].cpu().numpy(), want['flags'])
    for k, name in enumerate(model.LIABILITY_NAMES):
        assert got[name].cpu().tolist() == want['counts'][:, k].tolist(), name
    for name, col in (('flagged', 7), ('positive', 8), ('negative', 9), ('his', 10), ('scored', 11)):
        assert got[name].cpu().tolist() == want['counts'][:, col].tolist(), name
    assert got['hyd10'].cpu().tolist() == want['hyd10'].tolist()
    assert got['net_charge'].cpu().tolist() == (want['counts'][:, 8] - want['counts'][:, 9]).tolist()
    assert got['gravy'].dtype == torch.float64 and got['gravy'].cpu().tolist() == (want['hyd10'] / (10.0 * want['counts'][:, 11])).tolist()
    none = sampler.sequence_liabilities(t(seqs), rows=torch.zeros(130, dtype=torch.bool, device=DEV))
    assert torch.isnan(none['gravy']).all() and not none['flags'].any() and not none['scored'].any()


# ------------------------------------------------------------------------------------------ GPU: the patches
@pytest.mark.gpu
@pytest.mark.parametrize('G,S,L,A', PATCH_CASES)
def test_patches_equal_the_float32_statement(G, S, L, A):
    """patch on its int32 view and nbr as integers against patches_f32, at every radius; with the sequences shared by a group; with a custom weight table that
    holds a NaN entry."""
    t = patch_inputs(G, S, L, A)
    if L >= 63:                                                                         # a condition on the inputs: neither nobody nor everybody is a neighbour
        share = patch_want(G, S, L, A, 10.0)[2]
        print(f'{share:.3f} of the participating pairs are neighbours at 10 A')
        assert 0.05 <= share <= 0.95, share
    for radius in RADII:
        _assert_patches(hip.surface_patches_grouped(radius=radius, **t), patch_want(G, S, L, A, radius), (G, S, L, A, radius))
    shared = dict(t, seqs=t['seqs'][::S].contiguous())
    _assert_patches(hip.surface_patches_grouped(radius=10.0, **shared), patch_want(G, S, L, A, 10.0, shared=True), 'shared sequences')
    w = torch.from_numpy(custom_weight())
    for radius in (4.5, 10.0):
        _assert_patches(hip.surface_patches_grouped(radius=radius, weight=w, **t), patch_want(G, S, L, A, radius, custom=True), ('custom weight', radius))
    if L >= 63:
        want = patch_want(G, S, L, A, 10.0)
        assert (want[1] == 0).any() and (want[1] > 1).any() and (want[0] < 0).any() and (want[0] > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize('G,S,L,A', FAR_CASES)
def test_patches_far_from_the_origin(G, S, L, A):
    """The same inputs rotated and moved by (900, -700, 500) A: the statement is recomputed on the moved fp32 coordinates and met bit for bit."""
    t = patch_inputs(G, S, L, A, far=True)
    assert float(t['pos'][torch.isfinite(t['pos'])].abs().max()) > 600
    for radius in (4.5, 10.0):
        _assert_patches(hip.surface_patches_grouped(radius=radius, **t), patch_want(G, S, L, A, radius, far=True), (G, S, L, A, radius))


@pytest.mark.gpu
def test_shared_mask_and_shared_sequences_equal_expanded():
    G, S, L, A = 2, 5, 65, 5
    t = patch_inputs(G, S, L, A)
    mask, seqs = t['mask'][::S].contiguous(), t['seqs'][::S].contiguous()               # the first candidate's, for the whole group
    a = hip.surface_patches_grouped(t['pos'], mask, t['group'], t['area'], seqs)
    b = hip.surface_patches_grouped(t['pos'], mask.repeat_interleave(S, 0), t['group'], t['area'], seqs.repeat_interleave(S, 0))
    harness.assert_same_results(_bits(a), _bits(b), 'shared against expanded')
    s = st.structure(G, S, L, A)
    _assert_patches(a, st.patches_grouped_f32(s['pos'], s['mask'][::S], s['group'], s['area'], s['seqs'][::S], st.default_weight(), 10.0, S), 'shared mask and sequences')


@pytest.mark.gpu
def test_many_candidates():
    """1100 candidates of L = 48 (more workgroups than one row of the grid's slices: every candidate is one wave) of ten distinct structures, and one candidate of
    L = 300, cut into five units of 64 targets over five slices."""
    G, S, L, A, reps = 2, 5, 48, 5, 110
    s = st.structure(G, S, L, A)
    rep = lambda a: torch.from_numpy(a).to(DEV).view(G, 1, S, *a.shape[1:]).expand(G, reps, S, *a.shape[1:]).reshape(G * reps * S, *a.shape[1:])
    got = hip.surface_patches_grouped(rep(s['pos']), rep(s['mask']), torch.from_numpy(s['group']).to(DEV), rep(s['area']), rep(s['seqs']))
    idx = (np.arange(G)[:, None, None] * S + np.arange(S)[None, None, :] + np.zeros((1, reps, 1), dtype=np.int64)).reshape(-1)
    want = patch_want(G, S, L, A, 10.0)
    _assert_patches(got, (want[0][idx], want[1][idx]), 'many candidates')
    _assert_patches(hip.surface_patches_grouped(**patch_inputs(1, 1, 300, 5)), patch_want(1, 1, 300, 5, 10.0), 'one candidate of 300 residues')
    many = liab(2, 5, 130, 16, False, True)                                             # ... and 1100 designs through the liabilities
    seqs = torch.from_numpy(many['seqs']).to(DEV).view(2, 1, 5, 130).expand(2, reps, 5, 130).reshape(-1, 130)
    got = hip.sequence_liabilities_grouped(seqs, 5 * reps, link=torch.from_numpy(many['link']).to(DEV), run_min=16, want_freq=True)
    assert np.array_equal(got['flags'].cpu().numpy(), many['want']['flags'][idx]) and np.array_equal(got['counts'].cpu().numpy(), many['want']['counts'][idx])
    assert np.array_equal(got['freq'].cpu().numpy(), many['want']['freq'] * reps)


# ------------------------------------------------------------------------------------------ GPU: the properties of a call
def _liab_call(S, run_min):
    return lambda seqs, rows, link: hip.sequence_liabilities_grouped(seqs, S, rows=rows, link=link, run_min=run_min, want_freq=True)


def _liab_tensors(c):
    return {k: None if c[k] is None else torch.from_numpy(c[k]).to(DEV) for k in ('seqs', 'rows', 'link')}


@pytest.mark.gpu
def test_grouped_call_equals_per_group_calls():
    G, S, L, A = 3, 2, 63, 5
    harness.grouped_equals_per_group(lambda **t: _bits(hip.surface_patches_grouped(**t)), [('patches', G, S, patch_inputs(G, S, L, A))], {'group'})
    cases = [(case, case[0], case[1], _liab_tensors(liab(*case))) for case in ((3, 2, 257, 5, True, True), (2, 5, 65, 16, True, True), (3, 2, 65, 5, True, False))]
    for case, G, S, t in cases:
        harness.grouped_equals_per_group(_liab_call(S, case[3]), [(case, G, S, t)], {'rows', 'link', 'freq'})


@pytest.mark.gpu
def test_call_is_capturable():
    """Each call recorded with torch.cuda.graph (one launch, no memset node) and replayed on OTHER inputs copied into the static tensors gives what the eager call
    gives on them."""
    G, S, L, A = 2, 5, 65, 5
    t = patch_inputs(G, S, L, A)
    o = st.structure(G, S, L, A, seed=1)
    first, held = harness.capture_replays_on_other_inputs(lambda **t: _bits(hip.surface_patches_grouped(**t)), t, {k: torch.from_numpy(o[k]).to(DEV) for k in t})
    _assert_patches(dict(patch=first['patch'].view(torch.float32), nbr=first['nbr']), patch_want(G, S, L, A, 10.0), 'replay on the captured inputs')
    assert not torch.equal(held['nbr'], first['nbr']), 'the other inputs give other neighbours'
    case = (2, 5, 257, 2, True, True)
    c, other = liab(*case), st.liability_case(*case, seed=1)
    first, held = harness.capture_replays_on_other_inputs(_liab_call(5, case[3]), _liab_tensors(c), {k: torch.from_numpy(other[k]).to(DEV) for k in ('seqs', 'rows', 'link')})
    _assert_liabilities(first, c['want'], 'replay on the captured inputs')
    assert not torch.equal(held['flags'], first['flags']), 'the other inputs give other flags'


@pytest.mark.gpu
def test_repeat_calls_are_bit_identical():
    t = patch_inputs(1, 1, 300, 5)
    first = _bits(hip.surface_patches_grouped(**t))
    c = _liab_tensors(liab(3, 2, 257, 5, True, True))
    first_l = _liab_call(2, 5)(**c)
    for _ in range(5):
        harness.assert_same_results(_bits(hip.surface_patches_grouped(**t)), first, 'patches')
        harness.assert_same_results(_liab_call(2, 5)(**c), first_l, 'liabilities')


# ------------------------------------------------------------------------------------------ GPU: the chain
@pytest.mark.gpu
def test_developability_equals_the_composition_of_public_calls():
    """sampler.developability on the screen's complex, three candidates with their own sequences and with a shared one, rows in all three forms: every field is
    what the three public calls give, and the summaries are what plain torch makes of them."""
    one = screen_workers.complex_(DEV)
    L, A = one['pos_heavyatom'].shape[1:3]
    S = 3
    gen = torch.Generator(device=DEV).manual_seed(5)
    pos = one['pos_heavyatom'].expand(S, L, A, 3) + 0.3 * torch.randn(S, L, A, 3, generator=gen, device=DEV)
    mask = one['mask_heavyatom']
    flag = one['generate_flag'].bool()
    own = torch.where(flag, torch.randint(0, 20, (S, L), generator=gen, device=DEV), one['aa'].expand(S, L))
    grp = screen.chain_groups(one['fragment_type'])
    link = sampler.backbone_links(one['chain_nb'], one['res_nb'])
    some = torch.zeros_like(flag)
    some[:, ::3] = True
    for seqs in (own, one['aa']):
        for rows, scored in (('generated', flag), ('antibody', grp == 1), (some, some)):
            got = sampler.developability(one, seqs, pos, mask, rows=rows, points=96, radius=8.0, run_min=4)
            sa = hip.sasa_grouped(pos, mask, grp, sampler.slot_radii(A), probe=1.4, points=96)
            free = sa['area'][..., 0].contiguous()
            pt = hip.surface_patches_grouped(pos, mask, grp, free, seqs, radius=8.0)
            lb = hip.sequence_liabilities_grouped(seqs, seqs.shape[0], rows=scored, link=link, run_min=4)
            assert torch.equal(got['pts'], sa['pts']) and torch.equal(got['area'], sa['area'])
            assert torch.equal(got['patch_res'].view(torch.int32), pt['patch'].view(torch.int32)) and torch.equal(got['nbr'], pt['nbr'])
            assert torch.equal(got['flags'], lb['flags']) and torch.equal(got['hyd10'], lb['hyd10']) and got['flags'].shape == (seqs.shape[0], L)
            for k, name in enumerate(model.LIABILITY_NAMES):
                assert torch.equal(got[name], lb['counts'][:, k])
            assert torch.equal(got['net_charge'], lb['counts'][:, 8] - lb['counts'][:, 9])
            part = pt['nbr'] > 0
            assert part.any() and torch.equal(part.any(-1), got['patch_argmax'] >= 0)
            p64 = pt['patch'].double()
            assert torch.equal(got['sap'], p64.clamp_min(0).sum(-1).float())
            for c in range(S):
                vals = pt['patch'][c][part[c]]
                assert got['patch_max'][c] == vals.max() and got['patch_argmax'][c] == int(part[c].nonzero()[(vals == vals.max()).nonzero()[0, 0], 0])
            w = hip.default_patch_weight(DEV)[seqs.long().clamp(0, 20)].expand(S, L)
            side1 = (grp == 1).expand(S, L)
            assert torch.equal(got['apolar_area'], torch.where(side1 & (w > 0), free.double(), 0.0).sum(-1).float())
            assert torch.equal(got['polar_area'], torch.where(side1 & (w <= 0), free.double(), 0.0).sum(-1).float())
            assert torch.allclose(got['apolar_area'] + got['polar_area'], torch.where(side1, free, 0.0).sum(-1), rtol=1e-5)
            assert (got['sap'] > 0).all() and (got['apolar_area'] > 0).all()
    with pytest.raises(ValueError, match='rows'):
        sampler.developability(one, own, pos, mask, rows='designed')
