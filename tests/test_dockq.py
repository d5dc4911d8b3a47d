"""DockQ scoring (abopt_dockq_lite / abopt_dockq_lite_grouped, csrc/dockq.hip; hip.dockq_lite / hip.dockq_lite_grouped) against oracle/dockq.py::dockq in float64
on the fp32 values the device gets, at the edges of the kernels: L around the 64 lanes of a wave and the 256 threads of a workgroup (every per-residue loop strides
by 256), both receptor choices and the tie, masks per candidate, all 15 atom slots under a random mask, interleaved chains, an empty interface, far from the
origin, a dirty workspace, many candidates, a captured call.  The inputs and the conditions they satisfy are tests/dockq_cases.py.

The bounds (`_assert_values`):
  fnat   exact: np.float32(nat_correct / nat_total), the same double division followed by one rounding; exactly 0 where nat_total = 0.
  irms,  |got - ref| <= 2^-23 ref + 1e-6 A.  The kernel accumulates centroids, covariance, the Jacobi eigenvector and the residuals in double from the fp32
  Lrms   inputs; under condition (b) of dockq_cases that error stays below 1e-10 A even at 1000 A coordinates with a 100 A lever arm.  What remains is the one
         rounding of the result to fp32, 2^-24 relative; the bound doubles it, and the floor covers values near zero.
  DockQ  |got - ref| <= 1e-6.  The slope of 1 / (1 + (x / 1.5)^2) peaks at 0.433 at 0.87 A, where the irms bound is 1.1e-6; the 8.5 A term adds less than a
         fifth of that; divided by 3, plus one fp32 rounding of 6e-8.
  -1     exactly where the statement has an empty selection (dockq() raises or returns NaN there; dockq_cases.dockq_from_tables maps that to -1 and
         test_tables_helper_equals_the_statement holds the two together)."""
import warnings

import numpy as np
import pytest
import torch

import dockq_cases as dc
import scorer_harness as harness
from oracle import dockq as odq

DEV = torch.device('cuda:0')
FIELDS = ('fnat', 'irms', 'Lrms', 'DockQ')
NAMES = ('model_pos', 'model_mask', 'native_pos', 'native_mask', 'group')
PER_NATIVE = {'native_pos', 'native_mask', 'group'}
WORST = {}                                                          # field -> the worst error / bound seen by this process, printed by every value test


# ------------------------------------------------------------------------------------------ CPU: the inputs and the statement
@pytest.mark.parametrize('name', list(dc.SPECS))
def test_case_conditions_hold(name):
    """(a) the 5 / 10 A margin, (b) the eigen-gap of every compared fit, (c) the case's claim -- near the origin and, where the case has one, on its far copy."""
    c = dc.case(name)
    sp = dc.SPECS[name]
    assert dc.conditions(c) == []
    assert c['model_pos'].dtype == np.float32 and c['model_pos'].shape == (sp['G'] * sp['S'], sp['L'], sp['A'], 3) and c['native_pos'].dtype == np.float32
    assert c['margin'] > dc.MARGIN and (name == 'two_residues' or c['gap'] > dc.GAP)
    if 'far' in c:
        assert c['far']['margin'] > dc.MARGIN and c['far']['gap'] > dc.GAP and np.abs(c['far']['native_pos'][c['native_mask']]).min() > 600.0
    print(name, 'seed', c['seed'], 'after', c['seeds_tried'], 'others; margin %.2e A, eigen-gap %.2e' % (c['margin'], c['gap']))


def test_tables_helper_equals_the_statement():
    """dockq_cases.dockq_from_tables, which takes the native's tables ready-made, equals oracle/dockq.py::dockq field for field on every candidate of
    per_candidate_masks and two_residues; on empty_interface, where the helper reports -1, dockq() raises or returns NaN."""
    for name in ('per_candidate_masks', 'two_residues'):
        c = dc.case(name)
        for k, r in enumerate(c['ref']):
            g = k // c['S']
            mm = c['model_mask'][k if c['per_candidate'] else g]
            want = odq.dockq(c['model_pos'][k], mm, c['native_pos'][g], c['native_mask'][g], c['group'][g])
            for f in ('fnat', 'nat_correct', 'nat_total', 'irms', 'Lrms', 'DockQ', 'n_interface'):
                assert r[f] == want[f], (name, k, f, r[f], want[f])
            assert np.array_equal(r['interface'], want['interface']), (name, k)
    c = dc.case('empty_interface')
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        try:
            irms = odq.dockq(c['model_pos'][0], c['model_mask'][0], c['native_pos'][0], c['native_mask'][0], c['group'][0])['irms']
        except (np.linalg.LinAlgError, ValueError, FloatingPointError):
            irms = float('nan')
    assert np.isnan(irms) and c['ref'][0]['irms'] == -1.0 and c['ref'][0]['DockQ'] == -1.0


def test_a_one_atom_fit_is_a_translation_in_the_statement():
    """two_residues: the receptor has one CA, so its covariance is exactly zero and nothing determines a rotation; the statement (numpy's SVD of the zero
    matrix) takes the identity, which is what the device's Jacobi solver does on a zero matrix.  Lrms is then the ligand's displacement less the receptor's."""
    c = dc.case('two_residues')
    x, grp = c['native_pos'][0][:, odq.CA].astype(np.float64), c['group'][0]
    for k, r in enumerate(c['ref']):
        y = c['model_pos'][k][:, odq.CA].astype(np.float64)
        rec, lig = np.nonzero(grp == r['rec'])[0][0], np.nonzero(grp == 3 - r['rec'])[0][0]
        assert abs(r['Lrms'] - np.linalg.norm((y[lig] - y[rec]) - (x[lig] - x[rec]))) < 1e-12, k


# ------------------------------------------------------------------------------------------ CPU: the wrappers' shape contract
_Z = lambda *s: torch.zeros(*s)
_M = lambda *s: torch.ones(*s, dtype=torch.bool)
_GOOD = dict(model_pos=_Z(4, 6, 4, 3), model_mask=_M(4, 6, 4), native_pos=_Z(2, 6, 4, 3), native_mask=_M(2, 6, 4), group=torch.ones(2, 6, dtype=torch.int32))
_N = 'dockq_lite_grouped'
GROUPED_REFUSALS = [
    (dict(group=_GOOD['group'][0]), f'{_N}: expected pos (G*S, L, A, 3), mask (G*S or G, L, A) and group (G, L), got (4, 6, 4, 3), (4, 6, 4) and (6,)'),
    (dict(model_mask=_M(6, 4)), f'{_N}: expected pos (G*S, L, A, 3), mask (G*S or G, L, A) and group (G, L), got (4, 6, 4, 3), (6, 4) and (2, 6)'),
    (dict(group=_GOOD['group'][:, :5]), f'{_N}: (4, 6, 4, 3) candidates are not whole groups of the 2 rows of group (2, 5)'),
    (dict(group=torch.ones(3, 6, dtype=torch.int32)), f'{_N}: (4, 6, 4, 3) candidates are not whole groups of the 3 rows of group (3, 6)'),
    (dict(model_pos=_Z(4, 6, 4, 2)), f'{_N}: (4, 6, 4, 2) candidates are not whole groups of the 2 rows of group (2, 6)'),
    (dict(model_mask=_M(3, 6, 4)), f'{_N}: mask (3, 6, 4) is neither per candidate nor per group'),
    (dict(model_mask=_M(4, 6, 5)), f'{_N}: mask (4, 6, 5) is neither per candidate nor per group'),
    (dict(native_pos=_Z(1, 6, 4, 3)), f'{_N}: native_pos (1, 6, 4, 3) and native_mask (2, 6, 4) are not (G, L, A, 3) and (G, L, A) with G >= 1 for the (G, L, A) = (2, 6, 4) '
                                      'of the candidates and group'),
    (dict(native_pos=_Z(2, 7, 4, 3)), f'{_N}: native_pos (2, 7, 4, 3) and native_mask (2, 6, 4) are not (G, L, A, 3) and (G, L, A) with G >= 1 for the (G, L, A) = (2, 6, 4) '
                                      'of the candidates and group'),
    (dict(native_pos=_Z(2, 6, 4)), f'{_N}: native_pos (2, 6, 4) and native_mask (2, 6, 4) are not (G, L, A, 3) and (G, L, A) with G >= 1 for the (G, L, A) = (2, 6, 4) '
                                   'of the candidates and group'),
    (dict(native_mask=_M(2, 6, 5)), f'{_N}: native_pos (2, 6, 4, 3) and native_mask (2, 6, 5) are not (G, L, A, 3) and (G, L, A) with G >= 1 for the (G, L, A) = (2, 6, 4) '
                                    'of the candidates and group'),
    (dict(native_mask=_M(6, 4)), f'{_N}: native_pos (2, 6, 4, 3) and native_mask (6, 4) are not (G, L, A, 3) and (G, L, A) with G >= 1 for the (G, L, A) = (2, 6, 4) '
                                 'of the candidates and group'),
    (dict(model_pos=_Z(0, 6, 4, 3), model_mask=_M(0, 6, 4), native_pos=_Z(0, 6, 4, 3), native_mask=_M(0, 6, 4), group=torch.ones(0, 6, dtype=torch.int32)),
     f'{_N}: native_pos (0, 6, 4, 3) and native_mask (0, 6, 4) are not (G, L, A, 3) and (G, L, A) with G >= 1 for the (G, L, A) = (0, 6, 4) of the candidates and group'),
    (dict(model_pos=_Z(4, 6, 1, 3), model_mask=_M(4, 6, 1), native_pos=_Z(2, 6, 1, 3), native_mask=_M(2, 6, 1)),
     f'{_N}: A=1 atoms per residue, expected 2 .. 15 (the CA is atom slot 1)'),
    (dict(model_pos=_Z(4, 6, 16, 3), model_mask=_M(4, 6, 16), native_pos=_Z(2, 6, 16, 3), native_mask=_M(2, 6, 16)), f'{_N}: A=16 atoms per residue, expected 1 .. 15'),
]
_P = 'dockq_lite'
_PGOOD = dict(model_pos=_Z(4, 6, 4, 3), model_mask=_M(4, 6, 4), native_pos=_Z(6, 4, 3), native_mask=_M(6, 4), group=torch.ones(6, dtype=torch.int32))
_DIMS = f'{_P}: expected model_pos (S, L, A, 3), model_mask (S, L, A) or (L, A), native_pos (L, A, 3), native_mask (L, A) and group (L,), got '
PLAIN_REFUSALS = [
    (dict(group=torch.ones(1, 6, dtype=torch.int32)), _DIMS + '(4, 6, 4, 3), (4, 6, 4), (6, 4, 3), (6, 4) and (1, 6)'),
    (dict(native_pos=_Z(1, 6, 4, 3)), _DIMS + '(4, 6, 4, 3), (4, 6, 4), (1, 6, 4, 3), (6, 4) and (6,)'),
    (dict(native_mask=_M(1, 6, 4)), _DIMS + '(4, 6, 4, 3), (4, 6, 4), (6, 4, 3), (1, 6, 4) and (6,)'),
    (dict(model_mask=_M(6)), _DIMS + '(4, 6, 4, 3), (6,), (6, 4, 3), (6, 4) and (6,)'),
    (dict(model_pos=_Z(6, 4, 3)), _DIMS + '(6, 4, 3), (4, 6, 4), (6, 4, 3), (6, 4) and (6,)'),
    (dict(group=torch.ones(5, dtype=torch.int32)), f'{_P}: model_pos (4, 6, 4, 3) is not (S, L, A, 3) with the L = 5 of group (5,)'),
    (dict(model_pos=_Z(4, 6, 4, 2)), f'{_P}: model_pos (4, 6, 4, 2) is not (S, L, A, 3) with the L = 6 of group (6,)'),
    (dict(model_mask=_M(3, 6, 4)), f'{_P}: model_mask (3, 6, 4) is neither per candidate (4, 6, 4) nor shared (6, 4)'),
    (dict(model_mask=_M(1, 6, 4)), f'{_P}: model_mask (1, 6, 4) is neither per candidate (4, 6, 4) nor shared (6, 4)'),
    (dict(model_mask=_M(5, 4)), f'{_P}: model_mask (5, 4) is neither per candidate (4, 6, 4) nor shared (6, 4)'),
    (dict(model_mask=_M(4, 6, 5)), f'{_P}: model_mask (4, 6, 5) is neither per candidate (4, 6, 4) nor shared (6, 4)'),
    (dict(native_pos=_Z(7, 4, 3)), f'{_P}: native_pos (7, 4, 3) and native_mask (6, 4) are not (6, 4, 3) and (6, 4)'),
    (dict(native_pos=_Z(6, 4, 2)), f'{_P}: native_pos (6, 4, 2) and native_mask (6, 4) are not (6, 4, 3) and (6, 4)'),
    (dict(native_mask=_M(6, 5)), f'{_P}: native_pos (6, 4, 3) and native_mask (6, 5) are not (6, 4, 3) and (6, 4)'),
    (dict(model_pos=_Z(4, 6, 16, 3), model_mask=_M(6, 16), native_pos=_Z(6, 16, 3), native_mask=_M(6, 16)), f'{_P}: A=16 atoms per residue, expected 2 .. 15 (the CA is atom slot 1)'),
    (dict(model_pos=_Z(4, 6, 1, 3), model_mask=_M(6, 1), native_pos=_Z(6, 1, 3), native_mask=_M(6, 1)), f'{_P}: A=1 atoms per residue, expected 2 .. 15 (the CA is atom slot 1)'),
]


@pytest.mark.parametrize('kw,text', GROUPED_REFUSALS)
def test_grouped_wrapper_refusal_texts(kw, text):
    """hip.dockq_lite_grouped refuses a wrong shape of any of its five tensors with ValueError before any device call: the tensors live on the CPU."""
    from ab_opt_amd import hip
    with pytest.raises(ValueError) as e:
        hip.dockq_lite_grouped(check=False, **dict(_GOOD, **kw))
    assert str(e.value) == text


@pytest.mark.parametrize('kw,text', PLAIN_REFUSALS)
def test_plain_wrapper_refusal_texts(kw, text):
    """hip.dockq_lite: the same contract with G = 1, every shape named as it was given; a (1, L, A) mask with S > 1 is not taken as shared."""
    from ab_opt_amd import hip
    with pytest.raises(ValueError) as e:
        hip.dockq_lite(check=False, **dict(_PGOOD, **kw))
    assert str(e.value) == text


def test_wrappers_accepted_shapes():
    """What the shape check returns for the accepted forms, and that those reach the binding (which has no CPU path)."""
    from ab_opt_amd import hip
    a = lambda **kw: hip._dockq_args('f', *[dict(_GOOD, **kw)[k] for k in NAMES])
    assert a() == (2, 2, 6, 4, False)
    assert a(model_mask=_M(2, 6, 4)) == (2, 2, 6, 4, True)                                                   # one mask per native
    assert a(model_pos=_Z(2, 6, 4, 3), model_mask=_M(2, 6, 4)) == (2, 1, 6, 4, True)                          # S = 1
    assert a(model_pos=_Z(0, 6, 4, 3), model_mask=_M(0, 6, 4)) == (2, 0, 6, 4, False)                         # no candidates
    two = dict(model_pos=_Z(4, 6, 2, 3), model_mask=_M(4, 6, 2), native_pos=_Z(2, 6, 2, 3), native_mask=_M(2, 6, 2))
    assert a(**two) == (2, 2, 6, 2, False)                                                                   # A = 2: the CA is the last slot
    for call, good in ((hip.dockq_lite_grouped, _GOOD), (hip.dockq_lite, _PGOOD), (hip.dockq_lite, dict(_PGOOD, model_mask=_M(6, 4))),
                       (hip.dockq_lite, dict(_PGOOD, model_pos=_Z(1, 6, 4, 3), model_mask=_M(1, 6, 4))), (hip.dockq_lite, dict(_PGOOD, model_pos=_Z(0, 6, 4, 3), model_mask=_M(0, 6, 4)))):
        with pytest.raises(RuntimeError, match='HIP device only'):
            call(**good)


# ------------------------------------------------------------------------------------------ GPU
def _dev(c):
    return dict(zip(NAMES, harness.dev(c, *NAMES)))


def _grouped(**t):
    from ab_opt_amd import hip
    return dict(out=hip.dockq_lite_grouped(t['model_pos'], t['model_mask'], t['native_pos'], t['native_mask'], t['group'], check=False))


def _plain(g=0, **t):
    """hip.dockq_lite on native g of the grouped tensors t and its candidates (the mask per candidate, or the native's own row of a shared one)"""
    from ab_opt_amd import hip
    G = t['native_pos'].shape[0]
    S = t['model_pos'].shape[0] // G
    sl = slice(g * S, (g + 1) * S)
    mm = t['model_mask'][g] if t['model_mask'].shape[0] == G and S > 1 else t['model_mask'][sl]
    return dict(out=hip.dockq_lite(t['model_pos'][sl], mm, t['native_pos'][g], t['native_mask'][g], t['group'][g], check=False))


def _assert_values(out, c, tag):
    """out (G*S, 4) against the statement c['ref'] under the bounds of the module docstring; prints every figure before it asserts"""
    got = out.cpu().numpy()
    assert got.shape == (c['G'] * c['S'], 4) and got.dtype == np.float32, tag
    for k, r in enumerate(c['ref']):
        want_fnat = np.float32(r['nat_correct'] / r['nat_total']) if r['nat_total'] else np.float32(0.0)
        line = [f'{tag} candidate {k}:']
        ok = got[k, 0] == want_fnat
        WORST['fnat'] = max(WORST.get('fnat', 0.0), float(got[k, 0] != want_fnat))
        for j, f in ((1, 'irms'), (2, 'Lrms'), (3, 'DockQ')):
            if r[f] < 0:
                ok &= got[k, j] == -1.0
                line.append(f'{f} {got[k, j]} (none)')
                continue
            err = abs(float(got[k, j]) - r[f])
            bound = 1e-6 if f == 'DockQ' else 2.0 ** -23 * r[f] + 1e-6
            WORST[f] = max(WORST.get(f, 0.0), err / bound)
            ok &= err <= bound
            line.append(f'{f} {got[k, j]:.7g} ref {r[f]:.9g} err/bound {err / bound:.3f}')
        print(' '.join(line), f'fnat {got[k, 0]} ref {r["nat_correct"]}/{r["nat_total"]}')
        assert ok, (tag, k, got[k].tolist(), [r[f] for f in FIELDS])
    print('worst error / bound so far:', {f: round(v, 3) for f, v in WORST.items()})


@pytest.mark.gpu
@pytest.mark.parametrize('name', dc.VALUE_CASES)
def test_values_match_the_float64_statement(name):
    """Every case through hip.dockq_lite_grouped and, per native, through hip.dockq_lite (bit-identical to the grouped rows): fnat exactly, irms / Lrms / DockQ
    within the bounds of the module docstring, -1 exactly where the statement has an empty selection."""
    c = dc.case(name)
    t = _dev(c)
    out = _grouped(**t)['out']
    _assert_values(out, c, name)
    for g in range(c['G']):
        assert torch.equal(_plain(g, **t)['out'], out[g * c['S']:(g + 1) * c['S']]), (name, g)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['long_interleaved', 'all_atoms'])
def test_values_far_from_the_origin(name):
    """Natives and candidates alike translated by (900, -700, 1100) A in float64 and rounded to fp32: conditions (a) and (b) hold again on the rounded values
    (dockq_cases.conditions covers the far copy), and the same three bounds hold against the statement on those values."""
    c = dc.case(name)
    assert dc.conditions(c) == []
    far = c['far']
    assert far['margin'] > dc.MARGIN and far['gap'] > dc.GAP
    t = _dev(far)
    out = _grouped(**t)['out']
    _assert_values(out, far, name + ' far')
    for g in range(c['G']):
        assert torch.equal(_plain(g, **t)['out'], out[g * c['S']:(g + 1) * c['S']]), (name, g)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['block_257', 'long_interleaved'])
def test_a_dirty_workspace_changes_nothing(name):
    """The shared workspace filled with 0xff before each of the two entries: the results equal those on a zeroed workspace, and the statement.  This pins the
    clears the entries make themselves (interface flags and the contact counter of every native)."""
    from ab_opt_amd import hip
    c = dc.case(name)
    t = _dev(c)
    for call in (_grouped, _plain):
        call(**t)                                                   # sizes the workspace of this stream
        ws = hip.Workspace.get(1, DEV)
        ws.fill_(0)
        clean = call(**t)['out'].clone()
        ws.fill_(0xff)
        dirty = call(**t)['out']
        assert hip.Workspace.get(1, DEV) is ws
        assert torch.equal(dirty, clean), (name, call.__name__)
    _assert_values(_grouped(**t)['out'], c, name + ' after a dirty workspace')


@pytest.mark.gpu
def test_many_candidates():
    """Seven distinct candidates (L = 8, A = 2) tiled to S = 70 000 through the plain entry, and seven natives x S = 10 000 through the grouped one: every row
    equals the row of the seven-candidate call."""
    c = dc.case('many')
    t = _dev(c)
    G, S = c['G'], c['S']
    small = _grouped(**t)['out']
    _assert_values(small, c, 'many')
    idx = torch.arange(70000, device=DEV) % S
    big = _plain(0, **dict(t, model_pos=t['model_pos'][idx], native_pos=t['native_pos'][:1], native_mask=t['native_mask'][:1], group=t['group'][:1],
                           model_mask=t['model_mask'][:1]))['out']
    assert big.shape == (70000, 4) and torch.equal(big, small[idx])
    idx = (torch.arange(G, device=DEV)[:, None] * S + torch.arange(10000, device=DEV)[None] % S).reshape(-1)
    big = _grouped(**dict(t, model_pos=t['model_pos'][idx]))['out']
    assert big.shape == (70000, 4) and torch.equal(big, small[idx])


def _mask_forms(name):
    """(tag, G, S, tensors, per_group) of a case with its model mask per candidate and shared per native"""
    c = dc.case(name)
    t = _dev(c)
    G, S = c['G'], c['S']
    per_cand = t['model_mask'] if c['per_candidate'] else t['model_mask'].repeat_interleave(S, 0)
    return [((name, 'per candidate'), G, S, dict(t, model_mask=per_cand), PER_NATIVE),
            ((name, 'per native'), G, S, dict(t, model_mask=t['native_mask']), PER_NATIVE | {'model_mask'})]


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['long_interleaved', 'per_candidate_masks'])
def test_grouped_call_equals_per_group_calls(name):
    """G natives in one call against G single-native calls of the grouped entry and of the plain one, torch.equal, for a mask per candidate and a mask per native;
    and a mask shared per native gives the bits of the same mask expanded per candidate."""
    forms = _mask_forms(name)
    for tag, G, S, t, per_group in forms:
        harness.grouped_equals_per_group(_grouped, [(tag, G, S, t)], per_group)
        whole = _grouped(**t)['out']
        for g in range(G):
            assert torch.equal(_plain(g, **t)['out'], whole[g * S:(g + 1) * S]), (tag, g)
    tag, G, S, t, _ = forms[1]
    expanded = dict(t, model_mask=t['model_mask'].repeat_interleave(S, 0))
    assert torch.equal(_grouped(**expanded)['out'], _grouped(**t)['out'])
    for g in range(G):
        assert torch.equal(_plain(g, **expanded)['out'], _plain(g, **t)['out']), g


@pytest.mark.gpu
def test_calls_are_capturable():
    """Each entry recorded with torch.cuda.graph and replayed gives the statement's values; replayed on OTHER candidate coordinates of the same shape, copied
    into the static input without a synchronisation, it gives what the eager call gives on them.  hip.Workspace is keyed by stream, so the recorded call
    allocates a workspace of its own under the capture stream's key, from the graph's pool: hip.Workspace.private lets it go again with the graph."""
    from ab_opt_amd import hip
    for name, call in (('per_candidate_masks', _grouped), ('wave_65', _plain)):
        c = dc.case(name)
        t = _dev(c)
        other = dict(model_pos=torch.roll(t['model_pos'], 1, 0).contiguous())
        with hip.Workspace.private():
            first, held = harness.capture_replays_on_other_inputs(call, t, other)
            torch.cuda.synchronize()
        _assert_values(first['out'], c, name + ' replayed')
        assert not torch.equal(first['out'], held['out'])


@pytest.mark.gpu
def test_repeat_calls_are_bit_identical():
    for name in ('block_257', 'per_candidate_masks'):
        t = _dev(dc.case(name))
        for call in (_grouped, _plain):
            runs = [call(**t)['out'].clone() for _ in range(5)]
            assert all(torch.equal(r, runs[0]) for r in runs[1:]), (name, call.__name__)


@pytest.mark.gpu
def test_bad_arguments_are_refused_by_the_c_entries_before_any_launch():
    """S < 0, L < 1, A < 2, a NULL pointer, L = 46341 (L * L > INT_MAX, on both entries) and G = 65536 (grouped): ABOPT_EINVAL; a short workspace:
    ABOPT_EWORKSPACE; `out` keeps the pattern it was filled with.  The pointers are small real buffers, and none of these calls reaches a launch."""
    from ab_opt_amd import hip
    L_ = hip.lib()
    c = dc.case('two_residues')
    t = _dev(c)
    G, S, L, A = 1, c['S'], c['L'], c['A']
    out = torch.full((S, 4), 77.0, device=DEV)
    need, need_g = L_.abopt_dockq_workspace_bytes(L), L_.abopt_dockq_grouped_workspace_bytes(G, L)
    assert need == L * L + L + 256 and need_g == G * L * L + G * L + 64 + 4 * G + 64
    ws = torch.zeros(max(need, need_g), dtype=torch.uint8, device=DEV)
    ptrs = dict(model_pos=hip.ptr(t['model_pos']), model_mask=hip.ptr(t['model_mask']), native_pos=hip.ptr(t['native_pos']), native_mask=hip.ptr(t['native_mask']),
                group=hip.ptr(t['group']), out=hip.ptr(out), ws=hip.ptr(ws))

    def plain(S=S, L=L, A=A, ws_bytes=need, **null):
        p = dict(ptrs, **null)
        return L_.abopt_dockq_lite(p['model_pos'], p['model_mask'], 1, p['native_pos'], p['native_mask'], p['group'], S, L, A, p['out'], p['ws'], ws_bytes, hip.stream())

    def grouped(G=G, S=S, L=L, A=A, ws_bytes=need_g, **null):
        p = dict(ptrs, **null)
        return L_.abopt_dockq_lite_grouped(p['model_pos'], p['model_mask'], 1, p['native_pos'], p['native_mask'], p['group'], G, S, L, A, p['out'], p['ws'], ws_bytes,
                                           hip.stream())
    for call in (plain, grouped):
        assert call(S=-1) == 1 and call(L=0) == 1 and call(A=1) == 1, call.__name__
        assert 'bad dims' in L_.abopt_last_error().decode()
        for name in ptrs:
            assert call(**{name: None}) == 1 and 'NULL' in L_.abopt_last_error().decode(), (call.__name__, name)
        assert call(L=46341) == 1 and 'L=46341' in L_.abopt_last_error().decode(), call.__name__
        assert call(L=46340, ws_bytes=need) == 4, call.__name__                 # the largest L that passes the check stops at its workspace
        assert call(S=0) == 0, call.__name__                                    # no candidates: a no-op
    assert plain(ws_bytes=need - 1) == 4 and 'workspace too small' in L_.abopt_last_error().decode()
    assert grouped(ws_bytes=need_g - 1) == 4 and 'workspace too small' in L_.abopt_last_error().decode()
    assert grouped(G=65536, S=1) == 1 and '65536' in L_.abopt_last_error().decode()
    assert grouped(G=-1) == 1 and grouped(G=0) == 0
    torch.cuda.synchronize()
    assert (out == 77.0).all()
    assert plain() == 0                                                         # ... and a good call fills the same buffer with the statement's values
    torch.cuda.synchronize()
    _assert_values(out, c, 'two_residues through the C entry')
    out.fill_(77.0)
    assert grouped() == 0
    torch.cuda.synchronize()
    _assert_values(out, c, 'two_residues through the grouped C entry')
