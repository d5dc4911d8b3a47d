"""Inputs of tests/test_dockq.py and the conditions they satisfy; numpy only, importable without a device.

The definition of every number is oracle/dockq.py::dockq (float64), evaluated on the float32 values the device gets.  `native_tables` / `dockq_from_tables` are
that function with the native's contact tables and the model's residue distances computed once and handed in (the distances also serve condition (a)), and with
the empty selections, where dockq() raises or returns NaN, mapped to the device's -1 markers; tests/test_dockq.py holds them equal to dockq() field for field.

A structure is two CA random walks (3.8 A steps) whose centroids lie `gap` A apart, with the other atom slots scattered around each CA; the native is rounded to
3 decimals; the candidates are the side-1 residues moved rigidly by growing amounts plus jitter, rounded likewise; everything is float32.  The residues are then
permuted, so the chains are interleaved, and a few have group 0.  Per-atom masks are random, with one CA missing on each side.

Conditions, asserted where a case is built (`case` searches seeds until they hold; they are conditions on the inputs, not on the code):
  (a) no residue pair with sides {1, 2} has a float64 minimum distance within 1e-4 A of 5 A or 10 A, in the native or in any candidate, under the mask that
      applies.  The device's fp32 d2 has one rounding in each difference and at most three more in the sum of squares, under 5 x 2^-24 relative: under 2e-6 A
      at 10 A, a fiftieth of the margin.
  (b) every superposition that is compared is well-conditioned: the two largest eigenvalues of the 4x4 key matrix of the fit (float64) differ by more than
      1e-3 of the largest.  A fit of fewer than three atoms cannot satisfy this (the roll about a line, or everything about a point, is free); only the case
      `two_residues` has such fits, and there the compared numbers do not depend on the free part: an RMSD over the fitted atoms themselves depends on the
      eigenvalue alone, and a one-atom fit has an exactly zero covariance in float64 on both sides, for which the statement (numpy's SVD of the zero matrix) and
      the device (Jacobi on the zero matrix) both take the identity rotation -- tests/test_dockq.py pins the statement's side of that.
  (c) what a case claims to exercise (CLAIMS) holds."""
import functools

import numpy as np

from oracle import dockq as odq

CA = odq.CA
FAR = np.array([900.0, -700.0, 1100.0])
MARGIN = 1e-4           # (a), Angstrom
GAP = 1e-3              # (b), relative

# name -> dict(G, S, L, A, builder options: sizes = residues of side 1, side 2 and group 0).  block_258 is one more than the block edges need: only from there on
# can residues >= 256 lie on both sides.  `many` feeds the many-candidates test.
SPECS = {
    'two_residues': dict(G=1, S=2, L=2, A=2, sizes=(1, 1, 0), gap=4.0),
    'wave_63': dict(G=1, S=3, L=63, A=5),
    'wave_64': dict(G=1, S=3, L=64, A=5),
    'wave_65': dict(G=1, S=3, L=65, A=5),
    'block_255': dict(G=1, S=3, L=255, A=5),
    'block_256': dict(G=1, S=3, L=256, A=5),
    'block_257': dict(G=1, S=3, L=257, A=5),
    'block_258': dict(G=1, S=3, L=258, A=5),
    'long_interleaved': dict(G=3, S=4, L=300, A=5, sizes=(146, 142, 12), far=True),
    'all_atoms': dict(G=1, S=3, L=65, A=15, far=True, p_atom=0.7),
    'receptor_1': dict(G=1, S=3, L=65, A=5, sizes=(40, 22, 3)),
    'receptor_2': dict(G=1, S=3, L=65, A=5, sizes=(22, 40, 3)),
    'receptor_tie': dict(G=1, S=3, L=65, A=5, sizes=(31, 31, 3)),
    'per_candidate_masks': dict(G=2, S=4, L=65, A=5, sizes=(32, 30, 3), per_candidate=True),
    'empty_interface': dict(G=1, S=2, L=40, A=5, sizes=(19, 19, 2), apart=True),
    'native_itself': dict(G=1, S=1, L=65, A=5, identity=True),
    'many': dict(G=7, S=7, L=8, A=2, sizes=(4, 3, 1), gap=4.0),
}
WAVE_EDGES = ('wave_63', 'wave_64', 'wave_65')
BLOCK_EDGES = ('block_255', 'block_256', 'block_257', 'block_258')
VALUE_CASES = tuple(n for n in SPECS if n != 'many')


# ------------------------------------------------------------------------------------------ the statement, with the native's tables built once
def native_tables(native_pos, native_mask, group):
    """What dockq() computes from the native alone: the 5 A contacts, their number and the 10 A interface (and the residue distances behind them)."""
    g = np.asarray(group)
    md2 = odq.residue_min_dist2(native_pos, native_mask)
    pair = (g[:, None] == 1) & (g[None, :] == 2)
    nat10 = (md2 <= 100.0) & pair
    return dict(md2=md2, pair=pair, nat5=(md2 <= 25.0) & pair, interface=nat10.any(1) | nat10.any(0))


def key_matrix_gap(x, y):
    """(lambda_1 - lambda_2) / lambda_1 of the 4x4 key matrix of the fit of y onto x (float64); 0 for fewer than three atoms or a vanishing matrix."""
    if len(x) < 3:
        return 0.0
    xc, yc = x - x.mean(0), y - y.mean(0)
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = yc.T @ xc
    K = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx], [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy], [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    w = np.linalg.eigvalsh(K)
    return float((w[3] - w[2]) / w[3]) if w[3] > 0 else 0.0


def dockq_from_tables(model_pos, model_mask, native_pos, native_mask, group, tab, model_md2=None):
    """dockq() of ONE model with the native's tables `tab` handed in -> its fields, with irms / Lrms / DockQ = -1 where a selection is empty (dockq() raises or
    returns NaN there: the interface, the receptor or the ligand has no CA present in both), and what the conditions and claims need on top: n1, n2, rec, the
    eigen-gaps of the two fits, the LRMS with the roles of receptor and ligand swapped, and the model's residue distances."""
    group = np.asarray(group)
    md2 = odq.residue_min_dist2(model_pos, model_mask) if model_md2 is None else model_md2
    nat_total = int(tab['nat5'].sum())
    nat_correct = int((tab['nat5'] & (md2 <= 25.0)).sum())
    fnat = nat_correct / nat_total if nat_total else 0.0
    both_ca = model_mask[:, CA] & native_mask[:, CA] & (group > 0)
    sel = tab['interface'] & both_ca
    x, y = np.asarray(native_pos, np.float64)[:, CA], np.asarray(model_pos, np.float64)[:, CA]
    n1, n2 = int((both_ca & (group == 1)).sum()), int((both_ca & (group == 2)).sum())
    rec, lig = (1, 2) if n1 > n2 else (2, 1)
    rsel, lsel = both_ca & (group == rec), both_ca & (group == lig)

    def ligand_rms(fit, ev):
        R, t = odq.kabsch(x[fit], y[fit])
        return float(np.sqrt((((y[ev] @ R.T + t) - x[ev]) ** 2).sum(-1).mean()))
    irms = odq.rmsd_after_fit(x[sel], y[sel]) if sel.any() else -1.0
    defined = rsel.any() and lsel.any()
    Lrms = ligand_rms(rsel, lsel) if defined else -1.0
    score = (fnat + 1 / (1 + (irms / 1.5) ** 2) + 1 / (1 + (Lrms / 8.5) ** 2)) / 3 if irms >= 0 and Lrms >= 0 else -1.0
    return dict(fnat=fnat, nat_correct=nat_correct, nat_total=nat_total, irms=irms, Lrms=Lrms, DockQ=score, interface=tab['interface'], n_interface=int(sel.sum()),
                n1=n1, n2=n2, rec=rec, gap_irms=key_matrix_gap(x[sel], y[sel]), gap_lrms=key_matrix_gap(x[rsel], y[rsel]),
                Lrms_swapped=ligand_rms(lsel, rsel) if defined else -1.0, md2=md2)


def cutoff_margin(md2, pair):
    """the distance (A) of the nearest residue pair with sides {1, 2} to the 5 A or the 10 A cutoff"""
    d = np.sqrt(md2[pair & np.isfinite(md2)])
    return float(min(np.abs(d - 5.0).min(), np.abs(d - 10.0).min())) if d.size else np.inf


# ------------------------------------------------------------------------------------------ the builder
def _rotation(axis, angle):
    a = axis / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _walk(rng, n):
    step = rng.normal(size=(n, 3))
    step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
    ca = np.cumsum(step, 0)
    return ca - ca.mean(0)


def _one_native(rng, S, L, A, sizes, gap, apart, identity, per_candidate, p_atom):
    """one native and its S candidates -> (native_pos, native_mask, group, model_pos [S], model_mask [S] or None: the native's)"""
    n1, n2, n0 = sizes
    w1, w2, w0 = _walk(rng, n1), _walk(rng, n2), rng.normal(size=(n0, 3)) * 12.0
    if apart:                                                        # nothing of side 2 within 30 A of side 1, whatever the atoms and the motion add
        gap = np.abs(w1).max() + np.abs(w2).max() + 60.0
    ca = np.concatenate([w1, w2 + np.array([gap, 0.0, 0.0]), w0])
    side = np.concatenate([np.full(n1, 1), np.full(n2, 2), np.zeros(n0, int)])
    pos = ca[:, None, :] + rng.normal(size=(L, A, 3)) * 1.5
    pos[:, CA] = ca
    mask = rng.random((L, A)) < p_atom
    mask[:, CA] = True
    for s in (1, 2):                                                 # a missing CA on each side
        if (side == s).sum() >= 4:
            mask[rng.choice(np.nonzero(side == s)[0]), CA] = False
    perm = rng.permutation(L)                                        # interleaved chains
    pos, mask, side = pos[perm], mask[perm], side[perm]
    native = np.round(pos, 3).astype(np.float32)
    one = side == 1
    cen = native[one][:, CA].astype(np.float64).mean(0)
    models, masks = [], []
    for k in range(S):
        m = native.astype(np.float64)
        if not identity:
            amount = k + 1
            R = _rotation(rng.normal(size=3), 0.05 * amount)
            m[one] = (m[one] - cen) @ R.T + cen + rng.normal(size=3) * 0.6 * amount + rng.normal(size=m[one].shape) * 0.08 * amount
        models.append(np.round(m, 3).astype(np.float32))
        if per_candidate:
            mm = rng.random((L, A)) < p_atom
            mm[:, CA] = True
            masks.append(mm)
    return native, mask, side.astype(np.int32), np.stack(models), np.stack(masks) if per_candidate else None


def _per_candidate_cas(rng, S, native_mask, group, interface, model_mask):
    """The CA atoms the candidates of one native lack (per_candidate_masks): candidate 1 lacks three of side 1 -- which turns its receptor choice --, every other
    one lacks one of side 2; all taken from the native's interface residues where there are enough, so the interface selection shrinks too."""
    for k in range(S):
        s, n = (1, 3) if k == 1 else (2, 1)
        pool = np.nonzero((group == s) & native_mask[:, CA] & interface)[0]
        if pool.size < n:
            pool = np.nonzero((group == s) & native_mask[:, CA])[0]
        model_mask[k, rng.choice(pool, n, replace=False), CA] = False


def _evaluate(c):
    """the statement on every candidate of case dict c (in place): ref = the list of dockq_from_tables results, margin (a), gap (b)"""
    G, S = c['G'], c['S']
    c['ref'], margin, gap = [], np.inf, np.inf
    for g in range(G):
        tab = native_tables(c['native_pos'][g], c['native_mask'][g], c['group'][g])
        margin = min(margin, cutoff_margin(tab['md2'], tab['pair']))
        for k in range(g * S, (g + 1) * S):
            mm = c['model_mask'][k if c['per_candidate'] else g]
            r = dockq_from_tables(c['model_pos'][k], mm, c['native_pos'][g], c['native_mask'][g], c['group'][g], tab)
            margin = min(margin, cutoff_margin(r.pop('md2'), tab['pair']))
            gap = min([gap] + [r[f] for f, v in (('gap_irms', r['irms']), ('gap_lrms', r['Lrms'])) if v >= 0])
            c['ref'].append(r)
    c['margin'], c['gap'] = margin, gap
    return c


def far_from_origin(c):
    """case c with natives and candidates alike translated by FAR in float64 and rounded to fp32, and the statement evaluated on those values"""
    f = dict(c)
    for k in ('native_pos', 'model_pos'):
        f[k] = (c[k].astype(np.float64) + FAR).astype(np.float32)
    return _evaluate(f)


def build(name, seed):
    """-> the case dict of SPECS[name] from `seed`: G, S, L, A, native_pos (G,L,A,3) fp32, native_mask (G,L,A) bool, group (G,L) int32, model_pos (G*S,L,A,3) fp32,
    model_mask (G*S,L,A) with per_candidate or (G,L,A) = native_mask, ref, margin, gap [, far: the same case far from the origin]"""
    sp = SPECS[name]
    G, S, L, A = sp['G'], sp['S'], sp['L'], sp['A']
    n0 = min(3, L // 16)
    sizes = sp.get('sizes', ((L - n0 + 1) // 2, (L - n0) // 2, n0))
    assert sum(sizes) == L
    rng = np.random.default_rng([seed, L, A])
    per_candidate = sp.get('per_candidate', False)
    parts = [_one_native(rng, S, L, A, sizes, sp.get('gap', 6.0), sp.get('apart', False), sp.get('identity', False), per_candidate, sp.get('p_atom', 0.85))
             for _ in range(G)]
    if per_candidate:
        for npos, nmask, grp, _, mm in parts:
            _per_candidate_cas(rng, S, nmask, grp, native_tables(npos, nmask, grp)['interface'], mm)
    c = dict(name=name, seed=seed, G=G, S=S, L=L, A=A, per_candidate=per_candidate, native_pos=np.stack([p[0] for p in parts]),
             native_mask=np.stack([p[1] for p in parts]), group=np.stack([p[2] for p in parts]), model_pos=np.concatenate([p[3] for p in parts]))
    c['model_mask'] = np.concatenate([p[4] for p in parts]) if per_candidate else c['native_mask']
    _evaluate(c)
    if sp.get('far'):
        c['far'] = far_from_origin(c)
    return c


# ------------------------------------------------------------------------------------------ the conditions
def conditions(c):
    """-> the list of conditions (a), (b), (c) that case c breaks (empty: all hold)"""
    name, G, S, L = c['name'], c['G'], c['S'], c['L']
    ref, grp = c['ref'], c['group']
    bad = []
    for tag, v in (('', c), ('far ', c.get('far'))):
        if v is None:
            continue
        if not v['margin'] > MARGIN:
            bad.append(f'(a) {tag}margin {v["margin"]:.2e} A')
        if name != 'two_residues' and not v['gap'] > GAP:
            bad.append(f'(b) {tag}eigen-gap {v["gap"]:.2e}')
    claim = lambda ok, text: None if ok else bad.append('(c) ' + text)
    iface = lambda r, g, k: bool(ref[g * S + k]['interface'][r] and c['native_mask'][g, r, CA] and c['model_mask'][(g * S + k) if c['per_candidate'] else g, r, CA])
    if name not in ('empty_interface', 'two_residues'):
        claim(all(r['nat_total'] > 0 and r['irms'] >= 0 and r['Lrms'] >= 0 for r in ref), 'an interface and both selections in every candidate')
    if name not in ('empty_interface', 'two_residues', 'native_itself', 'many'):
        claim(any(0 < r['nat_correct'] < r['nat_total'] for r in ref), 'a candidate with some but not all native contacts')
    if name == 'two_residues':
        claim(all(r['n1'] == 1 and r['n2'] == 1 and r['nat_total'] == 1 and r['n_interface'] == 2 for r in ref), 'one residue per side, in contact')
    def other_receptor_below_256(g):                                # the common-CA counts of residues < 256 alone would choose the other receptor
        both = c['model_mask'][g, :256, CA] & c['native_mask'][g, :256, CA]
        n1, n2 = int((both & (grp[g, :256] == 1)).sum()), int((both & (grp[g, :256] == 2)).sum())
        return (1 if n1 > n2 else 2) != ref[g * S]['rec']
    if name == 'block_257':
        claim(other_receptor_below_256(0), 'residue 256 decides the receptor')
    if name == 'long_interleaved':
        claim(any(other_receptor_below_256(g) for g in range(G)), 'the residues >= 256 decide the receptor of a native')
    if name in ('block_257', 'block_258'):
        claim(all(iface(256, 0, k) for k in range(S)), 'residue 256 is a common-CA interface residue')
    if name == 'block_258':
        claim(all(iface(257, 0, k) for k in range(S)) and {int(grp[0, 256]), int(grp[0, 257])} == {1, 2}, 'residues 256 and 257 are interface residues of the two sides')
    if name == 'long_interleaved':
        for g in range(G):
            hi = np.arange(L) >= 256
            claim(all(any(iface(r, g, 0) for r in np.nonzero(hi & (grp[g] == s))[0]) for s in (1, 2)), f'native {g}: interface members of both sides at r >= 256')
            claim((grp[g][hi] == 0).any() and (grp[g][:256] == 0).any(), f'native {g}: group 0 on both sides of r = 256')
            claim((np.diff(grp[g]) != 0).sum() > L // 4, f'native {g}: interleaved chains')
    if name == 'all_atoms':
        m = c['native_mask'][0][grp[0] > 0]
        claim(m.any(0).all() and (~m).any(0).all(), 'every atom slot present somewhere and absent somewhere')
    if name.startswith('receptor_'):
        want = dict(receptor_1=lambda a, b: a > b, receptor_2=lambda a, b: a < b, receptor_tie=lambda a, b: a == b)[name]
        claim(all(want(r['n1'], r['n2']) for r in ref), 'the common-CA counts of the two sides')
        claim(all(abs(r['Lrms'] - r['Lrms_swapped']) > 0.1 for r in ref), 'the LRMS with the roles swapped differs by more than 0.1 A')
    if name == 'per_candidate_masks':
        fewer = smaller = False
        for g in range(G):
            tab = native_tables(c['native_pos'][g], c['native_mask'][g], grp[g])
            for k in range(g * S, (g + 1) * S):
                r = dockq_from_tables(c['model_pos'][k], c['native_mask'][g], c['native_pos'][g], c['native_mask'][g], grp[g], tab)      # under the native's mask
                fewer |= ref[k]['nat_correct'] < r['nat_correct']
                smaller |= ref[k]['n_interface'] < r['n_interface']
            claim(len({ref[k]['rec'] for k in range(g * S, (g + 1) * S)}) == 2, f'native {g}: a candidate with another receptor than its peers')
            claim(all((c['model_mask'][k] & ~c['native_mask'][g]).any() and (c['model_mask'][k] != c['model_mask'][g * S]).any() for k in range(g * S + 1, (g + 1) * S)),
                  f'native {g}: masks that differ per candidate, with atoms the native lacks')
        claim(fewer, 'a candidate with fewer correct contacts than under the native mask')
        claim(smaller, 'a candidate with a smaller interface selection than under the native mask')
    if name == 'empty_interface':
        claim(all(r['nat_total'] == 0 and r['fnat'] == 0.0 and r['irms'] == -1.0 and r['DockQ'] == -1.0 and r['Lrms'] > 0 and not r['interface'].any() for r in ref),
              'no contact, no interface, a defined Lrms')
    if name == 'native_itself':
        claim(np.array_equal(c['model_pos'][0], c['native_pos'][0]) and ref[0]['fnat'] == 1.0, 'the candidate is the native')
    return bad


# name -> the seed `case` starts from: the first one, counting up from 7, that passed when the cases were written (absent: 7 itself passed).  long_interleaved
# passed over 19 seeds, nearly all on (a): 3 natives x (1 + 4) structures x 2 placements of ~20 000 pairs each leave a pair within 1e-4 A of a cutoff more often
# than not.  block_258 passed over 8 on its claim (two given residues in the interface), receptor_2 and receptor_tie over 5 and 3 on the swapped-role margin.
SEED = dict(block_257=8, block_258=15, long_interleaved=26, all_atoms=8, receptor_2=12, receptor_tie=10, per_candidate_masks=8)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case `name`, built once per process and shared by the tests, which leave it unchanged: the first seed from SEED[name] on whose inputs satisfy the
    conditions.  c['seeds_tried'] says how many were passed over."""
    first = SEED.get(name, 7)
    for seed in range(first, first + 200):
        c = build(name, seed)
        bad = conditions(c)
        if not bad:
            break
    assert not bad, (name, bad)                                      # conditions on the inputs, not on the code
    c['seeds_tried'] = seed - first
    return c
