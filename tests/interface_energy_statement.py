"""The definition of the interface energy (include/abopt.h: abopt_interface_energy_grouped) restated in numpy, and the inputs of
tests/test_interface_energy.py.

`statement(..., dtype)` mirrors the definition step by step in the arithmetic `dtype` on the same fp32 inputs (the constants and knobs are the fp32 numbers the
device reads): np.float64 is the reference, np.float32 -- every step rounded once, in the association the header states, the additions in ascending j, donor
before acceptor -- is the yardstick the device has to EQUAL.  It also returns the per-pair energies, the margins of every exact test (for the condition on the
inputs under which the fp32 and float64 counts agree) and a tally of which rule was reached how often, so that a test can assert that its inputs reach every
term and every reason for skipping one."""
import functools

import numpy as np

AA = 'ACDEFGHIKLMNPQRSTVWY'
PRO = AA.index('P')
Q_HB, CLAMP, COULOMB = np.float32(27.888), np.float32(-9.9), np.float32(332.0637)
KNOBS = dict(hb_cutoff=-0.5, elec_cutoff=15.0, salt_cutoff=7.0, pair_cutoff=8.0, eps=4.0, d_min=3.0)
OTHER_KNOBS = dict(hb_cutoff=-1.0, elec_cutoff=12.0, salt_cutoff=5.0, pair_cutoff=6.5, eps=2.0, d_min=2.5)
SHIFT = (1000.0, -1000.0, 1000.0)
# the rules a set of inputs has to reach
RULES = ('hb/donor', 'hb/acceptor', 'hb/no_h_first', 'hb/no_h_unlinked', 'hb/no_h_proline', 'hb/no_h_atom', 'hb/no_acceptor_atom', 'hb/no_ca', 'hb/ca_far',
         'hb/close', 'hb/floor', 'hb/weak', 'pair/bonded', 'pair/same_side', 'centre/cb', 'centre/ca', 'centre/none', 'elec/counted', 'elec/salt', 'elec/like',
         'elec/not_salt', 'elec/beyond', 'elec/neutral', 'elec/nan_charge', 'elec/floor', 'table/counted', 'table/nan', 'table/beyond', 'table/byte20',
         'atom/masked', 'atom/not_finite', 'side/none')


def default_charge():
    return np.array([1.0 if c in 'KR' else -1.0 if c in 'DE' else 0.0 for c in AA] + [0.0], dtype=np.float32)


def hydrophobic_table():
    h = np.array([1.0 if c in 'FILMVWY' else 0.0 for c in AA] + [0.0], dtype=np.float32)
    return (0.0 - h[:, None] * h[None, :]).astype(np.float32)


def custom_tables():
    """a charge table with a NaN entry (E takes no part), a half charge on H and a charge for "no type"; an asymmetric pair table with NaN entries"""
    q = default_charge()
    q[AA.index('E')] = np.nan
    q[AA.index('H')] = 0.5
    q[20] = -0.25
    rng = np.random.default_rng(21)
    t = rng.normal(size=(21, 21)).astype(np.float32)
    t[rng.random((21, 21)) < 0.1] = np.nan
    t[3, 5], t[5, 3] = 1.5, -2.25
    return q, t


def _d2(a, b):
    """(dx dx + dy dy) + dz dz on the last axis, in this association"""
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def statement(pos, mask, group, seqs, link=None, charge=None, pair_table=None, knobs=None, dtype=np.float32):
    """The definition for ONE candidate in the arithmetic `dtype`: pos (L, A, 3) fp32, mask (L, A), group (L,), seqs (L,) bytes, link (L,) or None, charge (21,)
    or None (the default table), pair_table (21, 21) or None, knobs a dict (KNOBS where absent).
    -> dict(energy (L, 3) dtype, count (L, 5) int64; e_don (L, L): the DSSP energy of donor i and acceptor j where all its gates but the cutoff hold, else NaN;
    e_elec (L, L), e_pair (L, L): the terms added, else 0; margins: dict of arrays, see `condition`; tally: {rule: how often})."""
    dt = dtype
    kn = {k: dt(np.float32(v)) for k, v in dict(KNOBS, **(knobs or {})).items()}
    pos32 = np.asarray(pos, dtype=np.float32)
    mask, group = np.asarray(mask).astype(bool), np.asarray(group).astype(np.int64)
    L, A = mask.shape
    t = np.minimum(np.asarray(seqs).astype(np.int64), 20)
    charge = default_charge() if charge is None else np.asarray(charge, dtype=np.float32)
    linked = np.ones(L, bool) if link is None else np.asarray(link).astype(bool)
    tally = dict.fromkeys(RULES, 0)
    with np.errstate(all='ignore'):
        ok = mask & np.isfinite(pos32).all(-1)                                                  # the one rule of taking part
        x = pos32.astype(dt)
        on = (group == 1) | (group == 2)
        tally['atom/masked'] += int((~mask[on, :4]).sum())
        tally['atom/not_finite'] += int((mask & ~np.isfinite(pos32).all(-1))[on].sum())
        tally['side/none'] += int((~on).sum())
        n, ca, c, o = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
        has_cb = ok[:, 4] if A >= 5 else np.zeros(L, bool)
        centre = np.where(has_cb[:, None], x[:, 4] if A >= 5 else ca, ca)
        has_x = has_cb | ok[:, 1]
        for name, sel in (('centre/cb', has_cb), ('centre/ca', ~has_cb & ok[:, 1]), ('centre/none', ~has_x)):
            tally[name] += int((sel & on).sum())
        qraw = charge[t]
        q = np.where(np.isnan(qraw), np.float32(0), qraw).astype(dt)
        # the amide hydrogen
        prev = np.maximum(np.arange(L) - 1, 0)
        first = np.arange(L) == 0
        u = c[prev] - o[prev]
        length = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
        atoms = ok[:, 0] & ok[prev, 2] & ok[prev, 3]
        has_h = ~first & linked[prev] & (t != PRO) & atoms & (length > 0)
        h = n + u / length[:, None]
        for name, sel in (('hb/no_h_first', first), ('hb/no_h_unlinked', ~first & ~linked[prev]), ('hb/no_h_proline', ~first & linked[prev] & (t == PRO)),
                          ('hb/no_h_atom', ~first & linked[prev] & (t != PRO) & ~atoms)):
            tally[name] += int((sel & on).sum())
        # the pairs
        i, j = np.arange(L)[:, None], np.arange(L)[None, :]
        cross = on[:, None] & on[None, :] & (group[:, None] + group[None, :] == 3)
        bonded = ((j == i + 1) & linked[:, None]) | ((j == i - 1) & linked[None, :])
        pair = cross & ~bonded
        tally['pair/bonded'] += int((cross & bonded).sum())
        tally['pair/same_side'] += int((on[:, None] & on[None, :] & ~cross).sum())
        # 1. hydrogen bonds: donor i (rows), acceptor j (columns)
        d2ca = _d2(ca[:, None], ca[None, :])
        want = pair & has_h[:, None]
        acc_ok = (ok[:, 2] & ok[:, 3])[None, :]
        ca_ok = ok[:, 1][:, None] & ok[:, 1][None, :]
        gate = want & acc_ok & ca_ok & (d2ca < dt(81))
        tally['hb/no_acceptor_atom'] += int((want & ~acc_ok).sum())
        tally['hb/no_ca'] += int((want & acc_ok & ~ca_ok).sum())
        tally['hb/ca_far'] += int((want & acc_ok & ca_ok & ~(d2ca < dt(81))).sum())
        r_on, r_ch = np.sqrt(_d2(o[None, :], n[:, None])), np.sqrt(_d2(c[None, :], h[:, None]))
        r_oh, r_cn = np.sqrt(_d2(o[None, :], h[:, None])), np.sqrt(_d2(c[None, :], n[:, None]))
        one = dt(1)
        raw = dt(Q_HB) * (((one / r_on + one / r_ch) - one / r_oh) - one / r_cn)
        close = (r_on < dt(0.5)) | (r_ch < dt(0.5)) | (r_oh < dt(0.5)) | (r_cn < dt(0.5))
        e = np.where(close, dt(CLAMP), np.where(raw < dt(CLAMP), dt(CLAMP), raw))
        bond = gate & (e < kn['hb_cutoff'])
        tally['hb/close'] += int((gate & close).sum())
        tally['hb/floor'] += int((gate & ~close & (raw < dt(CLAMP))).sum())
        tally['hb/weak'] += int((gate & ~bond).sum())
        tally['hb/donor'] += int(bond.sum())
        tally['hb/acceptor'] += int(bond.T.sum())
        e_don = np.where(gate, e, np.nan)
        # 2. charges, 3. the pair table: on the centre distance
        d2x = _d2(centre[:, None], centre[None, :])
        both = pair & has_x[:, None] & has_x[None, :]
        charged = both & (q[:, None] != 0) & (q[None, :] != 0)
        elec = charged & (d2x <= kn['elec_cutoff'] * kn['elec_cutoff'])
        qq = q[:, None] * q[None, :]
        dmin2 = kn['d_min'] * kn['d_min']
        e_el = np.where(elec, (dt(COULOMB) * qq) / (kn['eps'] * np.maximum(d2x, dmin2)), dt(0))
        inside = elec & (d2x <= kn['salt_cutoff'] * kn['salt_cutoff'])
        salt, like = inside & (qq < 0), inside & (qq > 0)
        tally['elec/counted'] += int(elec.sum())
        tally['elec/salt'] += int(salt.sum())
        tally['elec/like'] += int(like.sum())
        tally['elec/not_salt'] += int((elec & ~inside).sum())
        tally['elec/beyond'] += int((charged & ~elec).sum())
        tally['elec/neutral'] += int((both & ~charged).sum())
        tally['elec/nan_charge'] += int((both & (np.isnan(qraw)[:, None] | np.isnan(qraw)[None, :])).sum())
        tally['elec/floor'] += int((elec & (d2x < dmin2)).sum())
        near = both & (d2x <= kn['pair_cutoff'] * kn['pair_cutoff'])
        if pair_table is not None:
            w = np.asarray(pair_table, dtype=np.float32)[t[:, None], t[None, :]]
            adds = near & ~np.isnan(w)
            e_pr = np.where(adds, w, np.float32(0)).astype(dt)
            tally['table/counted'] += int(adds.sum())
            tally['table/nan'] += int((near & np.isnan(w)).sum())
            tally['table/beyond'] += int((both & ~near).sum())
            tally['table/byte20'] += int((adds & ((np.asarray(seqs) >= 20)[:, None] | (np.asarray(seqs) >= 20)[None, :])).sum())
        else:
            adds, e_pr = np.zeros((L, L), bool), np.zeros((L, L), dt)
        # the sums: ascending j, donor before acceptor, from 0
        energy = np.zeros((L, 3), dt)
        for k in range(L):
            energy[:, 0] = np.where(bond[:, k], energy[:, 0] + e[:, k], energy[:, 0])
            energy[:, 0] = np.where(bond[k, :], energy[:, 0] + e[k, :], energy[:, 0])
            energy[:, 1] = np.where(elec[:, k], energy[:, 1] + e_el[:, k], energy[:, 1])
            energy[:, 2] = np.where(adds[:, k], energy[:, 2] + e_pr[:, k], energy[:, 2])
        count = np.stack([bond.sum(1), bond.sum(0), salt.sum(1), like.sum(1), near.sum(1)], 1).astype(np.int64)
        rel = lambda v, thr: np.abs(v / thr - 1)
        margins = dict(hb=np.abs(e_don - kn['hb_cutoff'])[gate], half=np.concatenate([rel(r[gate], dt(0.5)) for r in (r_on, r_ch, r_oh, r_cn)]),
                       ca=rel(d2ca, dt(81))[want & acc_ok & ca_ok], elec=rel(d2x, kn['elec_cutoff'] * kn['elec_cutoff'])[charged],
                       salt=rel(d2x, kn['salt_cutoff'] * kn['salt_cutoff'])[elec], pair=rel(d2x, kn['pair_cutoff'] * kn['pair_cutoff'])[both])
        # what the error bound of a pair reads (tests/test_interface_energy.py): the inverse distances of a gated pair
        inv = dict(on=one / r_on, ch=one / r_ch, oh=one / r_oh, cn=one / r_cn)
    return dict(energy=energy, count=count, e_don=e_don, bond=bond, e_elec=e_el, elec=elec, e_pair=e_pr, adds=adds, gate=gate, close=close, margins=margins,
                tally=tally, inv=inv)


def condition(ref):
    """The condition on the inputs, on the FLOAT64 statement `ref`: no bond energy within 1e-3 kcal/mol of hb_cutoff, no squared distance within 1e-4 relative of
    a squared cutoff or of 81, no hydrogen-bond distance within 1e-4 relative of 0.5 A.  -> the names of the margins that are violated (empty: it holds)."""
    limit = dict(hb=1e-3, half=1e-4, ca=1e-4, elec=1e-4, salt=1e-4, pair=1e-4)
    return [name for name, v in ref['margins'].items() if v.size and np.nanmin(v) < limit[name]]


def grouped(pos, mask, group, seqs, link, charge, pair_table, knobs, S, dtype=np.float32):
    """statement over G groups of S candidates: mask (G*S or G, L, A), seqs (G*S or G, L), link (G, L) or None -> (energy (G*S, L, 3), count (G*S, L, 5) int64,
    tally summed, the per-candidate results)."""
    N, L = pos.shape[:2]
    outs = []
    for c in range(N):
        g = c // S
        outs.append(statement(pos[c], mask[c] if mask.shape[0] == N else mask[g], group[g], seqs[c] if seqs.shape[0] == N else seqs[g],
                              None if link is None else link[g], charge, pair_table, knobs, dtype))
    tally = {r: sum(o['tally'][r] for o in outs) for r in RULES}
    return np.stack([o['energy'] for o in outs]), np.stack([o['count'] for o in outs]), tally, outs


# ------------------------------------------------------------------------------------------ inputs
LOCAL = np.array([[-0.525, 1.363, 0.0], [0.0, 0.0, 0.0], [1.526, 0.0, 0.0], [2.153, -1.062, 0.0], [-0.529, -0.774, -1.205]])       # N, CA, C, O, CB around CA


def _unit(v):
    return v / np.linalg.norm(v)


def _rotation(rng):
    q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    return q * np.sign(np.linalg.det(q))


def _place_acceptor(x, a, n_d, hdir, r_on, rng):
    """residue a with O at r_on from the donor's N along the H direction, C 1.23 A beyond it, the rest of the residue further out"""
    perp = _unit(np.cross(hdir, rng.normal(size=3)))
    x[a, 3] = n_d + r_on * hdir
    x[a, 2] = x[a, 3] + 1.23 * hdir
    x[a, 1] = x[a, 2] + 1.52 * _unit(hdir + 0.8 * perp)
    x[a, 0] = x[a, 1] + 1.46 * _unit(hdir - 0.8 * perp)
    if x.shape[1] >= 5:
        x[a, 4] = x[a, 1] + 1.53 * _unit(np.cross(hdir, perp) + 0.3 * hdir)


def candidate(L, A, group, link, seed, far):
    """One candidate: a compact CA walk of 3.8 A steps (the sides are interleaved along the row, so cross pairs are everywhere), every residue the ideal
    backbone + CB under a random rotation, further slots normal(1.5 A) around CA, types uniform with K, R, D, E, P at triple weight.  PLANTED on residues drawn
    without order (a later plant may overwrite an earlier one; the tests assert on the statement that every rule was reached): acceptors at 2.9 A (an ideal
    bond), 1.6 A (below -9.9 with every distance above 0.5 A) and 1.2 A (O within 0.5 A of H) from a donor's N; charge pairs K-D at 4 A and at 10 A, K-K at 5 A,
    R-E at 2 A (below d_min); residues without atoms, without CA, N, C, O or CB, with NaN and inf coordinates, the bytes 20, 21 and 255.
    -> (pos (L, A, 3) fp32, mask (L, A) bool, seqs (L,) uint8)."""
    rng = np.random.default_rng(seed)
    step = rng.normal(size=(L, 3))
    step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
    walk = np.cumsum(step, 0)
    walk *= 0.8                                                                                 # compact: neighbours in space are not neighbours in sequence
    x = np.zeros((L, A, 3))
    for r in range(L):
        x[r, :min(A, 5)] = walk[r] + LOCAL[:min(A, 5)] @ _rotation(rng).T
        if A > 5:
            x[r, 5:] = walk[r] + rng.normal(size=(A - 5, 3)) * 1.5
    p = np.ones(20)
    p[[AA.index(c) for c in 'KRDEP']] = 3.0
    seqs = rng.choice(20, size=L, p=p / p.sum()).astype(np.uint8)
    mask = np.ones((L, A), bool)
    side1, side2 = np.flatnonzero(group == 1), np.flatnonzero(group == 2)
    if len(side1) and len(side2):
        linked = np.ones(L, bool) if link is None else link
        donors = [r for r in rng.permutation(np.concatenate([side1, side2])) if r >= 1 and linked[r - 1]]
        used = set()
        for r_on, d in zip((2.9, 1.6, 1.2, 2.9, 3.1), donors):
            others = [a for a in rng.permutation(side2 if group[d] == 1 else side1) if a not in used and abs(a - d) > 1]
            if d in used or d - 1 in used or not others:
                continue
            a = others[0]
            used.update((d, d - 1, a))
            if seqs[d] == PRO:
                seqs[d] = AA.index('S')
            _place_acceptor(x, a, x[d, 0], _unit(x[d - 1, 2] - x[d - 1, 3]), r_on, rng)
        free1 = [r for r in rng.permutation(side1) if r not in used]
        free2 = [r for r in rng.permutation(side2) if r not in used]
        slot = 4 if A >= 5 else 1
        for (ti, tj, dist), i, j in zip((('K', 'D', 4.0), ('K', 'D', 10.0), ('K', 'K', 5.0), ('R', 'E', 2.0), ('D', 'R', 6.0)), free1, free2):
            if abs(i - j) <= 1:
                continue
            seqs[i], seqs[j] = AA.index(ti), AA.index(tj)
            x[j] += x[i, slot] + dist * _unit(rng.normal(size=3)) - x[j, slot]
            used.update((i, j))
    if far:
        x = x @ _rotation(np.random.default_rng(99)).T + np.array(SHIFT)
    pos = x.astype(np.float32)
    if L >= 7:
        r = rng.permutation(L)
        pick = lambda k: r[k % L]
        mask[pick(0)] = False
        for k, s in enumerate((1, 0, 2, 3)):
            mask[pick(1 + k), s] = False
        if A >= 5:
            mask[pick(5), 4] = False
        pos[pick(6), int(rng.integers(4)), int(rng.integers(3))] = np.nan
        pos[pick(7), min(4, A - 1), int(rng.integers(3))] = np.inf
        seqs[pick(8)], seqs[pick(9)], seqs[pick(10)] = 20, 21, 255
    return pos, mask, seqs


SEEDS = 64                                  # a candidate that violates the condition on the inputs is drawn again, from the next of this many seeds


@functools.lru_cache(maxsize=None)
def case(G, S, L, A, with_link=False, custom=False, far=False, other_knobs=False, seed=0):
    """G groups of S candidates, built once per key and treated as read-only.  group: the sides interleaved along the row in runs of one to three residues, one
    residue in nine on no side (from L = 7 on).  link: None, or a row with one step in twelve unlinked.  custom: the tables of `custom_tables`, else the default
    charges and no pair table.  Every candidate satisfies `condition` on its float64 statement: it is drawn again from the next seed until it does (at most
    SEEDS times; `redraws` says how often), none is dropped.
    -> dict(pos, mask, group, seqs, link, charge, pair_table, knobs, redraws, and the float64 statement of every candidate as ref)."""
    rng = np.random.default_rng(9000 * seed + 41 * L + 13 * A + 5 * G + S + 2 * with_link + 7 * custom)
    group = np.zeros((G, L), np.int32)
    for g in range(G):
        r, side = 0, 1 + int(rng.integers(2))
        while r < L:
            n = int(rng.integers(1, 4))
            group[g, r:r + n] = side
            r, side = r + n, 3 - side
        if L >= 7:
            group[g, rng.random(L) < 1 / 9] = rng.choice([0, 3, -1])
    link = (rng.random((G, L)) >= 1 / 12) if with_link else None
    charge, table = custom_tables() if custom else (None, None)
    knobs = dict(OTHER_KNOBS if other_knobs else KNOBS)
    key = (((((G * 8 + S) * 512 + L) * 16 + A) * 2 + with_link) * 2 + custom) * 8 + 4 * far + 2 * other_knobs + seed
    pos, mask, seqs, ref, redraws = [], [], [], [], 0
    for c in range(G * S):
        g = c // S
        for attempt in range(SEEDS):
            one = candidate(L, A, group[g], None if link is None else link[g], (key * 1000 + c) * SEEDS + attempt, far)
            r64 = statement(one[0], one[1], group[g], one[2], None if link is None else link[g], charge, table, knobs, np.float64)
            if not condition(r64):
                break
            redraws += 1
        else:
            raise AssertionError(f'no candidate of {SEEDS} satisfies the condition on the inputs: {(G, S, L, A, c)}')
        pos.append(one[0]); mask.append(one[1]); seqs.append(one[2]); ref.append(r64)
    return dict(pos=np.stack(pos), mask=np.stack(mask), group=group, seqs=np.stack(seqs), link=link, charge=charge, pair_table=table, knobs=knobs, redraws=redraws,
                ref=ref)
