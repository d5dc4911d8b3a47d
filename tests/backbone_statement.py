"""The definition of the backbone conformation (include/abopt.h: abopt_backbone_conformation_grouped) restated in numpy, and the inputs
of tests/test_backbone.py.

`statement(..., dtype)` mirrors the definition step by step in the arithmetic `dtype` on the same fp32 inputs: np.float64 is the reference, np.float32 -- every
step rounded once, every dot and cross product in the association the header states -- is the yardstick the device has to EQUAL.  It also returns the relation
hb, the margins of every exact test (for the condition on the inputs under which the fp32 and float64 integers agree) and a tally of which rule was reached
how often, so that a test can assert that its inputs reach every state, every pattern alternative and every reason for "undefined".

Random atoms hold no structure, so the inputs are PLANTED: a NeRF builder with ideal bond lengths and angles makes segments with chosen phi, psi, omega, bridges
are made by placing one residue's C=O along another's N-H, atom by atom, and the degenerate cases are written down coordinate by coordinate."""
import functools

import numpy as np

AA = 'ACDEFGHIKLMNPQRSTVWY'
PRO, GLY = AA.index('P'), AA.index('G')
SS_LETTERS = 'HEGITC'
RAMA_REGIONS = ((-160.0, -20.0, -120.0, 50.0), (-180.0, -45.0, 90.0, -170.0), (20.0, 120.0, -30.0, 100.0))
# eight boxes, for K = 8: the default three, then five that cut the rest of the plane -- every one holds a planted residue somewhere in the case table
EIGHT_REGIONS = RAMA_REGIONS + ((20.0, 120.0, 100.0, -100.0), (-180.0, -45.0, -170.0, -120.0), (-180.0, -45.0, 50.0, 90.0), (-20.0, 20.0, -180.0, -10.0),
                                (120.0, 180.0, -180.0, -10.0))
Q_HB, CLAMP = np.float32(27.888), np.float32(-9.9)
HB_CUTOFF, OTHER_CUTOFF = -0.5, -1.5
SHIFT = (1000.0, -1000.0, 1000.0)
MAX_ROWS = 512
HV = dict(phi=1, psi=2, omega=4, len=8, ang_c=16, ang_n=32)
SS = dict(h4=1, h3=2, h5=4, par=8, anti=16, turn=32)
COUNTS = ('part', 'phipsi') + tuple(f'region{k}' for k in range(8)) + ('outliers', 'outliers_gly', 'omega', 'cis', 'cis_nonpro', 'twisted', 'H', 'E', 'G', 'I',
                                                                        'T', 'C', 'hb_donor', 'hb_acceptor')
# the rules a set of inputs has to reach: every state and pattern alternative, every reason for "undefined", every gate of a bond, every count column
RULES = tuple(f'count/{c}' for c in COUNTS) + (
    'turn/3', 'turn/4', 'turn/5', 'turn/unlinked', 'helix/3', 'helix/4', 'helix/5', 'inside', 'bridge/par_a', 'bridge/par_b', 'bridge/anti_a', 'bridge/anti_b',
    'bridge/unlinked', 'bridge/too_near', 'bridge/partner_not_scored', 'phi/defined', 'phi/first', 'phi/unlinked', 'phi/no_atom', 'phi/rho0', 'psi/defined',
    'psi/unlinked', 'psi/no_atom', 'psi/rho0', 'omega/defined', 'omega/unlinked', 'omega/no_atom', 'omega/rho0', 'omega/trans_exact', 'bond/len', 'bond/no_atom',
    'bond/ang_zero', 'rama/not_scored', 'rama/no_torsion', 'peptide/cis_pro', 'peptide/trans', 'hb/no_h_first', 'hb/no_h_unlinked', 'hb/no_h_proline',
    'hb/no_h_atom', 'hb/no_acceptor_atom', 'hb/no_ca', 'hb/ca_far', 'hb/close', 'hb/floor', 'hb/weak', 'hb/bonded', 'hb/unscored_donor', 'atom/masked',
    'atom/not_finite', 'residue/absent', 'row/not_scored', 'type/byte20')


def regions_array(table):
    """a table in degrees -> (K, 8) fp32: cos, sin of phi_lo, phi_hi, psi_lo, psi_hi in float64, rounded once (what hip.rama_regions has to return)"""
    t = np.radians(np.asarray(table, dtype=np.float64).reshape(-1, 4))
    return np.stack([np.cos(t), np.sin(t)], -1).reshape(-1, 8).astype(np.float32)


# ------------------------------------------------------------------------------------------ the arithmetic, in the header's association
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _d2(a, b):
    d = a - b
    return _dot(d, d)


def torsion(p0, p1, p2, p3):
    """-> (cos, sin, defined, flat) of the torsion of four point arrays, in their dtype; flat = min(|n1| / (|b1| |b2|), |n2| / (|b2| |b3|)), the smaller sine of
    the two bond angles, is for the condition on the inputs only"""
    b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
    n1, n2 = _cross(b1, b2), _cross(b2, b3)
    x = _dot(n1, n2)
    y = np.sqrt(_dot(b2, b2)) * _dot(b1, n2)
    rho = np.sqrt(x * x + y * y)
    ok = (rho > 0) & (rho < np.inf)
    safe = np.where(ok, rho, rho.dtype.type(1))
    l1, l2, l3 = np.sqrt(_dot(b1, b1)), np.sqrt(_dot(b2, b2)), np.sqrt(_dot(b3, b3))
    return x / safe, y / safe, ok, np.minimum(np.sqrt(_dot(n1, n1)) / (l1 * l2), np.sqrt(_dot(n2, n2)) / (l2 * l3))


def cos_angle(a, v, b):
    u, w = a - v, b - v
    den = np.sqrt(_dot(u, u)) * np.sqrt(_dot(w, w))
    ok = (den > 0) & (den < np.inf)
    return _dot(u, w) / np.where(ok, den, den.dtype.type(1)), ok


def statement(pos, mask, rows, seqs=None, link=None, regions=None, hb_cutoff=HB_CUTOFF, dtype=np.float32):
    """The definition for ONE candidate in the arithmetic `dtype`: pos (L, A, 3) fp32, mask (L, A), rows (L,) flags, seqs (L,) bytes or None, link (L,) or None,
    regions (K, 8) fp32 (None: regions_array(RAMA_REGIONS)).
    -> dict(torsion (L, 6), bond (L, 3) in dtype; have, rama, ss, state (L,) and partner (L, 2), count (24,) int64; hb (L, L) bool [acceptor, donor]; e: the
    energy where every gate but the cutoff holds, else NaN; margins: dict of arrays, see `condition`; tally: {rule: how often})."""
    dt = dtype
    pos32 = np.asarray(pos, dtype=np.float32)
    mask, rows = np.asarray(mask).astype(bool), np.asarray(rows).astype(bool)
    L = mask.shape[0]
    t = np.full(L, 255, np.int64) if seqs is None else np.asarray(seqs).astype(np.int64)
    pro, gly = t == PRO, t == GLY
    step = np.ones(L, bool) if link is None else np.asarray(link).astype(bool).copy()
    step[L - 1] = False                                                                      # there is no step L - 1
    regions = regions_array(RAMA_REGIONS) if regions is None else np.asarray(regions, dtype=np.float32).reshape(-1, 8)
    K = len(regions)
    cutoff = dt(np.float32(hb_cutoff))
    tally = dict.fromkeys(RULES, 0)
    idx = np.arange(L)
    with np.errstate(all='ignore'):
        ok = (mask & np.isfinite(pos32).all(-1))[:, :4]                                       # the one rule of taking part
        part = ok.any(1)
        x = pos32.astype(dt)
        n, ca, c, o = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
        tally['atom/masked'] += int((~mask[:, :4]).sum())
        tally['atom/not_finite'] += int((mask[:, :4] & ~np.isfinite(pos32[:, :4]).all(-1)).sum())
        tally['residue/absent'] += int((rows & ~part).sum())
        tally['row/not_scored'] += int((~rows).sum())
        tally['type/byte20'] += int((t >= 20).sum()) if seqs is not None else 0
        prev, nxt = np.maximum(idx - 1, 0), np.minimum(idx + 1, L - 1)
        first = idx == 0
        step_prev = ~first & step[prev]                                                       # step r - 1 is linked
        okn, okca, okc, oko = ok[:, 0], ok[:, 1], ok[:, 2], ok[:, 3]
        own3 = okn & okca & okc
        # ---- torsions
        have = np.zeros(L, np.int64)
        tor = np.zeros((L, 6), dt)
        near_flat, flats = [], []
        for k, (name, pts, linked, atoms) in enumerate((('phi', (c[prev], n, ca, c), step_prev, okc[prev] & own3),
                                                        ('psi', (n, ca, c, n[nxt]), step, own3 & okn[nxt]),
                                                        ('omega', (ca, c, n[nxt], ca[nxt]), step, okca & okc & okn[nxt] & okca[nxt]))):
            cs, sn, good, flat = torsion(*pts)
            want = rows & linked & atoms
            got = want & good
            tor[:, 2 * k] = np.where(got, cs, dt(0))
            tor[:, 2 * k + 1] = np.where(got, sn, dt(0))
            have |= np.where(got, HV[name], 0)
            tally[f'{name}/defined'] += int(got.sum())
            tally[f'{name}/unlinked'] += int((rows & ~linked & ~(first & (name == 'phi'))).sum())
            tally[f'{name}/no_atom'] += int((rows & linked & ~atoms).sum())
            tally[f'{name}/rho0'] += int((want & ~good).sum())
            near_flat.append(flat[got])
            flats.append(np.where(got, flat, np.inf))
        tally['phi/first'] += int((rows & first).sum())
        has_phi, has_psi, has_om = (have & 1) != 0, (have & 2) != 0, (have & 4) != 0
        tally['omega/trans_exact'] += int((has_om & (tor[:, 4] == -1) & (tor[:, 5] == 0)).sum())
        # ---- peptide geometry of the step r -> r + 1
        bond = np.zeros((L, 3), dt)
        wantb = rows & step & okc & okn[nxt]
        length = np.sqrt(_d2(c, n[nxt]))
        got = wantb & (length < np.inf)
        bond[:, 0] = np.where(got, length, dt(0))
        have |= np.where(got, HV['len'], 0)
        a1, g1 = cos_angle(ca, c, n[nxt])
        a2, g2 = cos_angle(c, n[nxt], ca[nxt])
        got1, got2 = wantb & okca & g1, wantb & okca[nxt] & g2
        bond[:, 1], bond[:, 2] = np.where(got1, a1, dt(0)), np.where(got2, a2, dt(0))
        have |= np.where(got1, HV['ang_c'], 0) | np.where(got2, HV['ang_n'], 0)
        tally['bond/len'] += int(got.sum())
        tally['bond/no_atom'] += int((rows & step & ~(okc & okn[nxt])).sum())
        tally['bond/ang_zero'] += int((wantb & okca & ~g1).sum() + (wantb & okca[nxt] & ~g2).sum())
        # ---- Ramachandran class
        both = has_phi & has_psi
        rama = np.where(both, K, 255)
        half = []
        for k in range(K - 1, -1, -1):                                                        # downwards: the lowest matching k is kept
            q = regions[k].astype(dt)
            tests = (tor[:, 1] * q[0] - tor[:, 0] * q[1], tor[:, 0] * q[3] - tor[:, 1] * q[2], tor[:, 3] * q[4] - tor[:, 2] * q[5], tor[:, 2] * q[7] - tor[:, 3] * q[6])
            inside = (tests[0] >= 0) & (tests[1] >= 0) & (tests[2] >= 0) & (tests[3] >= 0)
            rama = np.where(both & inside, k, rama)
            half += [np.abs(v[both]) for v in tests]
        tally['rama/not_scored'] += int((~rows).sum())
        tally['rama/no_torsion'] += int((rows & ~both).sum())
        # ---- peptide flags
        cis, twisted = has_om & (tor[:, 4] > 0), has_om & (np.abs(tor[:, 5]) > dt(0.5))
        tally['peptide/cis_pro'] += int((cis & pro[nxt]).sum())
        tally['peptide/trans'] += int((has_om & ~cis & ~twisted).sum())
        # ---- the amide hydrogen, as in section 6.10
        u = c[prev] - o[prev]
        ulen = np.sqrt(_dot(u, u))
        atoms = okn & okc[prev] & oko[prev]
        has_h = step_prev & ~pro & atoms & (ulen > 0)
        h = n + u / ulen[:, None]
        for name, sel in (('hb/no_h_first', first), ('hb/no_h_unlinked', ~first & ~step[prev]), ('hb/no_h_proline', step_prev & pro),
                          ('hb/no_h_atom', step_prev & ~pro & ~atoms)):
            tally[name] += int((sel & part).sum())
        # ---- the relation hb[a, d]: acceptor a (rows), donor d (columns)
        a, d = idx[:, None], idx[None, :]
        bonded = ((d == a + 1) & step[:, None]) | ((a == d + 1) & step[None, :])
        want = has_h[None, :] & (a != d) & ~bonded
        acc_ok = (okc & oko)[:, None]
        ca_ok = okca[:, None] & okca[None, :]
        d2ca = _d2(ca[None, :], ca[:, None])
        gate = want & acc_ok & ca_ok & (d2ca < dt(81))
        r_on, r_ch = np.sqrt(_d2(o[:, None], n[None, :])), np.sqrt(_d2(c[:, None], h[None, :]))
        r_oh, r_cn = np.sqrt(_d2(o[:, None], h[None, :])), np.sqrt(_d2(c[:, None], n[None, :]))
        one = dt(1)
        raw = dt(Q_HB) * (((one / r_on + one / r_ch) - one / r_oh) - one / r_cn)
        close = (r_on < dt(0.5)) | (r_ch < dt(0.5)) | (r_oh < dt(0.5)) | (r_cn < dt(0.5))
        e = np.where(close, dt(CLAMP), np.where(raw < dt(CLAMP), dt(CLAMP), raw))
        hb = gate & (e < cutoff)
        tally['hb/bonded'] += int((has_h[None, :] & bonded).sum())
        tally['hb/no_acceptor_atom'] += int((want & ~acc_ok & part[:, None]).sum())
        tally['hb/no_ca'] += int((want & acc_ok & ~ca_ok).sum())
        tally['hb/ca_far'] += int((want & acc_ok & ca_ok & ~(d2ca < dt(81))).sum())
        tally['hb/close'] += int((gate & close).sum())
        tally['hb/floor'] += int((gate & ~close & (raw < dt(CLAMP))).sum())
        tally['hb/weak'] += int((gate & ~hb).sum())
        tally['hb/unscored_donor'] += int((hb & ~rows[None, :]).sum())
        # ---- patterns
        H = np.zeros((L + 8, L + 8), bool)                                                    # Hbond(i, j), false outside the row: padded by 1 before, 7 after
        H[1:L + 1, 1:L + 1] = hb
        hbond = lambda i, j: H[np.clip(i + 1, 0, L + 7), np.clip(j + 1, 0, L + 7)]
        lk = np.zeros(L + 12, bool)                                                           # step r, false outside the row: padded by 1 before
        lk[1:L + 1] = step
        linked = lambda r: lk[np.clip(r + 1, 0, L + 11)]
        run = np.zeros(L, np.int64)
        for k in range(5):
            run = np.where((run == k) & linked(idx + k), k + 1, run)
        turn = {m: (run >= m) & hbond(idx, idx + m) for m in (3, 4, 5)}
        for m in (3, 4, 5):
            tally[f'turn/{m}'] += int(turn[m].sum())
            tally['turn/unlinked'] += int(((run < m) & hbond(idx, idx + m)).sum())
        tpad = {m: np.concatenate([np.zeros(8, bool), turn[m], np.zeros(8, bool)]) for m in (3, 4, 5)}
        at = lambda m, i: tpad[m][np.clip(i + 8, 0, L + 15)]
        helix = {m: np.zeros(L, bool) for m in (3, 4, 5)}
        inside_turn = np.zeros(L, bool)
        for m in (3, 4, 5):
            for i0 in range(-m + 1, 1):                                                       # i = r + i0 in r - m + 1 .. r
                i = idx + i0
                helix[m] |= (i >= 1) & at(m, i - 1) & at(m, i)
                if i0 < 0:
                    inside_turn |= at(m, i)
        scored = rows & part
        i, j = idx[:, None], idx[None, :]
        eligible = (np.abs(i - j) >= 3) & (linked(idx - 1) & linked(idx))[:, None] & (linked(idx - 1) & linked(idx))[None, :]
        par_a, par_b = hbond(i - 1, j) & hbond(j, i + 1), hbond(j - 1, i) & hbond(i, j + 1)
        anti_a, anti_b = hbond(i, j) & hbond(j, i), hbond(i - 1, j + 1) & hbond(j - 1, i + 1)
        any_form = par_a | par_b | anti_a | anti_b
        tally['bridge/unlinked'] += int((any_form & (np.abs(i - j) >= 3) & ~eligible & scored[:, None]).sum())
        tally['bridge/too_near'] += int((any_form & (np.abs(i - j) < 3) & scored[:, None]).sum())
        for name, m in (('par_a', par_a), ('par_b', par_b), ('anti_a', anti_a), ('anti_b', anti_b)):
            tally[f'bridge/{name}'] += int((m & eligible & scored[:, None]).sum())
        par, anti = (par_a | par_b) & eligible, (anti_a | anti_b) & eligible
        tally['bridge/partner_not_scored'] += int(((par | anti) & scored[:, None] & ~rows[None, :]).sum())
        lowest = lambda m: np.where(m.any(1), m.argmax(1), -1)
        ss = (np.where(helix[4], SS['h4'], 0) | np.where(helix[3], SS['h3'], 0) | np.where(helix[5], SS['h5'], 0) | np.where(par.any(1), SS['par'], 0) |
              np.where(anti.any(1), SS['anti'], 0) | np.where(inside_turn, SS['turn'], 0))
        ss = np.where(scored, ss, 0)
        state = np.where((ss & SS['h4']) != 0, 0, np.where((ss & (SS['par'] | SS['anti'])) != 0, 1, np.where((ss & SS['h3']) != 0, 2, np.where(
            (ss & SS['h5']) != 0, 3, np.where((ss & SS['turn']) != 0, 4, 5)))))
        state = np.where(scored, state, 255)
        partner = np.where(scored[:, None], np.stack([lowest(par), lowest(anti)], 1), -1)
        for m in (3, 4, 5):
            tally[f'helix/{m}'] += int((helix[m] & scored).sum())
        tally['inside'] += int((inside_turn & scored).sum())
        # ---- counts
        count = np.zeros(len(COUNTS), np.int64)
        col = {name: k for k, name in enumerate(COUNTS)}
        count[col['part']] = scored.sum()
        count[col['phipsi']] = both.sum()
        for k in range(min(K, 8)):
            count[col[f'region{k}']] = (both & (rama == k)).sum()
        count[col['outliers']] = (both & (rama == K)).sum()
        count[col['outliers_gly']] = (both & (rama == K) & gly).sum()
        count[col['omega']], count[col['cis']], count[col['cis_nonpro']], count[col['twisted']] = has_om.sum(), cis.sum(), (cis & ~pro[nxt]).sum(), twisted.sum()
        for k, letter in enumerate(SS_LETTERS):
            count[col[letter]] = (state == k).sum()
        count[col['hb_donor']], count[col['hb_acceptor']] = (hb & rows[None, :]).sum(), (hb & rows[:, None]).sum()
        for name in COUNTS:
            tally[f'count/{name}'] += int(count[col[name]])
        rel = lambda v, thr: np.abs(v / thr - 1)
        om = has_om
        margins = dict(hb=np.abs(e - cutoff)[gate], half=np.concatenate([rel(r[gate], dt(0.5)) for r in (r_on, r_ch, r_oh, r_cn)]),
                       ca=rel(d2ca, dt(81))[want & acc_ok & ca_ok], plane=np.concatenate(half) if half else np.zeros(0),
                       cis=np.abs(tor[om, 4]), twisted=np.abs(np.abs(tor[om, 5]) - dt(0.5)), flat=np.concatenate(near_flat))
        inv = dict(on=one / r_on, ch=one / r_ch, oh=one / r_oh, cn=one / r_cn)
    return dict(torsion=tor, bond=bond, have=have, rama=rama, ss=ss, state=state, partner=partner, count=count, hb=hb, e=np.where(gate, e, np.nan), gate=gate,
                close=close, inv=inv, margins=margins, tally=tally, flat=np.stack(flats, 1))


FLAT = 0.1                                  # |n1| >= FLAT |b1| |b2| and |n2| >= FLAT |b2| |b3| for every defined torsion: no bond angle within 5.7 degrees of straight


def condition(ref):
    """The condition on the inputs, on the FLOAT64 statement `ref`: no bond energy within 1e-3 kcal/mol of hb_cutoff, no d2(CA, CA) within 1e-4 relative of 81, no
    bond distance within 1e-4 relative of 0.5 A, no half-plane value, cos omega or |sin omega| - 0.5 within 1e-4 of 0, and |n1| >= FLAT |b1| |b2|,
    |n2| >= FLAT |b2| |b3| for every defined torsion (the exactly collinear cases are undefined and so not concerned).  With s = FLAT the rounding bound of
    cos and sin, u (7 / s^2 + 22 / s + 6) (tests/test_backbone.py: torsion_bound), is 5.5e-5: below the half-plane margin, so no class can flip.  -> the names of the margins that are violated (empty: it holds)."""
    limit = dict(hb=1e-3, half=1e-4, ca=1e-4, plane=1e-4, cis=1e-4, twisted=1e-4, flat=FLAT)
    return [name for name, v in ref['margins'].items() if v.size and np.nanmin(v) < limit[name]]


INTEGERS = ('have', 'rama', 'ss', 'state', 'partner', 'count')


def grouped(pos, mask, rows, seqs, link, regions, hb_cutoff, S, dtype=np.float32):
    """statement over G groups of S candidates: mask (G*S or G, L, A), seqs (G*S or G, L) or None, rows (G, L), link (G, L) or None
    -> (dict of the stacked outputs, tally summed, the per-candidate results)."""
    N = pos.shape[0]
    outs = []
    for c in range(N):
        g = c // S
        outs.append(statement(pos[c], mask[c] if mask.shape[0] == N else mask[g], rows[g], None if seqs is None else seqs[c] if seqs.shape[0] == N else seqs[g],
                              None if link is None else link[g], regions, hb_cutoff, dtype))
    tally = {r: sum(o['tally'][r] for o in outs) for r in RULES}
    return {k: np.stack([o[k] for o in outs]) for k in ('torsion', 'bond') + INTEGERS}, tally, outs


# ------------------------------------------------------------------------------------------ inputs: the builder
BOND = dict(n_ca=1.458, ca_c=1.525, c_n=1.329, c_o=1.231, ca_cb=1.53)
ANGLE = dict(n_ca_c=111.0, ca_c_n=116.2, c_n_ca=121.7, ca_c_o=120.5)


def _unit(v):
    return v / np.linalg.norm(v)


def place(a, b, c, length, angle, tors):
    """the point d with |d - c| = length, angle(b, c, d) = angle and torsion(a, b, c, d) = tors (degrees): the natural extension reference frame"""
    th, ch = np.radians(angle), np.radians(tors)
    bc = _unit(c - b)
    nrm = _unit(np.cross(b - a, bc))
    m = np.cross(nrm, bc)
    return c + length * (-np.cos(th) * bc + np.sin(th) * np.cos(ch) * m + np.sin(th) * np.sin(ch) * nrm)


def nerf(phi, psi, omega=None, A=5):
    """A segment with ideal bond lengths and angles: residue r gets phi[r], psi[r] and omega[r] (the peptide to r + 1; default 180) -> (n, A, 3) float64: N, CA, C,
    O, CB, the further slots scattered around CA (deterministically)."""
    n = len(phi)
    omega = [180.0] * n if omega is None else omega
    x = np.zeros((n, max(A, 5), 3))
    x[0, 0], x[0, 1] = [0.0, 0.0, 0.0], [BOND['n_ca'], 0.0, 0.0]
    ghost = np.array([-0.6, -1.2, 0.3])                                                       # stands for C of a residue before the first, for phi[0]
    for r in range(n):
        if r:
            x[r, 0] = place(x[r - 1, 0], x[r - 1, 1], x[r - 1, 2], BOND['c_n'], ANGLE['ca_c_n'], psi[r - 1])
            x[r, 1] = place(x[r - 1, 1], x[r - 1, 2], x[r, 0], BOND['n_ca'], ANGLE['c_n_ca'], omega[r - 1])
        x[r, 2] = place(x[r - 1, 2] if r else ghost, x[r, 0], x[r, 1], BOND['ca_c'], ANGLE['n_ca_c'], phi[r])
        x[r, 3] = place(x[r, 0], x[r, 1], x[r, 2], BOND['c_o'], ANGLE['ca_c_o'], psi[r] + 180.0)
        x[r, 4] = place(x[r, 2], x[r, 0], x[r, 1], BOND['ca_cb'], 110.5, -122.6)
        for s in range(5, A):
            x[r, s] = x[r, 1] + 1.5 * np.array([np.sin(1.3 * s + r), np.cos(2.1 * s - r), np.sin(0.7 * s * r + 1.0)])
    return x[:, :A]


def plant_co(x, a, d, r_on=2.9):
    """move C=O of residue a onto the N-H of residue d: O at r_on from N_d along H_d's direction (that of C - O of residue d - 1), C 1.23 A beyond it"""
    hdir = _unit(x[d - 1, 2] - x[d - 1, 3])
    x[a, 3] = x[d, 0] + r_on * hdir
    x[a, 2] = x[a, 3] + 1.23 * hdir


def _rotation(rng):
    q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    return q * np.sign(np.linalg.det(q))


def two_strands(form, A=5, rng=None):
    """Two extended five-residue strands 4.5 A apart, the second a translated copy of the first (rows 0 .. 4 and 5 .. 9, a chain break between them), and ONE
    bridge of `form` planted between i = 2 and j = 7 -- the two hydrogen bonds of that alternative, atom by atom."""
    s = nerf([-120.0] * 5, [130.0] * 5, A=A)
    axis = _unit(s[4, 1] - s[0, 1])
    side = _unit(np.cross(axis, [0.0, 1.0, 0.0] if rng is None else rng.normal(size=3)))     # (the fixed direction: no bond but the planted two)
    x = np.concatenate([s, s + 4.5 * side])
    i, j = 2, 7
    for a, d in () if form is None else dict(par_a=((i - 1, j), (j, i + 1)), par_b=((j - 1, i), (i, j + 1)), anti_a=((i, j), (j, i)), anti_b=((i - 1, j + 1), (j - 1, i + 1)))[form]:
        plant_co(x, a, d)
    return x


def exact_segment(A=5):
    """Six residues written down coordinate by coordinate (all exactly representable): 0 -> 1 an exactly planar trans peptide (CA, C, N', CA' at z = 0: sin omega = 0.0 and
    cos omega = -1.0 exactly; N of 0 lies off the plane, or psi would be exactly 0 and sit on a region's bound); CA, C of 2 and N of 3 exactly collinear along x (psi and omega of 2: rho = 0, undefined; the angle at C is a straight one);
    C of 4 coincides with its CA (every torsion through them: rho = 0; the angle at C: no denominator)."""
    x = np.zeros((6, max(A, 5), 3))
    x[0, :5] = [[-1.25, 1.0, 0.75], [0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.0, -1.125, 0.5], [-0.5, -0.75, -1.25]]
    x[1, :5] = [[2.25, 1.0, 0.0], [3.75, 1.0, 0.0], [4.5, 2.25, 0.75], [4.0, 3.25, 1.0], [4.25, 0.25, -1.0]]
    x[2, :5] = [[5.75, 2.25, 1.0], [6.5, 3.5, 1.5], [8.0, 3.5, 1.5], [8.5, 4.5, 2.0], [6.0, 4.5, 0.5]]
    x[3, :5] = [[9.25, 3.5, 1.5], [10.0, 4.75, 1.75], [11.5, 4.5, 2.0], [12.0, 3.5, 2.5], [9.5, 5.75, 2.75]]
    x[4, :5] = [[12.25, 5.5, 2.0], [13.5, 6.0, 2.5], [13.5, 6.0, 2.5], [14.5, 6.5, 3.5], [13.75, 7.25, 1.5]]
    x[5, :5] = [[14.5, 5.25, 3.0], [15.75, 5.5, 3.75], [17.0, 5.0, 3.0], [17.25, 3.75, 3.0], [15.5, 6.75, 4.5]]
    for s in range(5, A):
        x[:, s] = x[:, 1] + [0.5 * s, -0.25 * s, 1.0]
    return x[:, :A]


# module name -> (rows it takes, builder(A, rng) -> (coordinates, {offset: type letter}, [offsets of steps to unlink when a link row is given]))
def _helix(phi, psi, n):
    return lambda A, rng: (nerf([phi] * n, [psi] * n, A=A), {}, [])


def _pi(A, rng):
    """a loose coil with two consecutive 5-turns planted (helix_5 on residues 1 .. 5)"""
    x = nerf([-75.0] * 9, [-50.0] * 9, A=A)
    plant_co(x, 0, 5)
    plant_co(x, 1, 6)
    return x, {}, []


def _turn(A, rng):
    """a single 3-turn planted on an extended segment: residues 1, 2 are inside a turn and in no helix"""
    x = nerf([-65.0, -65.0, -90.0, -100.0, -120.0, -120.0], [-35.0, -35.0, 5.0, 120.0, 130.0, 130.0], A=A)
    plant_co(x, 0, 3)
    return x, {}, []


def _misc(A, rng):
    """alpha-L, a residue in no default region, a Gly outlier, cis before Pro, cis before a non-Pro, twisted (140 degrees: 150 lies ON the threshold
    |sin| = 0.5, which the condition on the inputs keeps away from), not twisted (160), and one residue in each of the five further boxes of EIGHT_REGIONS"""
    phi = [-70.0, 60.0, 60.0, 90.0, -80.0, -75.0, -90.0, -100.0, -110.0, 60.0, -100.0, -100.0, 5.0, 150.0, -120.0]
    psi = [140.0, 45.0, -150.0, 175.0, 155.0, 160.0, 120.0, 130.0, 140.0, 145.0, -150.0, 70.0, -95.0, -105.0, 130.0]
    omega = [180.0, 180.0, 180.0, 180.0, 0.0, 180.0, 0.0, 140.0, 160.0, 180.0, 180.0, 180.0, 180.0, 180.0, 180.0]
    return nerf(phi, psi, omega, A=A), {3: 'G', 5: 'P', 7: 'A'}, []


def _bridge(form):
    return lambda A, rng: (two_strands(form, A, rng), {}, [4])


def _clamps(A, rng):
    """both ways into the clamp of the energy at -9.9: O of residue 1 at 1.2 A from N of 7 (0.2 A from its H: a distance below 0.5 A), O of residue 8 at 1.6 A from
    N of 3 (every distance above 0.5 A, the energy below -9.9)"""
    x = two_strands(None, A, rng)
    plant_co(x, 1, 7, 1.2)
    plant_co(x, 8, 3, 1.6)
    return x, {}, [4]


def _broken_helix(A, rng):
    """an alpha helix with a Pro donor (no H: one bond missing) and, where links are given, an unlinked step in its middle"""
    return nerf([-57.0] * 14, [-47.0] * 14, A=A), {6: 'P'}, [8]


def _broken_bridge(A, rng):
    """an antiparallel bridge beside an unlinked step: step i = 2 of the first strand (the bridge needs it)"""
    return two_strands('anti_a', A, rng), {}, [2, 4]


MODULES = dict(alpha=(12, _helix(-57.0, -47.0, 12)), g310=(10, _helix(-49.0, -26.0, 10)), beta=(6, _helix(-120.0, 130.0, 6)), pi=(9, _pi), turn=(6, _turn),
               misc=(15, _misc), exact=(6, lambda A, rng: (exact_segment(A), {}, [])), par_a=(10, _bridge('par_a')), par_b=(10, _bridge('par_b')),
               anti_a=(10, _bridge('anti_a')), anti_b=(10, _bridge('anti_b')), broken_helix=(14, _broken_helix), broken_bridge=(10, _broken_bridge), clamps=(10, _clamps))
ORDER = ('alpha', 'anti_a', 'misc', 'g310', 'par_a', 'exact', 'pi', 'anti_b', 'turn', 'clamps', 'par_b', 'broken_helix', 'beta', 'broken_bridge')


def candidate(L, A, with_link, seed, far, start):
    """One candidate of L residues: the modules of ORDER from `start` on, cyclically, as long as they fit (the rest is an extended segment), each under a random
    rotation (none for 'exact': its exact plane and line survive a translation, not a rotation) 40 A from the last; a module ends in a chain break, which is an unlinked step when a
    link row is given and a long "bond" when not.  Then, from L = 7 on: residues without atoms, without N, CA, C or O, with NaN and inf coordinates, the bytes 20,
    21 and 255.  far: everything moved by SHIFT.  -> (pos (L, A, 3) fp32, mask (L, A) bool, seqs (L,) uint8, link (L,) bool or None)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((L, A, 3))
    seqs = rng.choice([AA.index(c) for c in 'ADEKLSTV'], size=L).astype(np.uint8)
    link = np.ones(L, bool)
    r, k, exact_rows = 0, start, []
    while r < L:
        name = ORDER[k % len(ORDER)]
        n, build = MODULES[name]
        k += 1
        if n > L - r:
            if k - start > len(ORDER):                                                       # nothing fits any more: an extended tail
                n, name = L - r, 'tail'
                build = lambda A, rng, n=n: (nerf([-120.0] * n, [130.0] * n, A=A), {}, [])
            else:
                continue
        seg, types, cuts = build(A, rng)
        rot = np.eye(3) if name == 'exact' else _rotation(rng)                            # a translation keeps a plane z = const and a line y, z = const exact
        x[r:r + n] = seg @ rot.T + 40.0 * (k - start) * _unit(rng.normal(size=3))
        if name == 'exact':
            exact_rows = list(range(r, r + n))
        for off, letter in types.items():
            seqs[r + off] = AA.index(letter)
        for off in cuts + [n - 1]:
            link[r + off] = False
        r += n
    if far:
        x = x + np.array(SHIFT)
    pos = x.astype(np.float32)
    mask = np.ones((L, A), bool)
    if L >= 7:
        free = [q for q in rng.permutation(L) if q not in exact_rows]
        pick = lambda m: free[m % len(free)]
        mask[pick(0)] = False
        for m, s in enumerate((1, 0, 2, 3)):
            mask[pick(1 + m), s] = False
        pos[pick(5), int(rng.integers(4)), int(rng.integers(3))] = np.nan
        pos[pick(6), int(rng.integers(4)), int(rng.integers(3))] = np.inf
        seqs[pick(7)], seqs[pick(8)], seqs[pick(9)] = 20, 21, 255
    return pos, mask, seqs, (link if with_link else None)


SEEDS = 64                                  # a candidate that violates the condition on the inputs is drawn again, from the next of this many seeds


@functools.lru_cache(maxsize=None)
def case(G, S, L, A, with_link=False, with_seqs=True, eight=False, far=False, other_cutoff=False, seed=0):
    """G groups of S candidates, built once per key and treated as read-only.  rows: four residues in five are scored, no prefix (every one at L <= 3).  link: None,
    or the chain breaks of the modules -- ONE row per group, so the candidates of a group share their modules' order and differ in rotations, planted masks
    and types.  regions: the default three boxes, or EIGHT_REGIONS.  Every candidate satisfies `condition` on its float64 statement: it is drawn again from the
    next seed until it does (at most SEEDS times; `redraws` says how often), none is dropped.
    -> dict(pos, mask, rows, seqs, link, regions, hb_cutoff, redraws, and the float64 statement of every candidate as ref)."""
    key = ((((((G * 8 + S) * 1024 + L) * 16 + A) * 2 + with_link) * 2 + eight) * 2 + far) * 8 + 4 * with_seqs + 2 * other_cutoff + seed
    rng = np.random.default_rng(key)
    rows = np.ones((G, L), bool) if L <= 3 else rng.random((G, L)) < 0.8
    regions = regions_array(EIGHT_REGIONS if eight else RAMA_REGIONS)
    cutoff = OTHER_CUTOFF if other_cutoff else HB_CUTOFF
    pos, mask, seqs, links, ref, redraws = [], [], [], [], [], 0
    for c in range(G * S):
        g = c // S
        start = int(key + 3 * g) % len(ORDER)
        for attempt in range(SEEDS):
            one = candidate(L, A, with_link, (key * 1000 + c) * SEEDS + attempt, far, start)
            r64 = statement(one[0], one[1], rows[g], one[2] if with_seqs else None, one[3], regions, cutoff, np.float64)
            if not condition(r64):
                break
            redraws += 1
        else:
            raise AssertionError(f'no candidate of {SEEDS} satisfies the condition on the inputs: {(G, S, L, A, c)}: {condition(r64)}')
        pos.append(one[0]); mask.append(one[1]); seqs.append(one[2]); ref.append(r64)
        if c % S == 0:
            links.append(one[3])
    return dict(pos=np.stack(pos), mask=np.stack(mask), rows=rows, seqs=np.stack(seqs) if with_seqs else None, link=np.stack(links) if with_link else None,
                regions=regions, hb_cutoff=cutoff, redraws=redraws, ref=ref)
