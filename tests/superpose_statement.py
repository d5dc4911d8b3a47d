"""The float64 statement of abopt_superposed_rmsd and abopt_cluster_shapes_grouped (include/abopt.h) and the inputs of
tests/test_superpose.py with the conditions they satisfy; numpy only, importable without a device.

The definition: Kabsch by SVD with the determinant correction (proper rotations only), the points paired by rank from the masks, the not-scored rule of the
header.  `horn` is the same fit by the largest eigenvector of the 4x4 key matrix (numpy's eigh), the form the device uses; the CPU tests hold the two equal.
Greedy clustering is the walk of tests/test_pose_clusters.py::greedy_f64 over the superposed relation (`greedy_walk`, held equal to it on a relation both can
express).

Conditions, asserted where a case is built (`case` / `cluster_case` walk seeds until they hold and record how many were passed over; they are conditions on
the inputs, not on the code):
  (a) no pair's float64 RMSD lies within 1e-4 A of a clustering cutoff used on it;
  (b) every scored pair of a Q x R case has a key-matrix eigen-gap above 1e-3 (tests/dockq_cases.py::key_matrix_gap): the rotation is well determined, so
      an RMSD over points other than the fitted ones, and rot / trans, are too;
  (c) the case contains what it claims to exercise."""
import functools

import numpy as np

from dockq_cases import FAR, _rotation, key_matrix_gap

MARGIN = 1e-4           # (a), Angstrom
GAP = 1e-3              # (b), relative
MAXLEN = 256


# ------------------------------------------------------------------------------------------ the fit
def kabsch(x, y):
    """Best proper rotation and translation of x (n, 3) onto y (n, 3), float64, by SVD with the determinant correction -> (R, t): y ~ x @ R.T + t."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    cx, cy = x.mean(0), y.mean(0)
    U, _, Vt = np.linalg.svd((x - cx).T @ (y - cy))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    return R, cy - R @ cx


def horn(x, y):
    """The same fit by Horn's quaternion: the eigenvector of the largest eigenvalue of the 4x4 key matrix of S[a][b] = sum (x_a - cx_a)(y_b - cy_b)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    cx, cy = x.mean(0), y.mean(0)
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = (x - cx).T @ (y - cy)
    K = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx], [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy], [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    a, b, c, d = np.linalg.eigh(K)[1][:, 3]
    R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
    return R, cy - R @ cx


def rmsd_under(R, t, x, y):
    """sqrt(mean |R x + t - y|^2) in float64"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return float(np.sqrt((((x @ np.asarray(R, np.float64).T + t) - y) ** 2).sum(-1).mean()))


def pair(x, xfit, xscore, y, yfit, yscore, fit=kabsch):
    """One query row x (na, 3) against one reference row y (nb, 3).  Masks: bool arrays or None (fit: all; score: the row's fit mask).
    -> dict(rmsd, n_fit, n_score, rot, trans, gap); a pair that is not scored has rmsd -1, counts 0, the identity and 0 (gap: inf)."""
    xf = np.ones(len(x), bool) if xfit is None else np.asarray(xfit, bool)
    yf = np.ones(len(y), bool) if yfit is None else np.asarray(yfit, bool)
    xs = xf if xscore is None else np.asarray(xscore, bool)
    ys = yf if yscore is None else np.asarray(yscore, bool)
    nf, ns = int(xf.sum()), int(xs.sum())
    if nf != int(yf.sum()) or ns != int(ys.sum()) or nf < 3 or ns == 0:
        return dict(rmsd=-1.0, n_fit=0, n_score=0, rot=np.eye(3), trans=np.zeros(3), gap=np.inf)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    R, t = fit(x[xf], y[yf])                                        # rank pairing: the k-th true element of either side
    return dict(rmsd=rmsd_under(R, t, x[xs], y[ys]), n_fit=nf, n_score=ns, rot=R, trans=t, gap=key_matrix_gap(y[yf], x[xf]))


def rows(q, qfit, qscore, r, rfit, rscore, fit=kabsch):
    """Every query row against every reference row -> dict of arrays: rmsd, gap (Q, R) float64, n_fit, n_score (Q, R) int32, rot (Q, R, 3, 3), trans (Q, R, 3)"""
    Q, R = len(q), len(r)
    out = dict(rmsd=np.zeros((Q, R)), gap=np.zeros((Q, R)), n_fit=np.zeros((Q, R), np.int32), n_score=np.zeros((Q, R), np.int32), rot=np.zeros((Q, R, 3, 3)),
               trans=np.zeros((Q, R, 3)))
    row = lambda m, i: None if m is None else m[i]
    for i in range(Q):
        for j in range(R):
            for k, v in pair(q[i], row(qfit, i), row(qscore, i), r[j], row(rfit, j), row(rscore, j), fit).items():
                out[k][i, j] = v
    return out


def fit_rmsd_batch(X, Y):
    """X, Y (P, n, 3): the RMSD of each pair after the best fit of X[p] onto Y[p] on all n points (float64, batched SVD); NaN where a pair holds a NaN."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    out = np.full(len(X), np.nan)
    ok = np.isfinite(X).all((1, 2)) & np.isfinite(Y).all((1, 2))
    if not ok.any():
        return out
    xc, yc = X[ok] - X[ok].mean(1, keepdims=True), Y[ok] - Y[ok].mean(1, keepdims=True)
    U, _, Vt = np.linalg.svd(np.einsum('pka,pkb->pab', xc, yc))
    V = np.swapaxes(Vt, 1, 2)
    d = np.sign(np.linalg.det(V @ np.swapaxes(U, 1, 2)))
    d[d == 0] = 1.0
    V[:, :, 2] *= d[:, None]
    R = V @ np.swapaxes(U, 1, 2)
    out[ok] = np.sqrt(((np.einsum('pab,pkb->pka', R, xc) - yc) ** 2).sum((1, 2)) / X.shape[1])
    return out


def shape_rmsd(x):
    """One group x (S, n, 3) -> (S, S) float64 superposed RMSD over all n points, the pair (a, b) evaluated as (row min, row max); 0 on the diagonal."""
    S = len(x)
    iu = np.triu_indices(S, 1)
    m = np.zeros((S, S))
    m[iu] = fit_rmsd_batch(x[iu[0]], x[iu[1]])
    return m + m.T


def greedy_walk(adj, max_clusters=0):
    """The greedy walk of tests/test_pose_clusters.py::greedy_f64 over a given neighbour relation adj (S, S) bool -> (label [S], centre [C], size [C])"""
    adj = np.array(adj, dtype=bool)
    S = len(adj)
    adj[np.arange(S), np.arange(S)] = True
    alive = np.ones(S, dtype=bool)
    label, centre, size = -np.ones(S, dtype=np.int64), [], []
    while alive.any() and not (max_clusters and len(centre) >= max_clusters):
        cnt = (adj & alive[None]).sum(1)
        cnt[~alive] = -1
        c = int(np.argmax(cnt))
        members = adj[c] & alive
        label[members] = len(centre)
        centre.append(c)
        size.append(int(members.sum()))
        alive &= ~members
    return label, np.array(centre, dtype=np.int64), np.array(size, dtype=np.int64)


def greedy_shapes(rm, cutoff, max_clusters=0):
    """The definition of abopt_cluster_shapes_grouped for ONE group from its float64 RMSD matrix rm (shape_rmsd): a ~ b iff rm[a, b] <= cutoff (NaN: no)."""
    with np.errstate(invalid='ignore'):
        return greedy_walk(rm <= float(cutoff), max_clusters)


# ------------------------------------------------------------------------------------------ inputs: Q x R
def _walk(rng, n):
    step = rng.normal(size=(n, 3))
    step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
    return np.cumsum(step, 0)


def random_motion(rng, shift=15.0):
    """a random proper rotation (any angle) and a translation of about `shift` A per axis, float64"""
    return _rotation(rng.normal(size=3), rng.uniform(0.5, np.pi)), rng.normal(size=3) * shift


def _mask_with(rng, n, count):
    """`count` true elements among n, not a prefix whenever that is possible"""
    m = np.zeros(n, bool)
    m[rng.choice(n, count, replace=False)] = True
    if 0 < count < n and m[:count].all():
        m[count - 1], m[n - 1] = False, True
    return m


# tag -> dict(na, nb, Q, R, masks): 'null' = no mask at all (na == nb); 'fit' = fit masks, the score masks NULL; 'score' = all four masks, the score sets
# other than the fit sets; 'half' = the query has masks and the reference none.  far: translated far from the origin.  The lengths are those at which a
# 64-lane ballot, the 16-row tile and the 256-element row end.
LENGTHS = (3, 4, 15, 16, 17, 63, 64, 65, 255, 256)
SPECS = {f'null_{n}': dict(na=n, nb=n, Q=5, R=7, masks='null') for n in LENGTHS}
SPECS.update({
    'fit_17_64': dict(na=17, nb=64, Q=18, R=17, masks='fit'),
    'fit_256_65': dict(na=256, nb=65, Q=6, R=5, masks='fit'),
    'score_63_255': dict(na=63, nb=255, Q=7, R=6, masks='score'),
    'score_16_15': dict(na=16, nb=15, Q=17, R=33, masks='score'),
    'score_256_256': dict(na=256, nb=256, Q=4, R=5, masks='score'),
    'half_65_4': dict(na=65, nb=4, Q=6, R=3, masks='half'),
    'far_64': dict(na=64, nb=64, Q=4, R=5, masks='null', far=True),
    'far_score_17_65': dict(na=17, nb=65, Q=5, R=4, masks='score', far=True),
})
TAGS = tuple(SPECS)


def build(tag, seed):
    """-> the case dict of SPECS[tag] from `seed`: q (Q, na, 3), r (R, nb, 3) fp32; qfit, qscore, rfit, rscore bool or None; want = rows(...) on those values"""
    sp = SPECS[tag]
    na, nb, Q, R, kind = sp['na'], sp['nb'], sp['Q'], sp['R'], sp['masks']
    rng = np.random.default_rng([seed, na, nb, Q])
    shift = FAR if sp.get('far') else 0.0
    q = np.stack([_walk(rng, na) + rng.normal(size=3) * 10.0 + shift for _ in range(Q)]).astype(np.float32)
    r = np.stack([_walk(rng, nb) + rng.normal(size=3) * 10.0 + shift for _ in range(R)]).astype(np.float32)
    c = dict(tag=tag, seed=seed, kind=kind, q=q, r=r, qfit=None, qscore=None, rfit=None, rscore=None)
    lo = min(na, nb)
    if kind != 'null':
        # fit counts: two sizes that occur on both sides, one pair of rows with fewer than three and one empty row
        big = [lo, max(3, lo - 1)] if kind != 'half' else [lo, lo]
        qcount = [big[i % 2] for i in range(Q)]
        rcount = [big[(i // 2) % 2] for i in range(R)]
        qcount[-1], qcount[-2] = 0, 2
        if kind != 'half':
            rcount[-1], rcount[-2] = 2, 0
            c['rfit'] = np.stack([_mask_with(rng, nb, k) for k in rcount])
        c['qfit'] = np.stack([_mask_with(rng, na, k) for k in qcount])
    if kind == 'score':
        # score counts: two sizes again, and one row that scores nothing
        small = [max(1, lo // 2), max(1, lo // 3)]
        qs = [small[(i // 2) % 2] for i in range(Q)]
        rs = [small[i % 2] for i in range(R)]
        qs[0] = 0
        c['qscore'] = np.stack([_mask_with(rng, na, k) for k in qs])
        c['rscore'] = np.stack([_mask_with(rng, nb, k) for k in rs])
    c['want'] = rows(q, c['qfit'], c['qscore'], r, c['rfit'], c['rscore'])
    return c


def conditions(c):
    """-> the list of conditions (b), (c) that case c breaks (empty: all hold)"""
    w, kind, bad = c['want'], c['kind'], []
    scored = w['n_fit'] > 0
    claim = lambda ok, text: None if ok else bad.append('(c) ' + text)
    if not (w['gap'][scored] > GAP).all():
        bad.append(f'(b) eigen-gap {w["gap"][scored].min():.2e}')
    claim(scored.any(), 'a scored pair')
    if kind == 'null':
        claim(scored.all(), 'every pair scored')
    count = lambda m, n: np.full(n, -1) if m is None else m.sum(1)
    if kind in ('fit', 'score'):
        fq, fr = count(c['qfit'], len(c['q'])), count(c['rfit'], len(c['r']))
        claim((~scored).any() and (fq[:, None] != fr[None]).any(), 'pairs whose fit counts differ')
        claim(((fq[:, None] == fr[None]) & (fq[:, None] == 2)).any(), 'a pair with two fit points on both sides')
        claim((fq == 0).any() and (fr == 0).any(), 'an empty row on either side')
        prefix = lambda m: all(row[:row.sum()].all() for row in m)
        claim(not prefix(c['qfit']) and not prefix(c['rfit']), 'masks that are no prefixes')
    if kind == 'score':
        sq, sr = c['qscore'].sum(1), c['rscore'].sum(1)
        fits = count(c['qfit'], len(c['q']))[:, None] == count(c['rfit'], len(c['r']))[None]
        claim((fits & (sq[:, None] != sr[None])).any(), 'pairs whose fit counts agree and whose score counts differ')
        claim((sq == 0).any(), 'a row that scores nothing')
        claim((scored & (w['n_score'] != w['n_fit'])).any() and (c['qscore'] != c['qfit']).any(), 'scored pairs whose score set is not their fit set')
    if kind == 'half':
        claim((~scored).any() and scored.any() and c['rfit'] is None, 'masks on the query side only, scored and unscored pairs')
    if c['tag'].startswith('far'):
        claim(np.abs(c['q']).min() > 500.0, 'every coordinate far from the origin')
    return bad


@functools.lru_cache(maxsize=None)
def case(tag):
    """The case `tag`, built once per process and shared by the tests, which leave it unchanged: the first seed from 7 on whose inputs satisfy the conditions."""
    for seed in range(7, 207):
        c = build(tag, seed)
        bad = conditions(c)
        if not bad:
            break
    assert not bad, (tag, bad)                                       # conditions on the inputs, not on the code
    c['seeds_tried'] = seed - 7
    return c


@functools.lru_cache(maxsize=None)
def _moved(tag):
    c = case(tag)
    for seed in range(1, 201):
        rng = np.random.default_rng([seed, len(c['q'])])
        q = np.stack([x.astype(np.float64) @ R.T + t for x, (R, t) in ((x, random_motion(rng, 100.0)) for x in c['q'])]).astype(np.float32)
        if c['kind'] != 'null' or (np.abs(plain_rmsd(q, c['r']) - plain_rmsd(c['q'], c['r'])) > 1.5).all():
            break
    else:
        raise AssertionError((tag, 'no motion that moves every unsuperposed RMSD'))       # a condition on the inputs, not on the code
    return q, rows(q, c['qfit'], c['qscore'], c['r'], c['rfit'], c['rscore'])


def moved(c):
    """case c with every query row moved by its own random rotation and translation (about 100 A per axis) in float64 and rounded to fp32 -> (q_moved fp32,
    the statement on it).  Where both sides have one length and no masks, the motion is one under which the float64 RMSD WITHOUT superposition of every pair
    changes by more than 1.5 A (seeds are walked until it does)."""
    return _moved(c['tag'])


def plain_rmsd(q, r):
    """(Q, R) float64 RMSD WITHOUT superposition of rows of one length"""
    d = np.asarray(q, np.float64)[:, None] - np.asarray(r, np.float64)[None]
    return np.sqrt((d * d).sum((2, 3)) / q.shape[1])


# ------------------------------------------------------------------------------------------ inputs: clustering
FAMILIES = 4
CLUSTER_SHAPES = [(S, n) for S in (1, 63, 64, 65, 129) for n in (3, 16, 40)]      # S: word boundaries of the bit rows; G = 3 throughout
CLUSTER_G = 3


def _family_shapes(rng, n):
    """FAMILIES shapes of n points.  n = 3: triangles with two 3.8 A sides and apex angles 50, 85, 120, 155 degrees (random walks of three points can be
    arbitrarily alike); else random walks."""
    if n == 3:
        return np.stack([np.array([[3.8, 0, 0], [0, 0, 0], [3.8 * np.cos(a), 3.8 * np.sin(a), 0]]) for a in np.deg2rad([50.0, 85.0, 120.0, 155.0])])
    return np.stack([_walk(rng, n) for _ in range(FAMILIES)])


def _cluster_inputs(S, n, seed):
    rng = np.random.default_rng([seed, S, n])
    x, fam = [], []
    for g in range(CLUSTER_G):
        shapes = _family_shapes(rng, n)
        f = rng.integers(0, FAMILIES, size=S)
        for k in f:
            R, t = random_motion(rng, 20.0)
            x.append(shapes[k] @ R.T + t + rng.normal(size=(n, 3)) * 0.05)
        fam.append(f)
    return np.stack(x).astype(np.float32), np.stack(fam)


def _window(values, lo, hi):
    """the midpoint of the widest gap of `values` inside [lo, hi] (the ends close the first and the last gap) -> (cutoff, distance of the nearest value)"""
    v = np.sort(values[np.isfinite(values)])
    pts = np.concatenate([[lo], v[(v > lo) & (v < hi)], [hi]])
    i = int(np.argmax(np.diff(pts)))
    cut = 0.5 * (pts[i] + pts[i + 1])
    return cut, (np.abs(v - cut).min() if v.size else np.inf)


@functools.lru_cache(maxsize=None)
def cluster_case(S, n):
    """G = 3 groups of S structures of n points: members of FAMILIES shape families, each rigidly displaced at random (about 20 A per axis) plus 0.05 A noise,
    rounded to fp32 -> dict(x (G*S, n, 3) fp32, family (G, S), rm (G, S, S) float64 superposed RMSDs, tight: a cutoff between the largest RMSD within a
    family and the smallest between two, mixed: a cutoff inside the range of the between-family RMSDs (clusters that merge families, and ties)).
    Conditions: (a) both cutoffs lie more than 1e-4 A from every pair's RMSD; (c) tight separates the families."""
    for seed in range(7, 207):
        x, fam = _cluster_inputs(S, n, seed)
        rm = np.stack([shape_rmsd(x[g * S:(g + 1) * S]) for g in range(CLUSTER_G)])
        iu = np.triu_indices(S, 1)
        same = np.concatenate([(fam[g][:, None] == fam[g][None])[iu] for g in range(CLUSTER_G)])
        pairs = np.concatenate([rm[g][iu] for g in range(CLUSTER_G)])
        within, between = pairs[same], pairs[~same]
        if S == 1:
            tight, mixed, margin, ok = 0.3, 1.0, np.inf, True
            break
        wmax = within.max() if within.size else 0.0
        if not between.size or not between.min() > wmax + 10 * MARGIN:
            continue
        tight = 0.5 * (wmax + between.min())
        mixed, m2 = _window(pairs, np.quantile(between, 0.3), np.quantile(between, 0.6))
        margin = min(np.abs(pairs - tight).min(), m2)
        ok = margin > MARGIN
        if ok:
            break
    assert ok, (S, n)                                                # conditions on the inputs, not on the code
    return dict(x=x, family=fam, rm=rm, tight=float(tight), mixed=float(mixed), margin=float(margin), seeds_tried=seed - 7)


def same_partition(label, family):
    """the clusters are the families: two structures share a label iff they share a family"""
    label, family = np.asarray(label), np.asarray(family)
    return bool(((label[:, None] == label[None]) == (family[:, None] == family[None])).all())
