"""What the tests of guided sampling share (tests/test_guided_sampling.py): the float64 statement of include/abopt.h: abopt_guide_positions, and the inputs of
its kernel cases.  numpy only: nothing here needs a device."""
import numpy as np

HOT, REP = 1, 2                     # the bits of a role word


def statement(p, gen, res, role, w_att, r_att, w_rep, r_rep, max_shift):
    """The definition in float64, sample by sample.  p (N, L, 3), gen / res (N, L) bool, role (N, L) or (G, L) with N % G == 0 (sample n reads row n // (N // G)).
    -> dict: p (N, L, 3) the updated positions; shift (N, L, 3) the applied shifts (0 on rows that do not move); moved (N, L) = gen & res; written (N, L): moved
    rows whose shift has a non-zero component; att (N, 3) the attraction; rep (N, L, 3) the repulsion f_i; capped (N, L); dmin: the smallest distance of a moved
    row to a repeller of its sample (inf without a pair)."""
    p = np.asarray(p, dtype=np.float64)
    gen, res, role = np.asarray(gen, bool), np.asarray(res, bool), np.asarray(role)
    N, L = gen.shape
    S = N // role.shape[0] if role.shape[0] else 1
    out = dict(p=p.copy(), shift=np.zeros((N, L, 3)), moved=gen & res, att=np.zeros((N, 3)), rep=np.zeros((N, L, 3)), capped=np.zeros((N, L), bool), dmin=np.inf)
    for n in range(N):
        M = gen[n] & res[n]
        ctx = res[n] & ~gen[n]
        H = ctx & ((role[n // S] & HOT) != 0)
        R = ctx & ((role[n // S] & REP) != 0)
        if not M.any():
            continue
        a = np.zeros(3)
        if H.any():
            d = p[n, H].mean(0) - p[n, M].mean(0)
            D = np.sqrt((d * d).sum())
            if D > 0:
                a = w_att * max(D - r_att, 0.0) / D * d
        out['att'][n] = a
        for i in np.nonzero(M)[0]:
            f = np.zeros(3)
            if R.any():
                diff = p[n, i] - p[n, R]
                d2 = (diff * diff).sum(1)
                ok = d2 >= 1e-12
                dist = np.sqrt(d2[ok])
                if dist.size:
                    out['dmin'] = min(out['dmin'], dist.min())
                f = w_rep * ((np.maximum(r_rep - dist, 0.0) / dist)[:, None] * diff[ok]).sum(0)
            out['rep'][n, i] = f
            delta = a + f
            norm = np.sqrt((delta * delta).sum())
            if norm > max_shift:
                delta = delta * (max_shift / norm)
                out['capped'][n, i] = True
            out['shift'][n, i] = delta
    out['written'] = out['moved'] & (out['shift'] != 0).any(-1)
    out['p'] = np.where(out['written'][..., None], p + out['shift'], p)
    return out


# L -> the scalars of the case, chosen on this statement (never on the device) so that capped, free-moving, repelled and attracted rows all occur: r_rep 6 A reaches
# the bonded neighbours of the walk (3.8 A); w_att and r_att are set against each case's centroid distance (7 .. 16 A) so that the pull alone stays below the cap.
# L = 1100 spreads its moved rows over a long walk and takes a gentler potential with a larger cap.
PARAMS = {63: dict(w_att=0.1, r_att=8.0, w_rep=0.7, r_rep=6.0, max_shift=2.0),
          64: dict(w_att=0.3, r_att=4.0, w_rep=0.7, r_rep=6.0, max_shift=2.0),
          65: dict(w_att=0.3, r_att=4.0, w_rep=0.7, r_rep=6.0, max_shift=2.0),
          1100: dict(w_att=0.25, r_att=10.0, w_rep=0.5, r_rep=5.0, max_shift=3.0)}
DEFAULT_PARAMS = dict(w_att=0.5, r_att=8.0, w_rep=0.7, r_rep=6.0, max_shift=2.0)
CASES = [(1, 1), (3, 7), (2, 63), (2, 64), (2, 65), (5, 130), (1, 1100)]
R_EMPTY_CASE = (3, 7)               # the case without any repeller
OFFSET = (900.0, -700.0, 500.0)     # the second placement of every case


def params(N, L):
    return dict(PARAMS.get(L, DEFAULT_PARAMS))


def case(N, L, offset=(0.0, 0.0, 0.0), seed=0):
    """The inputs of one kernel case, fp32-representable float64 positions: per sample two CA random walks of 3.8 A steps, the second (rows from max(1, L // 3) on)
    starting 6 A along x from the first.  Generated: a run at the end of the first walk plus every 11th row (not a prefix).  From L = 7 on one row per sample is
    absent from mask_res.  Roles random in 0..3 on ALL rows, 3 on the absent one (bits on generated and absent rows must be ignored).  With N >= 2 the last sample has no hotspot; in
    case (5, 130) sample 3 has no generated row; case (3, 7) has no repeller.  -> dict(p, gen, res, role, **params)."""
    rng = np.random.default_rng(1000 * L + N + seed)
    n1 = max(1, L // 3)
    run = max(1, min(n1, L // 6, 24))
    p = np.zeros((N, L, 3))
    for n in range(N):
        step = rng.normal(size=(L, 3))
        step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
        p[n, :n1] = np.cumsum(step[:n1], 0)
        p[n, n1:] = np.array([6.0, 0.0, 0.0]) + np.cumsum(step[n1:], 0)
    p = (p + np.asarray(offset)).astype(np.float32).astype(np.float64)
    gen = np.zeros((N, L), bool)
    gen[:, n1 - run:n1] = True
    gen[:, 10::11] = True
    res = np.ones((N, L), bool)
    if L >= 7:
        for n in range(N):
            res[n, int(rng.integers(0, L))] = False
    role = rng.integers(0, 4, size=(N, L)).astype(np.int32)
    role[~res] = HOT | REP                                             # an absent row carries both bits: they must mean nothing
    if N >= 2:
        role[N - 1] &= ~HOT
    if (N, L) == (5, 130):
        gen[3] = False
    if (N, L) == R_EMPTY_CASE:
        role &= ~REP
    return dict(p=p, gen=gen, res=res, role=role, **params(N, L))


def shares(c, st):
    """of the moved rows of a case: the shares that are capped, that move below the cap, that feel a non-zero repulsion, that feel a non-zero attraction"""
    m = st['moved']
    n = max(1, int(m.sum()))
    rep = (st['rep'] != 0).any(-1) & m
    att = (st['att'] != 0).any(-1)[:, None] & m
    return dict(capped=float((st['capped'] & m).sum()) / n, free=float((st['written'] & ~st['capped']).sum()) / n, repelled=float(rep.sum()) / n,
                attracted=float(att.sum()) / n, moved=int(m.sum()))
