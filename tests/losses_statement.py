"""Plain torch statements of the row kernels of the training path (csrc/rows.hip: dpm_losses_kernel, abdock_losses_kernel, row_layer_norm_kernel
with its backward, heads_epilogue_backward_kernel) and the cases they are tested on: TEST INFRASTRUCTURE.  Nothing in the product imports this file.

Every statement takes a dtype: float64 is the reference, float32 measures what float32 arithmetic can reach (tests/yardstick.py).  Each is
written from the reference's lines (D/ = AbDock/src/), not from the kernel:
  dpm_losses       rotation_matrix_cosine_loss D/modules/diffusion/dpm_full.py:15-32 (F.cosine_embedding_loss written out: 1e-12 on the squared norms),
                   the position MSE :217-220, the posterior KL :222-231 on transition.py:217-229 (plain_statement.posterior; F.kl_div written out)
  abdock_losses    pRMSDCa.calc_rmsd / calc_prmsd_loss D/modules/common/prmsd.py:49-111 on DistanceToBins(use_onehot) layers.py:48-51,
                   pred_start_from_noise transition.py:52-60, calc_dist_loss dpm_full.py:369-378 (cdist and SmoothL1 written out)
  layer_norm       D/modules/common/layers.py:146-155
  heads_epilogue   dpm_full.py:95-103 through plain_statement.quat1ijk_to_rot
The cases come from seeded generators on the CPU; no files.  tests/test_row_kernel_edges.py checks the statements against the torch functions
the older tests use and every case against its input conditions, on the CPU."""
import types

import torch

import plain_statement

SEQ_STATES = list(range(-1, 22)) + [24]                 # -1, 0 .. 19, 20, 21, 24: what s_t / s_0 are drawn from
ALPHA_BARS = [1.0, 0.999, 0.5, 0.011, 0.0]
MARGIN = 1e-3                                            # an unplanted RMSD is at least this far (relative) from every bin midpoint


def _leaf(x, dtype, dev):
    return x.to(device=dev, dtype=dtype).clone().requires_grad_()


# ------------------------------------------------------------------------------------------ dpm losses
def cosine_columns(R_pred, R_true):
    """rotation_matrix_cosine_loss: 1 - cos between the columns, summed over the three; cosine_embedding_loss adds 1e-12 to each squared norm."""
    x, y = R_pred.transpose(-2, -1), R_true.transpose(-2, -1)          # rows = the matrices' columns
    cos = (x * y).sum(-1) / torch.sqrt(((x * x).sum(-1) + 1e-12) * ((y * y).sum(-1) + 1e-12))
    return (1 - cos).sum(-1)


def posterior_kl(abar, s_t, s_0, c_den):
    """F.kl_div(log(post_pred + 1e-8), post_true, log_target=False).sum(-1) = sum xlogy(t, t) - t * input."""
    t = torch.arange(abar.shape[0], device=abar.device)
    post_true = plain_statement.posterior(abar, s_t, s_0, t)
    post_pred = plain_statement.posterior(abar, s_t, c_den, t)
    return (torch.xlogy(post_true, post_true) - post_true * torch.log(post_pred + 1e-8)).sum(-1)


def dpm_losses(c, dtype, dev='cpu'):
    """c: a dpm case -> rows (N, L, 3) per-residue (rot, pos, seq), sums (3,) over the generated residues, d sums / d (R_pred, p_pred, c_den)."""
    f = lambda x: x.to(device=dev, dtype=dtype)
    Rp, pp, cd = _leaf(c.R_pred, dtype, dev), _leaf(c.p_pred, dtype, dev), _leaf(c.c_den, dtype, dev)
    gen = c.gen.to(dev)
    rot = cosine_columns(Rp, f(c.R_0))
    pos = ((pp - f(c.p_target)) ** 2).sum(-1)
    seq = posterior_kl(f(c.abar), c.s_t.to(dev), c.s_0.to(dev), cd)
    rows = torch.stack([rot, pos, seq], -1)
    sums = (rows * gen[..., None]).sum((0, 1))
    gR, gp, gc = torch.autograd.grad([sums[0], sums[1], sums[2]], [Rp, pp, cd])
    return dict(rows=rows.detach(), sums=sums.detach(), gR=gR, gp=gp, gc=gc)


def dpm_case(N, L, mask_kind, seed):
    """Inputs mixed within the case: alpha_bar from ALPHA_BARS by sample (rotated by the seed), s_t / s_0 from SEQ_STATES, c_den rows that are smooth,
    exact one-hots (on s_t's state, where the posterior survives, and elsewhere, where it is 0 + 1e-8) or carry exact zeros, R_pred rows that are
    ordinary, equal to R_0 bit for bit, have one zero column (the 1e-12 guard) or are far from orthogonal.  mask_kind: 'mixed' (one sample
    generates nothing when N > 1), 'none' (nothing in the batch), 'last' (the last row only)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ri = lambda hi, *s: torch.randint(0, hi, s, generator=g)
    idx = torch.arange(N * L).reshape(N, L)
    R_0 = plain_statement.so3_exp(rn(N, L, 3).double() * 1.5).float()
    rk = (idx * 5 + seed) % 4
    R_pred = R_0 + 0.1 * rn(N, L, 3, 3)
    R_pred = torch.where((rk == 1)[..., None, None], R_0, R_pred)
    zero_col = torch.nn.functional.one_hot(ri(3, N, L), 3).bool()[:, :, None, :]
    R_pred = torch.where((rk == 2)[..., None, None] & zero_col, torch.zeros(()), R_pred)
    R_pred = torch.where((rk == 3)[..., None, None], 20 * rn(N, L, 3, 3), R_pred)
    states = torch.tensor(SEQ_STATES)
    s_t, s_0 = states[ri(len(SEQ_STATES), N, L)], states[ri(len(SEQ_STATES), N, L)]
    s_0 = torch.where(ri(3, N, L) == 0, s_t, s_0)                              # s_t == s_0 often enough: the true posterior is a one-hot there when alpha_bar = 1
    ck = (idx * 3 + seed) % 4
    smooth = torch.softmax(rn(N, L, 20) * 2, -1)
    hot_at = torch.where(ck == 1, s_t.clamp(0, 19), ri(20, N, L))
    c_den = torch.where(((ck == 1) | (ck == 2))[..., None], torch.nn.functional.one_hot(hot_at, 20).float(), smooth)
    c_den = torch.where((ck == 3)[..., None] & (ri(4, N, L, 20) == 0), torch.zeros(()), c_den)
    abar = torch.tensor([ALPHA_BARS[(n + seed) % 5] for n in range(N)])
    if mask_kind == 'mixed':
        gen = torch.rand(N, L, generator=g) < 0.6
        gen[:, L // 2] = True
        if N > 1:
            gen[(seed + 1) % N] = False
    else:
        gen = torch.zeros(N, L, dtype=torch.bool)
        if mask_kind == 'last':
            gen[-1, -1] = True
    return types.SimpleNamespace(N=N, L=L, R_pred=R_pred, R_0=R_0, p_pred=rn(N, L, 3), p_target=rn(N, L, 3), c_den=c_den, s_t=s_t, s_0=s_0, abar=abar,
                                 gen=gen, rot_kind=rk, c_kind=ck, mask_kind=mask_kind)


def dpm_other_rows(c, seed):
    """The same case with the inputs of the rows that are not generated replaced by other finite values of ordinary size (|x| <= 1e3)."""
    g = torch.Generator().manual_seed(seed)
    N, L, off = c.N, c.L, ~c.gen
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * 1e3
    d = types.SimpleNamespace(**vars(c))
    for name in ('R_pred', 'R_0', 'p_pred', 'p_target', 'c_den'):
        x = getattr(c, name)
        setattr(d, name, torch.where(off.reshape(N, L, *([1] * (x.dim() - 2))), u(*x.shape), x))
    states = torch.tensor(SEQ_STATES)
    for name in ('s_t', 's_0'):
        setattr(d, name, torch.where(off, states[torch.randint(0, len(SEQ_STATES), (N, L), generator=g)], getattr(c, name)))
    return d


# ------------------------------------------------------------------------------------------ abdock losses
def abdock_rmsd(c, dtype, p_pred=None, dev='cpu'):
    """-> rmsd (N,) of calc_rmsd on the un-normalised positions (the mean cancels in the difference: scale only), the chosen bin, and the margin:
    the distance of the rmsd to the nearest midpoint between two different offsets, relative to the rmsd (inf with one offset value)."""
    f = lambda x: x.to(device=dev, dtype=dtype)
    p_pred = f(c.p_pred) if p_pred is None else p_pred
    p0, gen = f(c.p0n), c.gen.to(dev)
    if c.pred_x0:
        pred_p0 = p_pred
    else:
        pred_p0 = torch.where(gen[..., None], f(c.coef_a).view(-1, 1, 1) * p0 - f(c.coef_b).view(-1, 1, 1) * p_pred, p0)
    pa, pb = pred_p0 * c.scale * gen[..., None], p0 * c.scale * gen[..., None]
    rmsd = torch.sqrt(((pa - pb) ** 2).sum(-1).sum(-1) / gen.sum(-1)).detach()
    off = f(c.offsets)
    bin_ = torch.argmin(torch.abs(rmsd[:, None] - off), dim=-1)
    vals = torch.unique(off)
    mid = (vals[1:] + vals[:-1]) / 2
    margin = (torch.abs(rmsd[:, None] - mid).min(-1).values / rmsd) if mid.numel() else torch.full_like(rmsd, float('inf'))
    return rmsd, bin_, margin


def smooth_l1(x):
    ax = x.abs()
    return torch.where(ax < 1, 0.5 * x * x, ax - 0.5)


def pair_distances(p):
    return (p[:, :, None, :] - p[:, None, :, :]).norm(dim=-1)


def abdock_losses(c, dtype, dev='cpu'):
    """c: an abdock case -> the raw outputs of the entry (part columns err, m0, sl_sum, sl_cnt; glogit = softmax - onehot; gp = d sum of the smooth-l1
    terms / d p_pred) and, as training.AbdockLosses returns them, prmsd, dist and their gradients with respect to the logits and p_pred."""
    f = lambda x: x.to(device=dev, dtype=dtype)
    logits, p_pred = _leaf(c.logits, dtype, dev), _leaf(c.p_pred, dtype, dev)
    gen, mres = c.gen.to(dev), c.mres.to(dev)
    rmsd, bin_, margin = abdock_rmsd(c, dtype, p_pred, dev)
    onehot = torch.zeros_like(logits).scatter_(-1, bin_[:, None], 1.0)
    logp = torch.log_softmax(logits, dim=-1)
    err = -(onehot * logp).sum(-1)
    m0 = gen[:, 0].to(dtype)
    prmsd = (err * m0).sum() / (m0.sum() + 1e-10)
    out = dict(rmsd=rmsd, bin=bin_, margin=margin, err=err.detach(), m0=m0, glogit=(torch.softmax(logits, -1) - onehot).detach(), prmsd=prmsd.detach())
    sel = gen[:, :, None] & (mres[:, :, None] & mres[:, None, :])
    out['sl_cnt'] = sel.sum((1, 2)).to(dtype)
    if c.pred_x0:
        sl = smooth_l1(pair_distances(p_pred) - pair_distances(f(c.p0n))) * sel
        sl_sum = sl.sum((1, 2))
        dist = sl_sum.sum() / sel.sum()
        out['gp'] = torch.autograd.grad(sl_sum.sum(), p_pred, retain_graph=True)[0]
        out['sl_sum'] = sl_sum.detach()
    else:
        dist = p_pred.sum() * 0.0
        out['gp'], out['sl_sum'], out['sl_cnt'] = torch.zeros_like(p_pred), torch.zeros_like(err), torch.zeros_like(err)
    out['dist'] = dist.detach()
    out['d_logits'] = torch.autograd.grad(prmsd, logits)[0]
    out['d_p_pred'] = torch.autograd.grad(dist, p_pred)[0] if torch.isfinite(dist) else None
    return out


# roles of a sample: how far the predicted positions lie from the true ones (x position_scale = the RMSD's size), and its masks
ROLES = ['ordinary', 'empty', 'below', 'above', 'no_first']
ROLE_SIGMA = dict(ordinary=0.5, empty=0.5, below=0.004, above=2.5, no_first=0.3)
TIE_SHIFT, TIE_SCALE = 0.1875, 8.0                     # 3/16 x 8 = 1.5 with every step exact in float32 and float64


def abdock_case(N, L, nb, pred_x0, seed, tie=False, no_first=False):
    """An abdock case.  Sample n takes role ROLES[(n + seed) % 5]: 'empty' generates nothing (RMSD = 0 / 0); 'below' / 'above' put the RMSD under the first / over
    the last offset; 'no_first' clears mask_generate[n, 0].  no_first=True clears it in every sample (prmsd = 0).  The residue mask has holes, and generated rows
    lie outside it (L = 1: every one, so the dist loss selects nothing).  With nb = 64 one offset is duplicated at the bin sample 0 chooses.  With L >= 16 and pred_x0, sample 0 carries two selected residues whose
    predicted points coincide and a pair whose distance error is exactly 1.  tie: the offsets are 1, 2, .., the scale 8, and the last sample has one generated
    residue displaced by (3/16, 0, 0) from a true position on the 1/16 grid: RMSD = 1.5 exactly in both precisions, midway between bins 0 and 1.
    (0.15 at scale 10 cannot serve: float32(0.15) x 10 lies half an ulp above 1.5, rounds to 1.5 in float32 and stays above it in float64.)
    Every other sample's RMSD is moved (by stretching one generated residue's displacement) until its margin is at least MARGIN."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    roles = [ROLES[(n + seed) % 5] for n in range(N)]
    scale = TIE_SCALE if tie else 10.0
    p0n = rn(N, L, 3)
    gen = torch.rand(N, L, generator=g) < 0.3
    mres = torch.rand(N, L, generator=g) < 0.85
    gen[:, 0] = True
    gen[:, L // 2] = True
    mres[:, L // 2] = True
    if L == 1:
        mres[:] = False                                     # generated, outside the residue mask: the dist loss selects nothing in the whole batch
    if L >= 4:
        mres[:, 1], gen[:, 1] = False, True                # a hole at the front (not a prefix) that is generated all the same
        mres[:, L - 1] = True
    dev_ = rn(N, L, 3) * torch.tensor([ROLE_SIGMA[r] for r in roles]).view(N, 1, 1)
    planted = torch.zeros(N, L, dtype=torch.bool)
    for n, r in enumerate(roles):
        if r == 'empty':
            gen[n] = False
        if r == 'no_first' or no_first:
            gen[n, 0] = False
    if tie:
        n, l = N - 1, L // 2
        gen[n], roles[n] = False, 'tie'
        gen[n, l] = True
        p0n[n, l] = torch.tensor([0.5, -1.25, 2.0])
        dev_[n, l] = torch.tensor([TIE_SHIFT, 0.0, 0.0])
        planted[n, l] = True
    coef_a, coef_b = torch.rand(N, generator=g) + 1.0, torch.rand(N, generator=g) + 0.5
    offsets = {1: torch.tensor([10.0])}.get(nb, torch.linspace(0.5, 19.5, nb))
    if tie:
        offsets = torch.arange(nb).float() + 1.0
    c = types.SimpleNamespace(N=N, L=L, nb=nb, pred_x0=pred_x0, scale=scale, p0n=p0n, gen=gen, mres=mres, coef_a=coef_a, coef_b=coef_b, offsets=offsets, roles=roles,
                              logits=rn(N, nb) * 2, tie=tie)
    if pred_x0 and L >= 16 and roles[0] != 'empty':         # sample 0: rows a, b coincide in p_pred; rows q, r have |dp| - |dt| = 3 - 2 = 1
        a, b, q, r = 2, 5, 7, 10
        for i in (a, b, q, r):
            gen[0, i] = mres[0, i] = planted[0, i] = True
        p0n[0, q], p0n[0, r] = torch.tensor([1.0, 0.5, -2.0]), torch.tensor([3.0, 0.5, -2.0])
        dev_[0, q], dev_[0, r] = torch.tensor([0.0, 0.0, 0.0]), torch.tensor([1.0, 0.0, 0.0])
        c.coincide, c.joint = (a, b), (q, r)

    def place():                                            # p_pred such that pred_p0 - p0 = dev_ on the generated rows under either objective
        if pred_x0:
            c.p_pred = p0n + dev_
        else:
            c.p_pred = ((coef_a.view(N, 1, 1) - 1) * p0n - dev_) / coef_b.view(N, 1, 1)
        if hasattr(c, 'coincide'):
            c.p_pred[0, c.coincide[1]] = c.p_pred[0, c.coincide[0]]
    place()
    if nb == 64 and not tie and roles[0] != 'empty':        # duplicate offsets: the lower index wins
        j = min(int(abdock_rmsd(c, torch.float64)[1][0]), nb - 2)
        offsets[j + 1] = offsets[j]
        c.duplicate = j
    for _ in range(60):
        rmsd, bin_, margin = abdock_rmsd(c, torch.float64)
        bad = [n for n in range(N) if roles[n] not in ('empty', 'tie') and not margin[n] >= 2 * MARGIN]
        if not bad:
            break
        for n in bad:
            free = (gen[n] & ~planted[n]).nonzero().flatten()
            dev_[n, free[-1]] *= 1.07
        place()
    c.planted = planted
    return c


# ------------------------------------------------------------------------------------------ LayerNorm
def layer_norm(x, gamma, beta, eps):
    """layers.py:146-155 -> y, xhat = (x - mean) / std, 1 / std."""
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    std = (var + eps).sqrt()
    xhat = (x - mean) / std
    return xhat * gamma + beta, xhat, (1 / std).squeeze(-1)


def layer_norm_grads(c, eps, dtype, dev='cpu', sequential=False):
    """-> y, xhat, rstd, dx, d gamma, d beta for the upstream gradient c.dy.  sequential: the same float statement with every sum taken one term after
    the other (forward and the closed-form backward), for the tensors whose float32 error hangs on the order of summation."""
    f = lambda x: x.to(device=dev, dtype=dtype)
    if sequential:
        return _layer_norm_sequential(f(c.x), f(c.gamma), f(c.beta), eps, f(c.dy))
    x, gamma, beta = _leaf(c.x, dtype, dev), _leaf(c.gamma, dtype, dev), _leaf(c.beta, dtype, dev)
    y, xhat, rstd = layer_norm(x, gamma, beta, eps)
    dx, dg, db = torch.autograd.grad((y * f(c.dy)).sum(), [x, gamma, beta])
    return dict(y=y.detach(), xhat=xhat.detach(), rstd=rstd.detach(), dx=dx, dgamma=dg, dbeta=db)


def _seq_sum(t, dim):
    s = torch.zeros_like(t.select(dim, 0))
    for k in range(t.shape[dim]):
        s = s + t.select(dim, k)
    return s


def _layer_norm_sequential(x, gamma, beta, eps, dy):
    cols = x.shape[-1]
    mean = (_seq_sum(x, -1) / cols)[..., None]
    std = (_seq_sum((x - mean) ** 2, -1) / cols + eps).sqrt()[..., None]
    xhat = (x - mean) / std
    g = dy * gamma
    m1, m2 = (_seq_sum(g, -1) / cols)[..., None], (_seq_sum(g * xhat, -1) / cols)[..., None]
    return dict(y=xhat * gamma + beta, xhat=xhat, rstd=(1 / std).squeeze(-1), dx=(g - m1 - xhat * m2) / std,
                dgamma=(dy * xhat).sum(0), dbeta=dy.sum(0))


LN_KINDS = ['ordinary', 'constant', 'offset']


def layer_norm_case(rows, cols, seed, kinds=None):
    """Rows that are ordinary (3 x randn), constant (a small integer: its mean is exact in any order of summation, so x - mean = 0 on every side) or have
    mean 1e4 with unit spread; row r is of kind (r + seed) % 3 unless kinds gives one for all."""
    g = torch.Generator().manual_seed(seed)
    kind = (torch.arange(rows) + seed) % 3 if kinds is None else torch.full((rows,), LN_KINDS.index(kinds))
    x = torch.randn(rows, cols, generator=g) * 3
    const = (torch.randint(-4, 5, (rows, 1), generator=g).float() * 2 + 1).expand(rows, cols)
    x = torch.where((kind == 1)[:, None], const, x)
    x = torch.where((kind == 2)[:, None], 1e4 + torch.randn(rows, cols, generator=g), x)
    return types.SimpleNamespace(rows=rows, cols=cols, x=x, kind=kind, gamma=torch.randn(cols, generator=g), beta=torch.randn(cols, generator=g),
                                 dy=torch.randn(rows, cols, generator=g))


# ------------------------------------------------------------------------------------------ heads epilogue
ROT_SIZES = [0.0, 1e-20, 1e-3, 1.0, 8.0, 1e3, 1e6]


def heads_epilogue(c, dtype, dev='cpu'):
    """dpm_full.py:95-103 -> R_next, eps_pos and d eps_crd, d eps_rot for the upstream gradients c.wR, c.wp."""
    f = lambda x: x.to(device=dev, dtype=dtype)
    crd, rot = _leaf(c.eps_crd, dtype, dev), _leaf(c.eps_rot, dtype, dev)
    R, gen = f(c.R), c.gen.to(dev)
    eps_pos = torch.einsum('lab,lb->la', R, crd)
    eps_pos = torch.where(gen[:, None].expand_as(eps_pos), eps_pos, torch.zeros_like(eps_pos))
    R_next = R @ plain_statement.quat1ijk_to_rot(rot)
    d_crd, d_rot = torch.autograd.grad((R_next * f(c.wR)).sum() + (eps_pos * f(c.wp)).sum(), [crd, rot])
    return dict(R_next=R_next.detach(), eps_pos=eps_pos.detach(), d_crd=d_crd, d_rot=d_rot)


def heads_case(rows, mask_kind, seed):
    """eps_rot rows of size ROT_SIZES[(r + seed) % 7] (the first: exact zeros), mask 'on' / 'off' / 'mixed'."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    size = torch.tensor(ROT_SIZES)[(torch.arange(rows) + seed) % len(ROT_SIZES)]
    gen = dict(on=torch.ones(rows, dtype=torch.bool), off=torch.zeros(rows, dtype=torch.bool), mixed=torch.rand(rows, generator=g) < 0.6)[mask_kind]
    return types.SimpleNamespace(rows=rows, R=plain_statement.so3_exp(rn(rows, 3).double() * 1.5).float(), eps_crd=rn(rows, 3), eps_rot=rn(rows, 3) * size[:, None],
                                 gen=gen, wR=rn(rows, 3, 3), wp=rn(rows, 3), size=size)
