"""The row kernels of the training path at their edges: csrc/rows.hip (dpm_losses_kernel, abdock_losses_kernel, row_layer_norm_kernel and its backward,
heads_epilogue_backward_kernel) against the float64 statements of tests/losses_statement.py.

What the cases are for ("Row kernels of the training path"):
  dpm losses       one thread per residue, 256 per block: N L = 1, 255, 256, 257, 513 (three blocks, the last partial; blocks that span samples with different
                   alpha_bar), 600; alpha_bar 1 and 0, sequence states outside 0 .. 19 on both sides, one-hot and zero-carrying c_den, R_pred = R_0, a zero column, masks
                   that generate nothing in a sample / in the batch / only the last row
  abdock losses    one workgroup per sample, thread k owns residues k, k + 256, ..: L = 1 .. 2049 (past 64 KB of dynamic LDS) and the largest accepted L; masks
                   that are no prefix, generated rows outside the residue mask, a sample without generated residue (RMSD = 0 / 0), an exact tie of the binning,
                   duplicate offsets, RMSD outside the offsets, coinciding points, the smooth-L1 joint
  LayerNorm        one wave per row, lane + 64 q columns: cols 1 .. 256 around the multiples of 64, rows around the 4 of a block and 4097
  heads epilogue   one thread per row: rows around 256; quaternion vectors from exact zero to 1e6

Measure: tests/yardstick.py with scaled floors -- the device is no further from the float64 statement than 1.5 x the float32 torch statement run on the device is
(+1e-6 on the maximum, +1e-7 on the mean, both x max(1, max |float64 value|) of the tensor).  Every pair is printed (pytest -s).

The first section runs on the CPU (not marked gpu): the statements against the torch functions the older tests use, and every case against its input conditions."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import plain_statement
import losses_statement as LS
from yardstick import yardstick

gpu = pytest.mark.gpu
DEV = torch.device('cuda:0')
F32, F64 = torch.float32, torch.float64

DPM_SHAPES = [(1, 1), (1, 255), (1, 256), (1, 257), (3, 171), (2, 300)]
DPM_CASES = [(N, L, kind) for N, L in DPM_SHAPES for kind in ('mixed', 'none', 'last')]
dpm_each = pytest.mark.parametrize('case', DPM_CASES, ids=[f'{N}x{L}-{k}' for N, L, k in DPM_CASES])

#               L     N  nb  tie    no_first
ABDOCK_SHAPES = [(1, 2, 40, False, False), (2, 3, 1, False, False), (255, 4, 64, False, False), (256, 5, 40, True, False), (257, 2, 1, False, True),
                 (300, 3, 64, False, False), (513, 4, 40, True, False), (2049, 2, 64, False, False)]
ABDOCK_CASES = [(L, N, nb, x0, tie and x0, nf) for L, N, nb, tie, nf in ABDOCK_SHAPES for x0 in (True, False)]
abdock_each = pytest.mark.parametrize('case', ABDOCK_CASES, ids=[f"L{c[0]}-N{c[1]}-nb{c[2]}-{'x0' if c[3] else 'noise'}" for c in ABDOCK_CASES])

LN_COLS = [1, 2, 63, 64, 65, 128, 131, 255, 256]
LN_ROWS = [1, 3, 4, 5, 4097]
LN_EPS = [1e-10, 1e-5]
HEADS_ROWS = [1, 255, 256, 257, 385]


@functools.lru_cache(maxsize=None)
def dpm_case(case):
    N, L, kind = case
    return LS.dpm_case(N, L, kind, seed=DPM_CASES.index(case))


@functools.lru_cache(maxsize=None)
def abdock_case(case):
    L, N, nb, x0, tie, nf = case
    return LS.abdock_case(N, L, nb, x0, seed=5 * ABDOCK_CASES.index(case) + (3 if L == 300 else 0), tie=tie, no_first=nf)


def max_length():
    from ab_opt_amd import hip
    return hip.lib().abopt_abdock_losses_max_length()


@functools.lru_cache(maxsize=None)
def bound_case():
    return LS.abdock_case(1, max_length(), 40, True, seed=0)


# ------------------------------------------------------------------------------------------ the statements' own checks and the cases' conditions (CPU)
def test_statements_equal_the_torch_functions():
    """float64: the written-out cosine loss, KL, smooth-L1 on pair distances and LayerNorm equal F.cosine_embedding_loss, F.kl_div, F.smooth_l1_loss with cdist and
    F.layer_norm on random inputs (values and gradients)."""
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    Rp, R0 = rn(7, 9, 3, 3).requires_grad_(), rn(7, 9, 3, 3)
    cp, ct = Rp.transpose(-2, -1).reshape(-1, 3), R0.transpose(-2, -1).reshape(-1, 3)
    ref = F.cosine_embedding_loss(cp, ct, torch.ones(cp.shape[0], dtype=torch.long), reduction='none').reshape(7, 9, 3).sum(-1)
    got = LS.cosine_columns(Rp, R0)
    assert (got - ref).abs().max().item() <= 1e-13
    w = rn(7, 9)
    assert (torch.autograd.grad((got * w).sum(), Rp)[0] - torch.autograd.grad((ref * w).sum(), Rp)[0]).abs().max().item() <= 1e-12
    c = LS.dpm_case(3, 40, 'mixed', seed=2)
    cd = c.c_den.double().requires_grad_()
    t = torch.arange(3)
    ref = F.kl_div(input=torch.log(plain_statement.posterior(c.abar.double(), c.s_t, cd, t) + 1e-8), target=plain_statement.posterior(c.abar.double(), c.s_t, c.s_0, t),
                   reduction='none', log_target=False).sum(-1)
    got = LS.posterior_kl(c.abar.double(), c.s_t, c.s_0, cd)
    assert got.dtype == F64 and ref.abs().max().item() > 0 and (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    ga, gb = torch.autograd.grad(got.sum(), cd)[0], torch.autograd.grad(ref.sum(), cd)[0]
    assert (ga - gb).abs().max().item() <= 1e-12 * gb.abs().max().item()
    p, q = (rn(2, 30, 3) * 2).requires_grad_(), rn(2, 30, 3) * 2
    with torch.no_grad():
        p[0, 3] = p[0, 8]                                                          # zero distance: zero gradient on both sides
    dp, dt = torch.cdist(p, p, compute_mode='donot_use_mm_for_euclid_dist'), torch.cdist(q, q, compute_mode='donot_use_mm_for_euclid_dist')
    ref = F.smooth_l1_loss(dp, dt, reduction='none')
    got = LS.smooth_l1(LS.pair_distances(p) - LS.pair_distances(q))
    assert (got - ref).abs().max().item() <= 1e-13 and (ref > 0.5).any() and (ref < 0.5).any()
    ga, gb = torch.autograd.grad(got.sum(), p)[0], torch.autograd.grad(ref.sum(), p)[0]
    assert torch.isfinite(ga).all() and (ga - gb).abs().max().item() <= 1e-11
    assert LS.smooth_l1(torch.tensor([1.0, -1.0], dtype=F64)).tolist() == [0.5, 0.5] == F.smooth_l1_loss(torch.tensor([3.0, 1.0]), torch.tensor([2.0, 2.0]), reduction='none').tolist()
    for eps in LN_EPS:
        c = LS.layer_norm_case(9, 131, seed=4)
        x, gm, bt = c.x.double().requires_grad_(), c.gamma.double().requires_grad_(), c.beta.double().requires_grad_()
        ordinary = c.kind == 0                  # (on constant and offset rows the two formulas of the variance differ by rounding amplified by 1 / sqrt(eps))
        y, xhat, rstd = LS.layer_norm(x, gm, bt, eps)
        ref = F.layer_norm(x, (131,), gm, bt, eps=eps)
        assert (y - ref)[ordinary].abs().max().item() <= 1e-12
        w = c.dy.double() * ordinary[:, None]
        for a, b in zip(torch.autograd.grad((y * w).sum(), [x, gm, bt]), torch.autograd.grad((ref * w).sum(), [x, gm, bt])):
            assert (a - b).abs().max().item() <= 1e-11
        seq = LS.layer_norm_grads(c, eps, F64, sequential=True)
        plain = LS.layer_norm_grads(c, eps, F64)
        for k in plain:
            assert (seq[k] - plain[k])[ordinary if plain[k].shape[0] == 9 else slice(None)].abs().max().item() <= 1e-9, k
    c = LS.heads_case(9, 'mixed', seed=1)
    out = LS.heads_epilogue(c, F64)
    U = plain_statement.quat1ijk_to_rot(c.eps_rot.double())
    assert (U @ U.transpose(-1, -2) - torch.eye(3, dtype=F64)).abs().max().item() <= 1e-12
    assert not out['eps_pos'][~c.gen].any() and not out['d_crd'][~c.gen].any() and torch.equal(out['R_next'][c.size == 0], c.R.double()[c.size == 0])


def test_dpm_cases_hold_what_they_are_for():
    seen_abar, seen_states = set(), set()
    for case in DPM_CASES:
        c = dpm_case(case)
        N, L, kind = case
        seen_abar |= set(c.abar.tolist())
        seen_states |= set(c.s_t.flatten().tolist()) & set(c.s_0.flatten().tolist())
        assert {'none': 0, 'last': 1}.get(kind, int(c.gen.sum())) == int(c.gen.sum())
        if kind == 'mixed' and N > 1:
            assert (c.gen.sum(1) == 0).sum() == 1
        if kind == 'last':
            assert c.gen[-1, -1]
        if N * L >= 255:
            assert all((c.rot_kind == k).any() and (c.c_kind == k).any() for k in range(4))
            assert torch.equal(c.R_pred[c.rot_kind == 1], c.R_0[c.rot_kind == 1]) and not torch.equal(c.R_pred[c.rot_kind == 0], c.R_0[c.rot_kind == 0])
            assert ((c.R_pred[c.rot_kind == 2] == 0).all(-2).sum(-1) == 1).all()
            hot = (c.c_den == 1).sum(-1) == 1
            assert hot[c.c_kind == 1].all() and hot[c.c_kind == 2].all() and ((c.c_den == 0).any(-1) & ~hot)[c.c_kind == 3].any()
            r64 = LS.dpm_losses(c, F64)
            assert all(torch.isfinite(v).all() for v in r64.values())
            d = LS.dpm_other_rows(c, seed=9)
            assert torch.equal(d.R_pred[c.gen], c.R_pred[c.gen]) and (kind != 'mixed' or not torch.equal(d.R_pred, c.R_pred)) and d.c_den.abs().max() <= 1e3
    assert seen_abar == {float(torch.tensor(a)) for a in LS.ALPHA_BARS} and seen_states == set(LS.SEQ_STATES)
    assert (3 * 171) == 513 and 513 % 256 == 1


def _abdock_conditions(c):
    """Every sample of the case: planted (an exact tie, or no generated residue) or at least MARGIN from every bin midpoint, in float64 -- so the float32 rounding
    of the RMSD (relative 1e-6 at the very most: a sum of up to 3 x 5118 squares) cannot choose another bin."""
    r64, b64, m64 = LS.abdock_rmsd(c, F64)
    r32, b32, _ = LS.abdock_rmsd(c, F32)
    for n, role in enumerate(c.roles):
        if role == 'empty':
            assert c.gen[n].sum() == 0 and torch.isnan(r64[n]) and torch.isnan(r32[n]) and b64[n] == 0 and b32[n] == 0, (n, role)
        elif role == 'tie':
            assert c.gen[n].sum() == 1 and r64[n].item() == 1.5 == r32[n].item() and c.offsets[0] == 1.0 and c.offsets[1] == 2.0 and b64[n] == 0 and b32[n] == 0, (n, role)
        else:
            assert m64[n].item() >= LS.MARGIN and b64[n] == b32[n] and abs(r32[n].item() / r64[n].item() - 1) < 1e-5, (n, role, m64[n].item())
    return r64, b64


def test_abdock_cases_meet_their_input_conditions():
    """No sample of any case is skipped: each is a planted tie, a planted empty sample, or has margin >= 1e-3.  And the cases hold what they are for."""
    below = above = dup = ties = empty = 0
    for case in ABDOCK_CASES:
        c = abdock_case(case)
        L, N, nb, x0, tie, nf = case
        rmsd, bin_ = _abdock_conditions(c)
        live = ~torch.isnan(rmsd)
        below += int((rmsd[live] < c.offsets[0]).sum())
        above += int((rmsd[live] > c.offsets[-1]).sum())
        ties += c.roles.count('tie')
        empty += c.roles.count('empty')
        if hasattr(c, 'duplicate'):
            j = c.duplicate
            assert c.offsets[j] == c.offsets[j + 1] and bin_[0] == j
            dup += 1
        if L >= 4:
            assert ((c.mres[:, :-1] < c.mres[:, 1:]).any(1)).all(), 'a residue mask that is a prefix'
            assert (c.gen & ~c.mres).any()
        assert (not c.gen[:, 0].any()) == (nf or all(r in ('empty', 'no_first', 'tie') for r in c.roles))
        if x0 and L >= 16 and c.roles[0] != 'empty':
            (a, b), (q, r) = c.coincide, c.joint
            assert torch.equal(c.p_pred[0, a], c.p_pred[0, b]) and (c.gen & c.mres)[0, [a, b, q, r]].all()
            assert (c.p_pred[0, q] - c.p_pred[0, r]).norm().item() - (c.p0n[0, q] - c.p0n[0, r]).norm().item() == 1.0
    assert min(below, above, dup, ties, empty) >= 1, (below, above, dup, ties, empty)
    assert sum(1 for c in ABDOCK_CASES if c[5]) == 2
    c = abdock_case(ABDOCK_CASES[0])                                        # L = 1: generated, outside the residue mask: the selection of the dist loss is empty
    assert not (c.gen[:, :, None] & c.mres[:, :, None] & c.mres[:, None, :]).any() and c.gen.any()
    _abdock_conditions(bound_case())
    assert max_length() * 32 > 64 * 1024 and 2049 * 32 > 64 * 1024


def _device_or_host():
    return DEV if torch.cuda.is_available() else torch.device('cpu')


def test_abdock_losses_refuses_a_length_its_kernel_cannot_be_launched_with():
    """abopt_abdock_losses at L one above abopt_abdock_losses_max_length() (and at the 5120 the entry once accepted): ABOPT_EINVAL with the entry's message before any
    HIP call, the output buffers -- pre-filled with a sentinel -- untouched.  Runs with or without a device: without one, any HIP call would come back as ABOPT_EHIP.
    The bound is the kernel's: 160 KB of LDS per workgroup less its 48 bytes of static LDS, at 32 bytes a residue."""
    from ab_opt_amd import hip
    lib, dev = hip.lib(), _device_or_host()
    Lmax = max_length()
    assert 2049 < Lmax <= 160 * 1024 // 32
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for L in (Lmax + 1, Lmax + 2, 10000):
        z = lambda *s: torch.zeros(*s, device=dev)
        logits, pos, off = z(1, 40), z(1, L, 3), z(40) + 1
        gen, mres = torch.ones(1, L, dtype=torch.bool, device=dev), torch.ones(1, L, dtype=torch.bool, device=dev)
        part, gl, gp = z(1, 4) + 7.5, z(1, 40) + 7.5, z(1, L, 3) + 7.5
        rc = lib.abopt_abdock_losses(p(logits), p(pos), p(pos), None, None, p(gen), p(mres), p(off), 40, 1, L, 10.0, 1, p(part), p(gl), p(gp), None)
        msg = lib.abopt_last_error().decode()
        assert rc == 1 and f'L={L} (at most {Lmax})' in msg and msg.startswith('abdock_losses:'), (rc, msg)
        if dev.type == 'cuda':
            torch.cuda.synchronize()
        assert (part == 7.5).all() and (gl == 7.5).all() and (gp == 7.5).all()
    z = lambda *s: torch.zeros(*s, device=dev)
    for nb in (0, 65):
        rc = lib.abopt_abdock_losses(p(z(1, 65)), p(z(1, 4, 3)), p(z(1, 4, 3)), None, None, p(z(1, 4).bool()), p(z(1, 4).bool()), p(z(65)), nb, 1, 4, 10.0, 1, p(z(1, 4)),
                                     p(z(1, 65)), p(z(1, 4, 3)), None)
        assert rc == 1 and f'num_bins={nb}' in lib.abopt_last_error().decode()


def test_layer_norm_refuses_0_and_257_columns():
    from ab_opt_amd import hip
    lib, dev = hip.lib(), _device_or_host()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for cols in (0, 257):
        b = [torch.full((3, 257), 7.5, device=dev) for _ in range(4)] + [torch.full((3,), 7.5, device=dev)]
        gm = torch.ones(257, device=dev)
        assert lib.abopt_layer_norm_forward(p(b[0]), p(gm), p(gm), cols, 1e-5, 3, p(b[1]), p(b[2]), p(b[4]), None) == 1
        assert f'layer_norm: {cols} columns' in lib.abopt_last_error().decode()
        assert lib.abopt_layer_norm_backward(p(b[0]), p(b[2]), p(b[4]), p(gm), cols, 3, p(b[1]), p(b[3]), None) == 1
        assert f'layer_norm_backward: {cols} columns' in lib.abopt_last_error().decode()
        if dev.type == 'cuda':
            torch.cuda.synchronize()
        assert all((t == 7.5).all() for t in b)


# ------------------------------------------------------------------------------------------ device
RATIOS = {}                     # kernel -> {tensor name: (device error, float32 error)}: the worst pair per kernel is printed by each test


def _held(kernel, label, got, r32, r64):
    r = {}
    miss = yardstick(f'{kernel} {label}', got, r32, r64, scaled=True, ratios=r)
    for k, (a, b) in r.items():
        worst = RATIOS.setdefault(kernel, {})
        floor = 1e-6 * max(1.0, r64.abs().max().item())
        if a > floor:                                            # (pairs under the floor say nothing about the factor)
            worst[k] = a / max(b, 1e-300)
            print(f'RATIO {k}: {a / max(b, 1e-300):.3f}')
    return miss


def _d(x):
    return x.to(DEV)


class _Dpm:
    def __init__(self, case):
        self.c = dpm_case(case)
        self.r32, self.r64 = LS.dpm_losses(self.c, F32, DEV), LS.dpm_losses(self.c, F64, DEV)
        self.got = self.run(self.c)

    @staticmethod
    def run(c):
        from ab_opt_amd import hip
        return hip.dpm_losses(_d(c.R_pred), _d(c.R_0), _d(c.p_pred), _d(c.p_target), _d(c.c_den), _d(c.s_t), _d(c.s_0), _d(c.abar), _d(c.gen))


@functools.lru_cache(maxsize=None)
def _dpm(case):
    return _Dpm(case)


@gpu
@dpm_each
def test_dpm_losses_vs_float64(case):
    """hip.dpm_losses: the three sums and the three gradients by the yardstick; the gradient tensors once more on the rows of ordinary size alone (|float64| <= 1e3: a
    zero column of R_pred gives 1e6, a vanished predicted posterior 1e16, and a tensor's floor scales with its maximum); gradients exactly zero outside the mask."""
    k = _dpm(case)
    c, gen = k.c, _d(k.c.gen)
    miss = []
    for name, got in zip(('sums', 'gR', 'gp', 'gc'), k.got):
        assert torch.isfinite(got).all(), name
        miss += _held('dpm_losses', name, got, k.r32[name], k.r64[name])
        if name != 'sums':
            assert not got[~gen].any(), name
            plain = k.r64[name].reshape(c.N, c.L, -1).abs().amax(-1) <= 1e3
            if plain.any() and not plain.all():
                miss += _held('dpm_losses', name + ' (ordinary rows)', got[plain], k.r32[name][plain], k.r64[name][plain])
    assert not miss, miss


@gpu
@dpm_each
def test_dpm_losses_repeat_and_ignore_rows_outside_the_mask(case):
    """The call repeated is bit-identical; the outputs on generated rows and the sums do not change by a bit when the inputs of the other rows are replaced by other
    finite values (|x| <= 1e3)."""
    k = _dpm(case)
    again, other = _Dpm.run(k.c), _Dpm.run(LS.dpm_other_rows(k.c, seed=9))
    gen = _d(k.c.gen)
    for name, a, b, o in zip(('sums', 'gR', 'gp', 'gc'), k.got, again, other):
        assert torch.equal(a, b), name
        assert torch.equal(a, o) if name == 'sums' else (torch.equal(a[gen], o[gen]) and not o[~gen].any()), name


class _Abdock:
    def __init__(self, c):
        from ab_opt_amd import hip
        self.c = c
        self.r32, self.r64 = LS.abdock_losses(c, F32, DEV), LS.abdock_losses(c, F64, DEV)
        self.args = (_d(c.logits), _d(c.p_pred), _d(c.p0n), None if c.pred_x0 else _d(c.coef_a), None if c.pred_x0 else _d(c.coef_b), _d(c.gen), _d(c.mres),
                     _d(c.offsets), c.scale, c.pred_x0)
        self.got = hip.abdock_losses(*self.args)


@functools.lru_cache(maxsize=None)
def _abdock(case):
    return _Abdock(abdock_case(case))


def _abdock_raw(k):
    from ab_opt_amd import hip
    c, r32, r64 = k.c, k.r32, k.r64
    part, gl, gp = k.got
    assert torch.equal(part[:, 1].double(), r64['m0']) and torch.equal(part[:, 3].double(), r64['sl_cnt'])
    assert torch.isfinite(part).all() and torch.isfinite(gl).all() and torch.isfinite(gp).all()
    miss = _held('abdock_losses', 'err', part[:, 0], r32['err'], r64['err']) + _held('abdock_losses', 'sl_sum', part[:, 2], r32['sl_sum'], r64['sl_sum'])
    for n in range(c.N):                                                     # row by row: a wrong bin is an error of 1 in two places
        miss += _held('abdock_losses', f'glogit[{n}] ({c.roles[n]})', gl[n], r32['glogit'][n], r64['glogit'][n])
        onehot = (gl[n].double() - r64['glogit'][n]).abs() < 0.5
        assert onehot.all(), (n, c.roles[n], 'bin', int(r64['bin'][n]))
    miss += _held('abdock_losses', 'gp', gp, r32['gp'], r64['gp'])
    for a, b in zip(k.got, hip.abdock_losses(*k.args)):
        assert torch.equal(a, b)
    return miss


@gpu
@abdock_each
def test_abdock_losses_raw_outputs_vs_float64(case):
    """hip.abdock_losses: part (count and m0 exactly, the cross entropy and the smooth-L1 sum by the yardstick), glogit row by row -- the sample without generated
    residue included: softmax - onehot(0) --, gp; bit-identical on repetition."""
    miss = _abdock_raw(_abdock(case))
    assert not miss, miss


@gpu
@abdock_each
def test_abdock_losses_autograd_function_vs_float64(case):
    """training.AbdockLosses: the two losses and both gradients.  Where the selection of the dist loss is empty, it is non-finite on both sides and not compared further."""
    from ab_opt_amd import training
    k = _abdock(case)
    c, r32, r64 = k.c, k.r32, k.r64
    logits, p_pred = k.args[0].clone().requires_grad_(), k.args[1].clone().requires_grad_()
    prmsd, dist = training.AbdockLosses.apply(logits, p_pred, *k.args[2:])
    miss = _held('AbdockLosses', 'prmsd', prmsd.detach(), r32['prmsd'], r64['prmsd'])
    if not c.gen[:, 0].any():
        assert prmsd.item() == 0 and r64['prmsd'].item() == 0
    if torch.isfinite(r64['dist']):
        assert torch.isfinite(r32['dist'])
        miss += _held('AbdockLosses', 'dist', dist.detach(), r32['dist'], r64['dist'])
        (prmsd + dist).backward()
        miss += _held('AbdockLosses', 'd p_pred', p_pred.grad, r32['d_p_pred'], r64['d_p_pred'])
        if not c.pred_x0:
            assert dist.item() == 0 and not p_pred.grad.any()
    else:
        assert c.pred_x0 and not torch.isfinite(dist) and not torch.isfinite(r32['dist'])
        prmsd.backward()
    miss += _held('AbdockLosses', 'd logits', logits.grad, r32['d_logits'], r64['d_logits'])
    if not c.gen[:, 0].any():
        assert not logits.grad.any() and not r64['d_logits'].any()
    assert not miss, miss


@gpu
def test_abdock_losses_at_the_largest_accepted_length():
    """N = 1 at L = abopt_abdock_losses_max_length() (5118: 163 824 of the 163 840 bytes of LDS, about 26 million pair terms) runs and meets the yardstick."""
    miss = _abdock_raw(_Abdock(bound_case()))
    assert not miss, miss


def _ln_device(c, eps):
    from ab_opt_amd import hip
    x, gm, bt, dy = _d(c.x), _d(c.gamma), _d(c.beta), _d(c.dy)
    y, xhat, rstd = hip.layer_norm_forward(x, gm, bt, eps)
    dx, dg, db = hip.layer_norm_backward(dy, xhat, rstd, gm)
    assert torch.equal(hip.layer_norm_forward(x, gm, bt, eps, save=False)[0], y)
    return dict(y=y, xhat=xhat, rstd=rstd, dx=dx, dgamma=dg, dbeta=db)


@gpu
@pytest.mark.parametrize('cols', LN_COLS)
def test_layer_norm_vs_float64(cols):
    """hip.layer_norm_forward / _backward over rows x eps, ordinary, constant and mean-1e4 rows mixed (rows = 1: each kind on its own): y, xhat, rstd, dx, d gamma,
    d beta by the yardstick; the save=False path returns the same y bit for bit.  Constant rows are exempt from the dx yardstick, where both sides amplify rounding by
    1 / sqrt(eps): there dx is held to the float32 statement with sequential sums."""
    miss = []
    for rows in LN_ROWS:
        for kinds in (LS.LN_KINDS if rows == 1 else [None]):
            c = LS.layer_norm_case(rows, cols, seed=cols + rows, kinds=kinds)
            const = _d(c.kind == 1)
            for eps in LN_EPS:
                got, r32, r64 = _ln_device(c, eps), LS.layer_norm_grads(c, eps, F32, DEV), LS.layer_norm_grads(c, eps, F64, DEV)
                label = f'cols {cols} rows {rows} {kinds or "mixed"} eps {eps:g}'
                for name in ('y', 'xhat', 'rstd', 'dgamma', 'dbeta'):
                    miss += _held('layer_norm', f'{name} {label}', got[name], r32[name], r64[name])
                if (~const).any():
                    miss += _held('layer_norm', f'dx {label}', got['dx'][~const], r32['dx'][~const], r64['dx'][~const])
                if const.any():
                    s32 = LS.layer_norm_grads(c, eps, F32, DEV, sequential=True)
                    miss += _held('layer_norm', f'dx (constant rows, sequential float32) {label}', got['dx'][const], s32['dx'][const], r64['dx'][const])
                    assert not got['xhat'][const].any() and not r64['xhat'][const].any()
    assert not miss, miss


@gpu
@pytest.mark.parametrize('mask', ['on', 'off', 'mixed'])
@pytest.mark.parametrize('rows', HEADS_ROWS)
def test_heads_epilogue_vs_float64(rows, mask):
    """training.HeadsEpilogue: R_next, eps_pos, d eps_crd, d eps_rot by the yardstick, eps_rot rows from exact zeros to 1e6; d eps_crd exactly zero off the mask;
    dR_next = None and deps_pos = None each equal an explicit zero tensor bit for bit."""
    from ab_opt_amd import training, hip
    c = LS.heads_case(rows, mask, seed=rows)
    r32, r64 = LS.heads_epilogue(c, F32, DEV), LS.heads_epilogue(c, F64, DEV)
    R, gen, wR, wp = _d(c.R), _d(c.gen), _d(c.wR), _d(c.wp)
    crd, rot = _d(c.eps_crd).requires_grad_(), _d(c.eps_rot).requires_grad_()
    Rn, ep = training.HeadsEpilogue.apply(R, crd, rot, gen)
    ((Rn * wR).sum() + (ep * wp).sum()).backward()
    miss = []
    for name, got in (('R_next', Rn.detach()), ('eps_pos', ep.detach()), ('d_crd', crd.grad), ('d_rot', rot.grad)):
        assert torch.isfinite(got).all(), name
        miss += _held('heads_epilogue', f'{name} rows {rows} {mask}', got, r32[name], r64[name])
    assert not crd.grad[~gen].any() and not ep.detach()[~gen].any()
    assert torch.equal(Rn.detach()[_d(c.size == 0)], R[_d(c.size == 0)])
    with torch.no_grad():
        for dR, dp in ((None, wp), (wR, None), (None, None)):
            a = hip.heads_epilogue_backward(R, rot, gen, dR, dp)
            b = hip.heads_epilogue_backward(R, rot, gen, torch.zeros_like(wR) if dR is None else dR, torch.zeros_like(wp) if dp is None else dp)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not miss, miss
