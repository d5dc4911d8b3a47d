"""encode() off the 64-pair strip grid and on samples with holes: csrc/embed.hip against the layered float64 statement of
tests/encode_statement.py.

pair_embed_kernel / pair_embed_backward_kernel give one wave a strip of 64 pairs (i, j0 .. j0 + 63); the lengths here leave a strip with
1 or 2 live pairs (L = 65, 130), make the unit count no multiple of the four waves of a workgroup (3 x 65 x 2 = 390), and go down to L = 1.
The inputs (encode_statement.hard_batch) have absent CA / N / C atoms inside a sample, a numbering gap, two chains, generated rows in
two runs and both situations of the structure mask's wrap-around.

How each part is pinned:
  forward, residue features   per element against float64, by the yardstick of test_encode_hip_vs_autograd_statement: no further from the
                              float64 value than 1.5 x the float32 torch statement is
  backward kernel             per pair with the device's own ReLU gates and T, where it is linear: no further from float64 than 2 x the float32
                              evaluation of the same chain
  host contractions           float64 einsum / index_add_ of the device's own dys, acts, G, ds, at the project's product and summation bounds
  two invariances             bit for bit: padding the batch further, and whatever lies in absent rows

The tests of the first section run on the CPU (not marked gpu): they check the statement itself against plain_statement and torch.autograd.
"""
import functools

import pytest
import torch

import plain_statement
import encode_statement as ES
from yardstick import yardstick as _yardstick
from conftest import AttrDict
from ab_opt_amd.utils import synth

gpu = pytest.mark.gpu
DEV = torch.device('cuda:0')
ATOM_CA = 1
F_ = 128              # res_feat_dim

# The float32 torch statements are evaluated on at least this many pair rows (the batch repeated along N, the first copy kept).  Measured
# on the MI355X: at the 1 .. 4 pair rows of the smallest cases torch.nn.functional.linear comes out 1.5 .. 3.5 x closer to float64 than at the
# sizes the model runs at (presumably a small-M kernel that reduces along K as a tree), so its error there would not measure what
# sequential float32 accumulation -- the MFMA chain's, or the same library's at a few thousand rows -- can reach.
MIN_ROWS = 4096

SHAPES = [(1, (1,)), (2, (2, 1)), (3, (17, 16, 9)), (2, (63, 40)), (3, (65, 64, 33)), (2, (130, 129))]
ALL_FLAGS = [(True, True), (False, True), (False, False)]          # (remove_structure, remove_sequence)
CASES = []
for _N, _lengths in SHAPES:
    for _res in ('full', 'backbone+CB'):
        for _flags in (ALL_FLAGS if max(_lengths) in (65, 130) else ALL_FLAGS[:1]):
            CASES.append((_N, _lengths, _res, _flags, 'abdock'))
CASES.append((3, (65, 64, 33), 'full', (True, False), 'abdesign'))          # the hotspot embedding
_id = lambda c: f"{c[4]}-{'x'.join(map(str, c[1]))}-{'A15' if c[2] == 'full' else 'A5'}-{int(c[3][0])}{int(c[3][1])}"
each_case = pytest.mark.parametrize('case', CASES, ids=[_id(c) for c in CASES])


@functools.lru_cache(maxsize=None)
def _models(flavour, resolution, device):
    """A fresh model (not the session's cached one) with hash-filled weights and non-zero distance coefficients, and its float64 copy."""
    from ab_opt_amd import get_model
    cfg = synth.cfg_abdock(10)
    cfg['resolution'] = resolution
    if flavour == 'abdesign':
        for k in ('num_bins', 'dist_min', 'dist_max'):
            cfg.pop(k)
        cfg['diffusion'].pop('obj')
    m = synth.fill_module_(get_model(AttrDict(cfg)).eval(), seed=17)
    with torch.no_grad():
        m.pair_embed.aapair_to_distcoef.weight.copy_(synth.hash_tensor(tuple(m.pair_embed.aapair_to_distcoef.weight.shape), 23, scale=2.0))
    m64 = get_model(AttrDict(cfg)).eval()
    m64.load_state_dict(m.state_dict())
    return m.to(device), m64.to(device).double()


def _inputs(N, lengths, resolution, flags, flavour, device):
    batch = ES.hard_batch(N, list(lengths), resolution, seed=5)
    if flavour == 'abdesign':
        batch['hotspot'] = ((synth.hash_tensor((N, max(lengths)), 31) + 0.5) * 2.99).long() * batch['mask'].long()
    batch = {k: v.to(device) for k, v in batch.items()}
    ctx = batch['mask_heavyatom'][:, :, ATOM_CA] & ~batch['generate_flag']
    return batch, (ctx if flags[0] else None), (ctx if flags[1] else None)


def _as64(batch):
    return {k: (v.double() if v.dtype == torch.float32 else v) for k, v in batch.items()}


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


# ------------------------------------------------------------------------------------------ the statement's own checks (CPU, float64)
SELF = [((3, (17, 16, 9), 'full', (True, True), 'abdock')), ((3, (17, 16, 9), 'backbone+CB', (False, True), 'abdock')),
        ((2, (2, 1), 'full', (False, False), 'abdock')), ((2, (33, 20), 'full', (True, False), 'abdesign'))]
self_case = pytest.mark.parametrize('case', SELF, ids=[_id(c) for c in SELF])


def test_hard_batch_builds_every_case():
    """hard_batch asserts what each case is for; the lengths of the device tests all build, and the largest has the strips the issue names."""
    for N, lengths in SHAPES:
        for res in ('full', 'backbone+CB'):
            b = ES.hard_batch(N, list(lengths), res, seed=5)
            assert b['aa'].shape == (N, max(lengths)) and b['mask'].sum(1).tolist() == list(lengths)
    assert 3 * 65 * 2 % 4 != 0


@self_case
def test_statement_pair_layers_equal_plain_statement(case):
    _, m64 = _models(case[4], case[2], 'cpu')
    batch, sm, qm = _inputs(*case, 'cpu')
    b64 = _as64(batch)
    with torch.no_grad():
        lay = ES.pair_layers(m64.pair_embed, b64, sm, qm)
        ref = plain_statement.pair_embedding(m64.pair_embed, b64['aa'], b64['res_nb'], b64['chain_nb'], b64['pos_heavyatom'], b64['mask_heavyatom'],
                                             structure_mask=sm, sequence_mask=qm)
    assert lay['out'].dtype == torch.float64 and _rel(lay['out'], ref) <= 1e-12
    assert torch.equal(lay['h0'], torch.relu(lay['pre_d0'])) and torch.equal(lay['o1'], torch.relu(lay['pre_o1']))
    assert lay['f_dih'].shape[-1] == 26 and lay['G'].shape[-2:] == (m64.pair_embed.max_num_atoms,) * 2
    assert torch.equal(lay['out'] != 0, (lay['out'] != 0) & lay['mpair'][..., None])


def _statement_backward(case):
    _, m64 = _models(case[4], case[2], 'cpu')
    batch, sm, qm = _inputs(*case, 'cpu')
    pe = m64.pair_embed
    lay = ES.pair_layers(pe, _as64(batch), sm, qm)                        # under autograd: the parameters are float64 leaves
    dout = synth.hash_tensor(tuple(lay['out'].shape), 77).double()
    loss = (lay['out'] * dout).sum()
    dys, ds = ES.pair_backward_chain(pe, dout, ES.gates_of(ES.pack_acts(lay).detach()), lay['T'].detach(), lay['mpair'])
    return pe, batch, qm, lay, loss, dys, ds


@self_case
def test_statement_backward_chain_equals_autograd(case):
    pe, batch, qm, lay, loss, dys, ds = _statement_backward(case)
    ref = torch.autograd.grad(loss, [lay['pre_o1'], lay['pre_o0'], lay['pre_d1'], lay['pre_d0'], lay['sp']])
    for name, a, b in zip(ES.DY_NAMES[1:] + ('softplus(coef)',), dys[1:] + [ds], ref):
        assert b.abs().max().item() > 0 or max(batch['aa'].shape) < 3, name
        assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item(), name


@self_case
def test_statement_param_grads_equal_autograd(case):
    pe, batch, qm, lay, loss, dys, ds = _statement_backward(case)
    names, params = zip(*[(n, p) for n, p in pe.named_parameters()])
    ref = dict(zip(names, torch.autograd.grad(loss, params)))
    with torch.no_grad():
        got = ES.pair_param_grads(pe, batch, torch.cat(dys, -1), ES.pack_acts(lay), lay['G'], ds, qm=qm)
    assert sorted(got) == sorted(ref) and len(got) == 13
    for n in names:
        assert (got[n] - ref[n]).abs().max().item() <= 1e-10 * max(ref[n].abs().max().item(), 1e-300), n


# ------------------------------------------------------------------------------------------ device
class _Case:
    """One (shape, resolution, flags, flavour): inputs, statements and device results, each computed once and shared by the tests below
    (nobody writes to them)."""

    def __init__(self, N, lengths, resolution, flags, flavour):
        from ab_opt_amd import hip
        self.flags, self.flavour = flags, flavour
        self.m, self.m64 = _models(flavour, resolution, 'cuda:0')
        self.batch, self.sm, self.qm = _inputs(N, lengths, resolution, flags, flavour, DEV)
        self.b64 = _as64(self.batch)
        self.N, self.L, self.A = N, max(lengths), self.m.pair_embed.max_num_atoms
        self.mres = self.batch['mask_heavyatom'][:, :, ATOM_CA]
        self.mpair = self.mres[:, :, None] & self.mres[:, None, :]
        self.eye = torch.eye(self.L, dtype=torch.bool, device=DEV)[None].expand(N, -1, -1)
        self.inp, self._keep = self.encode_inputs(self.batch)
        self.w = self.m.pair_embed._hip_weights()
        self.hip = hip

    def encode_inputs(self, batch):
        from ab_opt_amd import hip
        ctx = batch['mask_heavyatom'][:, :, ATOM_CA] & ~batch['generate_flag']
        return hip.encode_inputs(batch['aa'], batch['res_nb'], batch['chain_nb'], batch['pos_heavyatom'], batch['mask_heavyatom'], self.A,
                                 fragment_type=batch['fragment_type'], hotspot=batch.get('hotspot'),
                                 structure_mask=ctx if self.flags[0] else None, sequence_mask=ctx if self.flags[1] else None)

    @property
    def reps(self):
        return max(1, -(-MIN_ROWS // (self.N * self.L * self.L)))

    def rep(self, x):
        """x repeated along N so that the float32 statement runs on MIN_ROWS pair rows at least."""
        return None if x is None else x.repeat((self.reps,) + (1,) * (x.dim() - 1))

    @functools.cached_property
    def ref(self):
        """plain_statement.encode in float32 and float64."""
        with torch.no_grad():
            return ([t.detach()[:self.N] for t in plain_statement.encode(self.m, {k: self.rep(v) for k, v in self.batch.items()}, *self.flags)],
                    [t.detach() for t in plain_statement.encode(self.m64, dict(self.b64), *self.flags)])

    @functools.cached_property
    def layers(self):
        with torch.no_grad():
            l32 = ES.pair_layers(self.m.pair_embed, {k: self.rep(v) for k, v in self.batch.items()}, self.rep(self.sm), self.rep(self.qm))
            return {k: v[:self.N] for k, v in l32.items()}, ES.pair_layers(self.m64.pair_embed, self.b64, self.sm, self.qm)

    @functools.cached_property
    def fwd(self):
        """the training dump: out, acts, G, T."""
        return self.hip.pair_embed_forward(self.inp, self.w, save_activations=True, save_T=True)

    @functools.cached_property
    def dout(self):
        return synth.hash_tensor((self.N, self.L, self.L, 64), 77).to(DEV)

    @functools.cached_property
    def bwd(self):
        return self.hip.pair_embed_backward(self.inp, self.w, self.dout, self.fwd[1], colsum=True)


@functools.lru_cache(maxsize=None)
def _case(case):
    return _Case(*case)


def _own_sign(ref, like, eye, freq):
    """f_dih of the float64 statement with the two angles of the i == j pairs at the sign `like` has them.  Both are degenerate there --
    (C_i, N_i, CA_i, C_i) and (N_i, CA_i, C_i, N_i) repeat a point, the normals are parallel, the cosine clamps -- so each is
    s x acos(0.999999) with s the sign of an exactly-zero triple product: -1, 0 or +1 by rounding, implementation-defined in the reference
    itself (float64 often gets exactly 0).  Pairs the structure mask removed stay zero."""
    on = eye & (ref != 0).any(-1)
    out = ref.clone()
    theta = torch.acos(torch.tensor(0.999999, dtype=ref.dtype, device=ref.device))
    for a in (0, 13):
        x = (torch.sign(like[..., a]).to(ref.dtype) * theta)[..., None]
        enc = torch.cat([x, torch.sin(x * freq), torch.cos(x * freq)], dim=-1)
        out[..., a:a + 13] = torch.where(on[..., None], enc, ref[..., a:a + 13])
    return out


@gpu
@each_case
def test_encode_forward_vs_float64(case):
    """(a) res_feat, pair_feat, R, p of m.encode, inference and training path, against the float64 statement; masked pairs and absent residues
    exactly zero; the training path's pair_feat, R and p equal the inference path's bit for bit (res_feat runs its MLP on another GEMM kernel
    there and is held to the float64 yardstick like the inference path's)."""
    c = _case(case)
    with torch.no_grad():
        out = c.m.encode(dict(c.batch), *c.flags)
    with torch.enable_grad():
        out_train = [t.detach() for t in c.m.encode(dict(c.batch), *c.flags)]
    r32, r64 = c.ref
    off = ~c.eye[..., None]
    # i == j: the psi-like dihedral (N_i, CA_i, C_i, N_i) carries the sign of an exactly-zero triple product, implementation-defined in the
    # reference itself: the diagonal gets the looser bound of test_encode_hip_vs_autograd_statement
    miss = []
    for path, o in (('inference', out), ('training', out_train)):
        for name, a, b32, b64 in zip(('res_feat', 'pair_feat', 'R', 'p'), o, r32, r64):
            miss += _yardstick(f'{path} {name}', a, b32, b64, where=off if name == 'pair_feat' else None, loose_vs32=2e-3)
        assert not o[1][~c.mpair].any() and not o[0][~c.mres].any()
    assert not miss, miss
    for name, a, b in zip(('pair_feat', 'R', 'p'), out[1:], out_train[1:]):
        assert torch.equal(a, b), name


@gpu
@each_case
def test_pair_embed_training_dump_vs_float64(case):
    """(a) the five activation tiles, G and T of abopt_pair_embed_forward's training dump against pair_layers, on every j < L; padding columns zero.

    Finding: f_dih at lengths [63, 40] missed this yardstick (max error 1.200e-04 against 1.5 x 7.644e-05 + 1e-6) while the kernel took the angle
    through acos as the reference does: an off-diagonal pair 2.5e-3 rad from zero, beside the clamp, where acos amplifies rounding 400 x.
    dihedral_from_four_points takes the magnitude through atan2 since; the tile's error is now 2.5e-05 there."""
    c = _case(case)
    out, acts, G, T = c.fwd
    l32, l64 = c.layers
    off = ~c.eye[..., None]
    with torch.no_grad():
        assert torch.equal(out, c.m.encode(dict(c.batch), *c.flags)[1])
    miss = []
    for k, (lo, hi) in ES.ACT_SLICES.items():
        got = acts[..., lo:hi]
        if k == 'f_dih':          # every element, the i == j pairs against the statement at their own sign of the degenerate angle
            freq = c.m64.pair_embed.dihedral_embed.freq_bands
            miss += _yardstick(k, got, l32[k], _own_sign(l64[k], got, c.eye, freq), r64_for32=_own_sign(l64[k], l32[k], c.eye, freq))
        else:                     # o0, o1 depend on that sign through out_mlp.0: their diagonal gets the looser bound
            miss += _yardstick(k, got, l32[k], l64[k], where=off if k in ('o0', 'o1') else None, loose_vs32=2e-3)
    assert acts[..., 154:160].abs().max().item() == 0
    A = c.A
    for name, x in (('G', G), ('T', T)):
        x = x.view(c.N, c.L, c.L, A, 16)
        assert x[..., A:].abs().max().item() == 0, name
        miss += _yardstick(name, x[..., :A], l32[name], l64[name])
    assert not miss, miss
    # pairs of absent atoms are exact zeros in G
    matom = c.batch['mask_heavyatom'][:, :, :A]
    am = matom[:, :, None, :, None] & matom[:, None, :, None, :]
    assert G.view(c.N, c.L, c.L, A, 16)[..., :A][~am].abs().max().item() == 0


def _residue_weights(c):
    from ab_opt_amd import hip
    re_ = c.m.residue_embed
    t = [x.detach().contiguous() for x in (re_.aatype_embed.weight, re_.type_embed.weight, re_.dihed_embed.freq_bands)]
    hs = re_.hotspot_embed.weight.detach().contiguous() if re_.hotspot_embed is not None else None
    w = hip.ResidueEmbedWeights(hip.ptr(t[0], torch.float32), hip.ptr(t[1], torch.float32), hip.ptr(hs, torch.float32, optional=True),
                                hip.ptr(t[2], torch.float32), *([None] * 8))
    in_dim = F_ + 22 * c.A * 3 + 39 + F_ + (F_ if hs is not None else 0)
    return w, in_dim, t + [hs]


@gpu
@each_case
def test_residue_features_vs_float64(case):
    """(b) abopt_residue_features elementwise against the float64 statement of the MLP's input; the dihedral block is non-zero exactly where the
    chain-break mask (consecutive numbers, same chain, PREVIOUS residue present) and the rolled structure mask (wraps at L) say so."""
    c = _case(case)
    w, in_dim, keep = _residue_weights(c)
    feat, R, p = c.hip.residue_features(c.inp, w, in_dim)
    feat = feat.reshape(c.N, c.L, in_dim)
    with torch.no_grad():
        l32 = ES.residue_layers(c.m.residue_embed, c.batch, c.sm, c.qm, hotspot=c.batch.get('hotspot'))
        l64 = ES.residue_layers(c.m64.residue_embed, c.b64, c.sm, c.qm, hotspot=c.batch.get('hotspot'))
    assert l64['feat'].shape[-1] == in_dim
    miss = _yardstick('residue features', feat, l32['feat'], l64['feat']) + _yardstick('R', R, c.ref[0][2], c.ref[1][2])
    assert not miss, miss
    assert torch.equal(p, c.ref[0][3])
    live = l64['mdih'] if l64['dm'] is None else l64['mdih'] & l64['dm'][..., None]              # (N, L, 3)
    o = F_ + 22 * c.A * 3
    dih = feat[..., o:o + 39].reshape(c.N, c.L, 3, 13)
    assert torch.equal((dih[..., 7:] != 0).all(-1), live) and torch.equal((dih != 0).any(-1), live)       # cos(x f) is never 0: the mask, exactly
    if c.L >= 17:
        assert live.any() and (~live).any()
        if c.sm is not None:                                        # residue 0's psi: kept where residue L - 1 is present context, dropped where it is generated
            assert live[:, 0, 2].any() and (~live[:, 0, 2]).any()


@gpu
@each_case
def test_pair_embed_backward_per_pair_vs_float64(case):
    """(c) abopt_pair_embed_backward per pair with the device's own gates and T: with the gates fixed the chain is linear in d out, so no ReLU
    kink is involved and every element of every j < L is compared.  Bound: 2 x the error of the same chain evaluated in float32 torch
    (+1e-7 of the group's maximum); the factor covers the MFMA's other accumulation order.  Measured worst ratios: DESIGN.md section 4."""
    c = _case(case)
    out, acts, G, T = c.fwd
    dys, ds, db = c.bwd
    dys_t, ds_t = c.hip.pair_embed_backward(c.inp, c.w, c.dout, acts, T)
    assert torch.equal(dys, dys_t) and torch.equal(ds, ds_t)                      # T recomputed in the kernel = T read from the forward's dump
    A = c.A
    gates, Tu = ES.gates_of(acts), ES.unpad_atoms(T, A)
    with torch.no_grad():
        y32, s32 = ES.pair_backward_chain(c.m.pair_embed, c.rep(c.dout), {k: c.rep(v) for k, v in gates.items()}, c.rep(Tu), c.rep(c.mpair))
        y32, s32 = [y[:c.N] for y in y32], s32[:c.N]
        y64, s64 = ES.pair_backward_chain(c.m64.pair_embed, c.dout.double(), gates, Tu.double(), c.mpair)
    assert ds.view(c.N, c.L, c.L, A, 16)[..., A:].abs().max().item() == 0
    groups = [(ES.DY_NAMES[k], dys[..., 64 * k:64 * (k + 1)], y32[k], y64[k]) for k in range(5)] + [('ds', ES.unpad_atoms(ds, A), s32, s64)]
    miss = []
    for name, got, b32, b64 in groups:
        top = b64.abs().max().item()
        e_hip, e_t32 = (got.double() - b64).abs().max().item(), (b32.double() - b64).abs().max().item()
        print(f'RATIO {_id(case)} {name}: hip {e_hip:.3e} t32 {e_t32:.3e} max {top:.3e} ratio {e_hip / max(e_t32, 1e-300):.3f}')
        if not e_hip <= 2 * e_t32 + 1e-7 * top:
            miss.append(f'{name}: {e_hip:.3e} > 2 x {e_t32:.3e} + 1e-7 x {top:.3e}')
        assert top > 0 or c.L < 17, name
    assert not miss, miss
    # the 320 column sums against the float64 sum of the device's own dys (the summation bound of test_bucket_colsum_vs_index_add)
    ref = dys.double().reshape(-1, ES.PAIR_DY).sum(0)
    assert (db.double() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


@gpu
@each_case
def test_pair_embed_host_contractions_vs_float64(case):
    """(d) the parameter gradients of m.pair_embed under autograd against pair_param_grads in float64 on the device's own dys, acts, G, ds
    (the kernels are deterministic: (c) asserts the repeat).  Products: 2e-6 x (|a|^T |b|).max() (test_gemm_tn_grouped_vs_fp64); bucket
    sums: 2e-5 x max (test_bucket_colsum_vs_index_add); a bucket sum s followed by a small product s E: both bounds chained,
    2e-5 max|s| max_k sum_e |E[e, k]| + 2e-6 (|s| |E|).max().  Pins the relative-position buckets (clamp at +-32, other-chain pairs skipped)
    and the [A][16] -> A*A un-padding at A = 5 and A = 15."""
    c = _case(case)
    pe, b, A = c.m.pair_embed, c.batch, c.A
    out, acts, G, T = c.fwd
    dys, ds, db = c.bwd
    pe.zero_grad(set_to_none=True)
    with torch.enable_grad():
        pf = pe(aa=b['aa'], res_nb=b['res_nb'], chain_nb=b['chain_nb'], pos_atoms=b['pos_heavyatom'], mask_atoms=b['mask_heavyatom'],
                structure_mask=c.sm, sequence_mask=c.qm)
        assert torch.equal(pf.detach(), out)
        pf.backward(c.dout)
    got = {n: p.grad.double() for n, p in pe.named_parameters()}
    pe.zero_grad(set_to_none=True)
    Gu, dsu = ES.unpad_atoms(G, A), ES.unpad_atoms(ds, A)
    ref = ES.pair_param_grads(pe, b, dys, acts, Gu, dsu, qm=c.qm)
    assert sorted(got) == sorted(ref)
    w = ES.pair_weights(pe, torch.float64)
    M = c.N * c.L * c.L
    y, a = dys.double().reshape(M, -1), acts.double().reshape(M, -1)
    do2, do1, do0, dh1, dh0 = y.split(64, dim=1)
    aap, rel, same = (t.reshape(M) for t in ES.pair_indices(pe, b, c.qm))
    z = lambda r, k: torch.zeros(r, k, dtype=torch.float64, device=DEV)
    s_aap = z(22 * 22, 64).index_add_(0, aap, do0)
    s_rel = z(65, 64).index_add_(0, rel[same], do0[same])
    s_ds = z(22 * 22, A * A).index_add_(0, aap, dsu.double().reshape(M, A * A))
    prod = lambda p, q: 2e-6 * (p.abs().t() @ q.abs()).max().item()
    chained = lambda s, E: 2e-5 * s.abs().max().item() * E.abs().sum(0).max().item() + 2e-6 * (s.abs().t() @ E.abs()).max().item()
    top_db = y.sum(0).abs().max().item()
    tol = {'out_mlp.4.weight': prod(do2, a[:, 224:288]), 'out_mlp.2.weight': prod(do1, a[:, 160:224]), 'distance_embed.2.weight': prod(dh1, a[:, :64]),
           'distance_embed.0.weight': prod(dh0, Gu.double().reshape(M, A * A)),
           'aa_pair_embed.weight': chained(s_aap.t(), w['wo0'][:, :64]), 'relpos_embed.weight': chained(s_rel.t(), w['wo0'][:, 64:128]),
           'aapair_to_distcoef.weight': 2e-5 * s_ds.abs().max().item()}
    for n in ref:
        if n.endswith('.bias'):
            tol[n] = 2e-5 * top_db
    err = lambda n, sl=slice(None): (got[n][:, sl] - ref[n][:, sl]).abs().max().item()
    for n in ref:
        if n == 'out_mlp.0.weight':                                # [aa-pair table | relpos table x same chain | f_dist | f_dih]
            for name, sl, t in (('aap', slice(0, 64), chained(s_aap, w['E_aap'])), ('rel', slice(64, 128), chained(s_rel, w['E_rel'])),
                                ('dist|dih', slice(128, 218), prod(do0, a[:, 64:154]))):
                print(f'{n}[{name}]: err {err(n, sl):.3e} tol {t:.3e}')
                assert err(n, sl) <= t, (n, name)
            continue
        e = (got[n] - ref[n]).abs().max().item()
        print(f'{n}: err {e:.3e} tol {tol[n]:.3e} max {ref[n].abs().max().item():.3e}')
        assert e <= tol[n], n
    if c.L >= 17:
        r = ref['relpos_embed.weight']
        assert r[0].abs().max().item() > 0 and r[64].abs().max().item() > 0           # both clamps met
        assert (~same).any()                                                          # pairs that went to index -1
        assert ref['aapair_to_distcoef.weight'].abs().max().item() > 0


@gpu
@each_case
def test_residue_table_gradients_vs_index_add(case):
    """(d) d_aa, d_type, d_hot of the residue features' autograd function against index_add_ in float64 (2e-5 x max); padding rows zero."""
    from ab_opt_amd.embed import _ResidueFeaturesFn
    c = _case(case)
    re_, b = c.m.residue_embed, c.batch
    hot = re_.hotspot_embed
    re_.zero_grad(set_to_none=True)
    with torch.enable_grad():
        feat, R, p = _ResidueFeaturesFn.apply(b['aa'], b['res_nb'], b['chain_nb'], b['pos_heavyatom'], b['mask_heavyatom'], b['fragment_type'], b.get('hotspot'),
                                              c.sm, c.qm, c.A, re_.type_embed.padding_idx, None if hot is None else hot.padding_idx,
                                              re_.aatype_embed.weight, re_.type_embed.weight, None if hot is None else hot.weight, re_.dihed_embed.freq_bands)
        dfeat = synth.hash_tensor(tuple(feat.shape), 91).to(DEV)
        feat.backward(dfeat)
    aa = b['aa'] if c.qm is None else torch.where(c.qm, b['aa'], torch.full_like(b['aa'], 20))
    off = feat.shape[1] - F_ - (F_ if hot is not None else 0)
    todo = [('aatype_embed', re_.aatype_embed, aa, 0), ('type_embed', re_.type_embed, b['fragment_type'], off)]
    if hot is not None:
        todo.append(('hotspot_embed', hot, b['hotspot'], off + F_))
    for name, emb, idx, col in todo:
        ref = torch.zeros(emb.weight.shape, dtype=torch.float64, device=DEV).index_add_(0, idx.reshape(-1), dfeat[:, col:col + F_].double())
        if emb.padding_idx is not None:
            assert ref[emb.padding_idx].abs().max().item() > 0 or c.L < 3, name         # the padding row IS looked up: its zero gradient is the module's rule
            assert emb.weight.grad[emb.padding_idx].abs().max().item() == 0, name
            ref[emb.padding_idx] = 0
        assert (emb.weight.grad.double() - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item()), name
    re_.zero_grad(set_to_none=True)


def _padded(batch, extra):
    """The same samples padded further, as collate pads: aa 21, everything else 0 / False (CA absent, res_nb 0)."""
    out = {}
    for k, v in batch.items():
        pad = torch.full((v.shape[0], extra) + tuple(v.shape[2:]), 21 if k == 'aa' else 0, dtype=v.dtype, device=v.device)
        out[k] = torch.cat([v, pad], dim=1)
    return out


@gpu
@each_case
def test_pair_feat_unchanged_by_further_padding(case):
    """(e1) a lane's arithmetic depends on its own pair and on wave-uniform weights only: the same samples padded to L + 1, L + 15, L + 63 give
    the [:, :L, :L] block of pair_feat and of the training dump bit for bit (another strip count, other clamped tail lanes, other base
    pointers).  res_feat is left out: the rolled structure mask wraps at the padded L."""
    c = _case(case)
    L = c.L
    out, acts, G, T = c.fwd
    for extra in (1, 15, 63):
        pb = _padded(c.batch, extra)
        with torch.no_grad():
            assert torch.equal(c.m.encode(dict(pb), *c.flags)[1][:, :L, :L], out), extra
        inp, keep = c.encode_inputs(pb)
        out_p, acts_p, G_p, _ = c.hip.pair_embed_forward(inp, c.w, save_activations=True)
        assert torch.equal(out_p[:, :L, :L], out) and torch.equal(acts_p[:, :L, :L], acts) and torch.equal(G_p[:, :L, :L], G), extra
        assert out_p[:, L:].abs().max().item() == 0 and out_p[:, :, L:].abs().max().item() == 0


@gpu
@pytest.mark.parametrize('case', [c for c in CASES if c[1] != (1,)], ids=[_id(c) for c in CASES if c[1] != (1,)])          # (L = 1 has no absent row)
def test_pair_feat_ignores_what_lies_in_absent_rows(case):
    """(e2) coordinates and residue types of rows whose CA is absent (holes and padding) do not reach pair_feat: large finite values there leave it
    bit-identical.  res_feat is left out: psi of the residue before a hole reads the hole's N by the reference's own rule."""
    c = _case(case)
    absent = ~c.mres
    assert absent.any()
    b = dict(c.batch)
    far = synth.hash_tensor(tuple(b['pos_heavyatom'].shape), 63, scale=2000.0).to(DEV)
    far = far + torch.where(far >= 0, 1e4, -1e4)
    b['pos_heavyatom'] = torch.where(absent[:, :, None, None], far, b['pos_heavyatom'])
    b['aa'] = torch.where(absent, ((synth.hash_tensor(tuple(b['aa'].shape), 64) + 0.5) * 20.99).long().to(DEV), b['aa'])
    assert int(b['aa'].max()) < 21 and torch.isfinite(b['pos_heavyatom']).all() and not torch.equal(b['pos_heavyatom'], c.batch['pos_heavyatom'])
    with torch.no_grad():
        assert torch.equal(c.m.encode(b, *c.flags)[1], c.fwd[0])
