"""Model boundary: `get_model(cfg)` -> nn.Module with forward / sample / optimize.

Drop-in for AbDock/src/models/{_base.py:1-13, diffab.py:19-205} and AbDesign/diffab/models/{_base.py,
diffab.py:19-142}: same registry, constructor cfg keys, method signatures, batch-dict schema, trajectory
layout and state_dict keys.  Everything under `self.diffusion` executes in libabopt_hip.so.
"""
import torch
import torch.nn as nn

from . import hip
from .dpm import FullDPM
from .embed import ResidueEmbedding, PairEmbedding, ATOM_CA

_MODEL_DICT = {}
max_num_heavyatoms = 15
resolution_to_num_atoms = {'backbone+CB': 5, 'full': max_num_heavyatoms}


def register_model(name):
    def decorator(cls):
        _MODEL_DICT[name] = cls
        return cls
    return decorator


def _cfg_get(cfg, key, default=None):
    if hasattr(cfg, 'get'):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def get_model(cfg):
    """_base.py:12-13.  cfg.type 'diffab' resolves to the AbDock flavour when the config carries the prmsd
    keys (`num_bins`), else to the AbDesign flavour; 'diffab_abdock' / 'diffab_abdesign' force one."""
    name = _cfg_get(cfg, 'type')
    if name == 'diffab':
        name = 'diffab_abdock' if _cfg_get(cfg, 'num_bins') is not None else 'diffab_abdesign'
    return _MODEL_DICT[name](cfg)


def generate_mask_from_str(str_input, tensor):
    """'start-end' (1-based, inclusive) -> bool mask like `tensor` (diffab.py:184-205)."""
    start, end = str_input.split('-')
    mask = torch.zeros_like(tensor, dtype=torch.bool)
    mask[..., int(start) - 1:int(end)] = True
    return mask


AA_LETTERS = 'ACDEFGHIKLMNPQRSTVWY'      # residue type k of the kernels = AA_LETTERS[k]: the reference's AA enum (utils/protein/constants.py)


def _aa_bits(letters):
    bits = 0
    for c in letters:
        k = AA_LETTERS.find(c.upper()) if len(c) == 1 else -1
        if k < 0:
            raise ValueError(f'unknown residue type {c!r}: the twenty types are {AA_LETTERS}')
        bits |= 1 << k
    return bits


def aa_allowed_mask(length, exclude='', at=None, device=None):
    """The per-residue sets of allowed types that batch['aa_allowed'] takes, for one complex: int32 (length,), bit k of a word = type AA_LETTERS[k] may be designed there.
    Every position allows all twenty types minus the letters of `exclude`; at = {position: 'letters'} replaces the set at that position (1-based, like `contig`)."""
    mask = torch.full((int(length),), (1 << len(AA_LETTERS)) - 1 & ~_aa_bits(exclude), dtype=torch.int32)
    for pos, letters in (at or {}).items():
        if not 1 <= int(pos) <= length:
            raise ValueError(f'position {pos} is outside 1..{length}')
        mask[int(pos) - 1] = _aa_bits(letters)
    return mask.to(device) if device is not None else mask


# Developability (include/abopt.h: abopt_sequence_liabilities_grouped): the liability classes in the bit order of a flag byte, and the
# Kyte-Doolittle hydropathy (J. Mol. Biol. 157, 1982) of the twenty types in AA_LETTERS order -- in tenths, the exact integers the kernel sums, and as floats.
LIABILITY_NAMES = ('n_glyc', 'deamidation', 'isomerisation', 'cleavage', 'cys', 'met', 'hydrophobic_run')
KD_HYDROPATHY_TENTHS = (18, 25, -35, -35, 28, -4, -32, 45, -39, 38, 19, -35, -16, -35, -45, -8, -7, 42, -9, -13)
KD_HYDROPATHY = tuple(v / 10.0 for v in KD_HYDROPATHY_TENTHS)

# Interface energetics (include/abopt.h: abopt_interface_energy_grouped): the formal charge of each type in AA_LETTERS order plus entry
# 20 ("no type"): K, R = +1, D, E = -1, everything else 0 (His is taken as neutral) -- the conventional value at neutral pH, not a tuned one.
RESIDUE_CHARGE = tuple(1.0 if c in 'KR' else -1.0 if c in 'DE' else 0.0 for c in AA_LETTERS) + (0.0,)


def hydrophobic_contact_table():
    """A PLACEHOLDER pair table for hip.interface_energy_grouped, (21, 21) fp32 on the CPU: -1 where both types are among F, I, L, M, V, W, Y, else 0 (entry 20,
    "no type", is 0 throughout).  It counts hydrophobic contacts with a minus sign; it is NOT a statistical contact potential -- none is shipped, a caller who
    has one passes it as pair_table."""
    h = torch.tensor([1.0 if c in 'FILMVWY' else 0.0 for c in AA_LETTERS] + [0.0])
    return 0.0 - h[:, None] * h[None, :]


# Backbone conformation (include/abopt.h: abopt_backbone_conformation_grouped).  SS_LETTERS[k] names code k of `state`, in the order of
# the reduction H > E > G > I > T > C: helix_4, a bridge of either kind, helix_3, helix_5, inside an n-turn, none of these.  The states are DSSP-LIKE, from
# Kabsch & Sander's patterns on single hydrogen bonds; they are NOT DSSP's (no ladders or sheets, no B / E distinction, no bends, no helix trimming).
SS_LETTERS = 'HEGITC'
RAMA_REGIONS = ((-160.0, -20.0, -120.0, 50.0), (-180.0, -45.0, 90.0, -170.0), (20.0, 120.0, -30.0, 100.0))
"""RAMA_REGIONS: a COARSE default table for hip.rama_regions, three boxes (phi_lo, phi_hi, psi_lo, psi_hi) in degrees, each arc counter-clockwise from lo to hi:
    0  alpha-R  phi -160 ..  -20, psi -120 ..   50
    1  beta     phi -180 ..  -45, psi   90 .. -170  (the psi arc runs through 180 and is 100 degrees wide)
    2  alpha-L  phi   20 ..  120, psi  -30 ..  100
The three boxes are disjoint.  These bounds are THIS LIBRARY'S CONVENTION -- rectangles drawn generously around the three classical basins --, not a published
contour: they are not MolProbity's or any other validation tool's regions, "outlier" here means "in none of these three boxes", and no fraction of outliers
computed with them is comparable with such a tool's."""


def identity_table(match=2, mismatch=-2):
    """The simplest substitution table of hip.align_sequences, (21, 21) int32 on the CPU: `match` on the diagonal, `mismatch` elsewhere;
    entry 20 serves every byte >= 20 ("no type"), which therefore scores `match` against itself -- whether two bytes MATCH is decided on the raw bytes."""
    for what, v in (('match', match), ('mismatch', mismatch)):
        if isinstance(v, bool) or int(v) != v or abs(int(v)) > 32767:
            raise ValueError(f'identity_table: {what} must be an integer within +-32767 (got {v!r})')
    t = torch.full((21, 21), int(mismatch), dtype=torch.int32)
    t.fill_diagonal_(int(match))
    return t


def substitution_table(letters, matrix, scale=2):
    """A caller's substitution matrix as a table of hip.align_sequences, (21, 21) int32 on the CPU: reordered from the caller's alphabet `letters` (a string, one
    letter per row and column of `matrix`; case is ignored) into AA_LETTERS order, multiplied by `scale`, which must make every entry an integer (ValueError
    otherwise: the kernel is integer-only, so halves are carried by scale = 2 and the gaps are scaled with them).  A type the alphabet lacks, and entry 20
    ("no type") unless the alphabet has 'X', gets the minimum of the entries taken, in its whole row and column.  No matrix is shipped.  The reference's
    alignment (BLOSUM62, gaps -10 / -0.5) is, with Biopython installed,
        m = Bio.Align.substitution_matrices.load('BLOSUM62')
        table = substitution_table(m.alphabet, numpy.array(m), scale=2)        # half units
        hip.align_sequences(q, r, table, gap_open=-20, gap_extend=-1)          # the reference's -10 / -0.5 in the same units"""
    letters = [c.upper() for c in letters]
    m = torch.as_tensor(matrix, dtype=torch.float64)
    if len(set(letters)) != len(letters) or any(len(c) != 1 for c in letters):
        raise ValueError(f'substitution_table: the alphabet {"".join(letters)!r} repeats a letter')
    if tuple(m.shape) != (len(letters), len(letters)):
        raise ValueError(f'substitution_table: matrix {tuple(m.shape)} does not fit the alphabet of {len(letters)} letters')
    s = m * float(scale)
    if not torch.isfinite(s).all() or not torch.equal(s, s.round()):
        raise ValueError(f'substitution_table: scale={scale!r} does not make every entry an integer')
    if s.abs().max() > 32767:
        raise ValueError('substitution_table: an entry exceeds +-32767 after scaling')
    src = [letters.index(c) if c in letters else -1 for c in AA_LETTERS + 'X']
    have = [k for k in src if k >= 0]
    if not have:
        raise ValueError(f'substitution_table: the alphabet {"".join(letters)!r} holds none of {AA_LETTERS}')
    low = s[have][:, have].min()
    t = torch.full((21, 21), float(low), dtype=torch.float64)
    for i, a in enumerate(src):
        for j, b in enumerate(src):
            if a >= 0 and b >= 0:
                t[i, j] = s[a, b]
    return t.to(torch.int32)


def alignment_strings(ops, q_row, r_row, qmask=None, rmask=None):
    """The two gapped strings of one alignment, on the host.  ops: one row of hip.align_traceback's `ops` (1 a pair, 2 a query residue
    against a gap, 3 a gap against a reference residue, 0 = beyond the alignment); q_row (na,) and r_row (nb,): the two rows of residue types the pair was traced
    on, type k = AA_LETTERS[k], anything else 'X'; qmask / rmask: their masks (None = all).  -> (query string, reference string), equally long, '-' for a gap.
    ValueError unless ops spells exactly the mask-true residues of both rows."""
    def seq(row, mask):
        row = [int(v) for v in torch.as_tensor(row).reshape(-1).tolist()]
        keep = [True] * len(row) if mask is None else [bool(v) for v in torch.as_tensor(mask).reshape(-1).tolist()]
        if len(keep) != len(row):
            raise ValueError(f'alignment_strings: a mask of {len(keep)} elements on a row of {len(row)}')
        return [AA_LETTERS[v] if 0 <= v < len(AA_LETTERS) else 'X' for v, k in zip(row, keep) if k]
    a, b = seq(q_row, qmask), seq(r_row, rmask)
    word = [int(v) for v in torch.as_tensor(ops).reshape(-1).tolist()]
    while word and word[-1] == 0:
        word.pop()
    if any(v not in (1, 2, 3) for v in word) or sum(v != 3 for v in word) != len(a) or sum(v != 2 for v in word) != len(b):
        raise ValueError(f'alignment_strings: ops does not spell the {len(a)} query and {len(b)} reference residues')
    ia, ib = iter(a), iter(b)
    return ''.join(next(ia) if v != 3 else '-' for v in word), ''.join(next(ib) if v != 2 else '-' for v in word)


ROLE_HOTSPOT, ROLE_REPEL = 1, 2        # the bits of a guide_role word (include/abopt.h: abopt_guide_positions)


def guide_roles(batch_or_length, hotspots=None, repel=None, device=None):
    """The per-residue roles that batch['guide_role'] takes (guided sampling): int32 words, bit 0 = hotspot (the generated residues are
    pulled towards the centroid of these), bit 1 = repeller (every generated residue is pushed out of these residues' radius).
    batch_or_length: a batch dict -> (N, L) like batch['aa'], on its device; or a length -> (length,) for one complex.
    hotspots: 1-based positions like `contig` (an iterable of ints), or a bool mask of the result's shape (or (L,)).
    repel: None; a bool mask; or, with a batch, 'context' (every real residue that is not generated) / 'antigen' (fragment_type 3).
    The kernel ignores the bits of generated and of masked-out residues, so a mask need not be exact there."""
    if isinstance(batch_or_length, dict):
        batch = batch_or_length
        shape, device = tuple(batch['aa'].shape), batch['aa'].device
    else:
        batch, shape = None, (int(batch_or_length),)
    L = shape[-1]
    role = torch.zeros(shape, dtype=torch.int32, device=device)

    def as_mask(name, m):
        m = torch.as_tensor(m, device=role.device)
        if m.dtype != torch.bool or m.shape[-1] != L or m.dim() > len(shape) or (m.dim() == len(shape) and tuple(m.shape) != shape):
            raise ValueError(f'{name}: expected a bool mask of shape {shape} or ({L},), got {m.dtype} {tuple(m.shape)}')
        return m.expand(shape)
    if hotspots is not None:
        if torch.is_tensor(hotspots) and hotspots.dtype == torch.bool:
            hot = as_mask('hotspots', hotspots)
        else:
            hot = torch.zeros(L, dtype=torch.bool)
            for pos in (hotspots.tolist() if torch.is_tensor(hotspots) else hotspots):
                if int(pos) != pos or not 1 <= int(pos) <= L:
                    raise ValueError(f'hotspot position {pos!r} is outside 1..{L}')
                hot[int(pos) - 1] = True
            hot = hot.to(role.device).expand(shape)
        role = role | torch.where(hot, ROLE_HOTSPOT, 0).to(torch.int32)
    if repel is not None:
        if isinstance(repel, str):
            if batch is None or repel not in ('context', 'antigen'):
                raise ValueError(f"repel={repel!r}: 'context' and 'antigen' need a batch dict; otherwise pass a bool mask")
            rm = torch.logical_and(batch['mask'].bool(), ~batch['generate_flag'].bool()) if repel == 'context' else batch['fragment_type'] == 3
        else:
            rm = as_mask('repel', repel)
        role = role | torch.where(rm, ROLE_REPEL, 0).to(torch.int32)
    return role


def generate_random_mask_from(tensor, mask_ratio_min, mask_ratio_max):
    """diffab.py:166-180."""
    ratio = float(torch.empty(1).uniform_(mask_ratio_min, mask_ratio_max))
    return torch.bernoulli(torch.zeros_like(tensor.float()).fill_(ratio)).bool()


class _DiffabBase(nn.Module):
    ABDOCK = True

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        g = lambda k, d=None: _cfg_get(cfg, k, d)
        num_atoms = resolution_to_num_atoms[g('resolution', 'full')]
        F, Cp = g('res_feat_dim'), g('pair_feat_dim')
        self.residue_embed = ResidueEmbedding(F, num_atoms, hotspot=not self.ABDOCK)
        self.pair_embed = PairEmbedding(Cp, num_atoms)
        dcfg = dict(g('diffusion'))
        if self.ABDOCK:
            self.diffusion = FullDPM(F, Cp, **dcfg, num_bins=g('num_bins'), dist_min=g('dist_min'), dist_max=g('dist_max'))
        else:
            self.diffusion = FullDPM(F, Cp, **dcfg, _abdesign=True)

    def encode(self, batch, remove_structure, remove_sequence):
        """diffab.py:39-83 -> res_feat (N,L,F), pair_feat (N,L,L,C), R (N,L,3,3), p (N,L,3)."""
        ctx = torch.logical_and(batch['mask_heavyatom'][:, :, ATOM_CA], ~batch['generate_flag'])
        sm = ctx if remove_structure else None
        qm = ctx if remove_sequence else None
        extra = {} if self.ABDOCK else dict(hotspot=batch.get('hotspot'))
        if not torch.is_grad_enabled():          # sample / optimize / validation: the inference kernels (csrc/embed.hip), nothing saved for a backward
            inp, keep = hip.encode_inputs(batch['aa'], batch['res_nb'], batch['chain_nb'], batch['pos_heavyatom'], batch['mask_heavyatom'],
                                          self.residue_embed.max_num_atoms, fragment_type=batch['fragment_type'], hotspot=extra.get('hotspot'),
                                          structure_mask=sm, sequence_mask=qm)
            res_feat, R, p = self.residue_embed.forward_hip(inp)
            return res_feat, self.pair_embed.forward_hip(inp), R, p
        # training: the same kernels under custom autograd functions (embed.py); the frames come out of the residue-feature kernel
        res_feat, R, p = self.residue_embed.forward_with_frames(aa=batch['aa'], res_nb=batch['res_nb'], chain_nb=batch['chain_nb'],
                                                                pos_atoms=batch['pos_heavyatom'], mask_atoms=batch['mask_heavyatom'],
                                                                fragment_type=batch['fragment_type'], structure_mask=sm, sequence_mask=qm, **extra)
        pair_feat = self.pair_embed(aa=batch['aa'], res_nb=batch['res_nb'], chain_nb=batch['chain_nb'],
                                    pos_atoms=batch['pos_heavyatom'], mask_atoms=batch['mask_heavyatom'],
                                    structure_mask=sm, sequence_mask=qm)
        return res_feat, pair_feat, R, p

    def forward(self, batch):
        """diffab.py:85-112 -> loss dict (AbDock: prmsd, dist, rot, pos, seq; AbDesign: rot, pos, seq)."""
        g = lambda k, d=None: _cfg_get(self.cfg, k, d)
        mask_generate = batch['generate_flag']
        if self.ABDOCK and g('mask_ratio_min', False):
            mask_generate = torch.logical_and(mask_generate, generate_random_mask_from(mask_generate, g('mask_ratio_min'), g('mask_ratio_max')))
            batch['generate_flag'] = mask_generate
        mask_res = batch['mask']
        res_feat, pair_feat, R_0, p_0 = self.encode(batch, remove_structure=g('train_structure', True), remove_sequence=g('train_sequence', True))
        v_0 = hip.so3_log(R_0.detach(), grad_mode=torch.is_grad_enabled())     # frames come from input coordinates: no gradient flows here;
        # the clamp follows autograd state like the reference's log_rotation (so3.py:12-16): validation runs under no_grad
        return self.diffusion(v_0, p_0, batch['aa'], res_feat, pair_feat, mask_generate, mask_res,
                              denoise_structure=g('train_structure', True), denoise_sequence=g('train_sequence', True))

    @torch.no_grad()
    def sample(self, batch, sample_opt={'sample_structure': True, 'sample_sequence': True, 'contig': ''}):
        """diffab.py:114-140."""
        mask_generate = batch['generate_flag']
        if self.ABDOCK and sample_opt.get('sample_sequence', False) and sample_opt['contig'] != '':
            mask_generate = torch.logical_and(mask_generate, generate_mask_from_str(sample_opt['contig'], mask_generate))
            batch['generate_flag'] = mask_generate
        mask_res = batch['mask']
        res_feat, pair_feat, R_0, p_0 = self.encode(batch, remove_structure=sample_opt.get('sample_structure', True),
                                                    remove_sequence=sample_opt.get('sample_sequence', True))
        v_0 = hip.so3_log(R_0, grad_mode=False)
        opt = {k: v for k, v in sample_opt.items() if k != 'contig'}
        # batch['aa_allowed'] (optional, (N, L); no reference counterpart): the types each generated residue may take -- with a contig, at those that remain generated
        # batch['guide_role'] (optional, (N, L); no reference counterpart): hotspot and repeller residues of guided sampling (guide_roles); the knobs ride in sample_opt
        return self.diffusion.sample(v_0, p_0, batch['aa'], res_feat, pair_feat, mask_generate, mask_res, aa_allowed=batch.get('aa_allowed'),
                                     guide_role=batch.get('guide_role'), **opt)

    @torch.no_grad()
    def optimize(self, batch, opt_step, optimize_opt={'sample_structure': True, 'sample_sequence': True}):
        """diffab.py:142-163."""
        mask_generate, mask_res = batch['generate_flag'], batch['mask']
        res_feat, pair_feat, R_0, p_0 = self.encode(batch, remove_structure=optimize_opt.get('sample_structure', True),
                                                    remove_sequence=optimize_opt.get('sample_sequence', True))
        v_0 = hip.so3_log(R_0, grad_mode=False)
        return self.diffusion.optimize(v_0, p_0, batch['aa'], opt_step, res_feat, pair_feat, mask_generate, mask_res, aa_allowed=batch.get('aa_allowed'),
                                       guide_role=batch.get('guide_role'), **optimize_opt)


@register_model('diffab_abdock')
class DiffusionAntibodyDesign(_DiffabBase):
    """AbDock flavour: prmsd head, obj in {pred_x0, pred_noise}, contig masks (AbDock/src/models/diffab.py)."""
    ABDOCK = True


@register_model('diffab_abdesign')
class DiffusionAntibodyDesignAbDesign(_DiffabBase):
    """AbDesign flavour (AbDesign/diffab/models/diffab.py): no prmsd head, noise-prediction objective."""
    ABDOCK = False
