"""Multi-GPU batched sampling: shard independent samples over ranks, one exchange at the end.

The denoising loop has no cross-sample dependence, so ranks never communicate inside it.  The only
exchange is the batched-sampling reduction the reference performs on files written by Ray subprocesses
(AbDock/optimize_ab.py:21-31,66-72; AbDock/src/tools/runner/design_for_pdb.py:326-345): gather every rank's generated
candidates and rank them by "commonness" (AbDock/src/tools/runner/design_for_testset.py:556-589).
One process per GPU, `torch.distributed` backend "nccl" (= RCCL over xGMI) on device tensors; the same code runs on
"gloo" with host tensors in the CPU tests.
"""
import torch
import torch.distributed as dist


def shard_range(n_total, world_size, rank):
    """Contiguous, balanced split of n_total samples: first (n_total % world) ranks get one extra."""
    base, extra = divmod(n_total, world_size)
    start = rank * base + min(rank, extra)
    return start, start + base + (1 if rank < extra else 0)


def shard_batch(batch, world_size, rank):
    n = batch['aa'].shape[0]
    a, b = shard_range(n, world_size, rank)
    return {k: (v[a:b] if isinstance(v, torch.Tensor) and v.shape[:1] == (n,) else v) for k, v in batch.items()}, (a, b)


def candidates_from_positions(p, generate_flag):
    """(N, L, 3) positions + (N, L) mask with the same count per sample -> (N, n_gen, 3)."""
    n_gen = int(generate_flag[0].sum())
    if not bool((generate_flag.sum(1) == n_gen).all()):
        raise ValueError('every sample must generate the same number of residues to be ranked together')
    return p[generate_flag].reshape(p.shape[0], n_gen, 3).contiguous()


def all_gather_candidates(cand, counts=None, group=None):
    """Concatenate (N_r, n, 3) candidate tensors of all ranks in rank order (ragged N_r allowed via `counts`)."""
    world = dist.get_world_size(group)
    if counts is None:
        counts = [cand.shape[0]] * world
    nmax = max(counts)
    pad = cand
    if cand.shape[0] < nmax:
        pad = torch.cat([cand, cand.new_zeros((nmax - cand.shape[0],) + tuple(cand.shape[1:]))], 0)
    pad = pad.contiguous()
    staged = pad.is_cuda and dist.get_backend(group) == 'gloo'          # gloo: the gather goes through host memory
    src = pad.cpu() if staged else pad
    bufs = [torch.empty_like(src) for _ in range(world)]
    dist.all_gather(bufs, src, group=group)
    out = torch.cat([b[:c] for b, c in zip(bufs, counts)], 0)
    return out.to(cand.device) if staged else out


def commonness_score(structs, score_fn=None):
    """score[b] = mean RMSD of structure b to the others * B/(B-1) (lower = more common)."""
    if score_fn is not None:
        return score_fn(structs)
    from . import hip
    return hip.commonness_score(structs)          # HIP kernel; raises on CPU tensors (no fallback)


def rank_commoness(structs, k, score_fn=None):
    """Indices of the k most common structures (design_for_testset.py:575-589)."""
    return torch.topk(commonness_score(structs, score_fn), k=k, largest=False)[1]


def cluster_poses(ca, cutoff, max_clusters=None):
    """Greedy clustering of P docked poses on the device (include/abopt.h: abopt_cluster_poses_grouped): what a docking tool hands
    back instead of a flat list -- one representative per binding mode with its population.  ca (P, n, 3): the poses' CA (all in one frame: the
    distance is the RMSD WITHOUT superposition, as in `commonness_score`); cutoff in Angstrom: a and b are neighbours iff RMSD(a, b) <= cutoff.
    The pose with the most unassigned neighbours (ties: lowest index) becomes a centre, its unassigned neighbours its members; repeat until every
    pose is assigned or max_clusters (optional, >= 1) clusters exist.
    -> dict(label (P,) cluster of every pose (-1: left over at the cap), centre (C,) pose index of every centre, size (C,) members per cluster), int64 on
    the device, in order of discovery (not sorted).  Costs one host read (the number of clusters C).  Raises on CPU tensors (no fallback)."""
    from . import hip
    cutoff = hip.check_cluster_cutoff('cluster_poses: cutoff', cutoff)
    if max_clusters is not None and int(max_clusters) < 1:
        raise ValueError(f'cluster_poses: max_clusters must be >= 1 or None (got {max_clusters!r})')
    if ca.dim() != 3 or ca.shape[0] < 1 or ca.shape[1] < 1 or ca.shape[2] != 3:
        raise ValueError(f'cluster_poses: expected (P, n, 3) poses with P, n >= 1, got {tuple(ca.shape)}')
    out = hip.cluster_poses_grouped(ca, ca.shape[0], cutoff, int(max_clusters or 0))
    C = int(out['count'][0])
    return dict(label=out['label'].long(), centre=out['centre'][0, :C].long(), size=out['size'][0, :C].long())


def cluster_shapes(ca, cutoff, max_clusters=None):
    """`cluster_poses` with every pair of structures superposed before the distance is taken (include/abopt.h:
    abopt_cluster_shapes_grouped): loops are grouped by conformation, whatever frame each lives in -- the designs of several docked poses pooled.  ca (P, n, 3)
    with 3 <= n <= 256; cutoff in Angstrom: a and b are neighbours iff their RMSD after the best proper rotation and translation, over all n points, is
    <= cutoff.  The greedy walk, max_clusters and the result are those of `cluster_poses`.  Costs one host read (C).  Raises on CPU tensors (no fallback)."""
    from . import hip
    cutoff = hip.check_cluster_cutoff('cluster_shapes: cutoff', cutoff)
    if max_clusters is not None and int(max_clusters) < 1:
        raise ValueError(f'cluster_shapes: max_clusters must be >= 1 or None (got {max_clusters!r})')
    if ca.dim() != 3 or ca.shape[0] < 1 or not 3 <= ca.shape[1] <= hip.SIMILARITY_MAX_LEN or ca.shape[2] != 3:
        raise ValueError(f'cluster_shapes: expected (P, n, 3) structures with P >= 1 and 3 <= n <= {hip.SIMILARITY_MAX_LEN}, got {tuple(ca.shape)}')
    out = hip.cluster_shapes_grouped(ca, ca.shape[0], cutoff, int(max_clusters or 0))
    C = int(out['count'][0])
    return dict(label=out['label'].long(), centre=out['centre'][0, :C].long(), size=out['size'][0, :C].long())


def cluster_sequences(seqs, max_mismatch, max_clusters=None):
    """Greedy clustering of S designed sequences on the device (include/abopt.h: abopt_cluster_sequences_grouped): the single-group form
    of `cluster_poses` on the sequence side.  seqs (S, n), any integer dtype, one residue type per entry; a and b are neighbours iff they differ at no more
    than max_mismatch positions (0: identical sequences only).  The sequence with the most unassigned neighbours (ties: lowest index) becomes a centre, its
    unassigned neighbours its members; repeat until every sequence is assigned or max_clusters (optional, >= 1) clusters exist.
    -> dict(label (S,) (-1: left over at the cap), centre (C,), size (C,)), int64 on the device, in order of discovery.  Costs one host read (C).  Raises on
    CPU tensors (no fallback)."""
    from . import hip
    m = hip.check_max_mismatch('cluster_sequences: max_mismatch', max_mismatch)
    if max_clusters is not None and int(max_clusters) < 1:
        raise ValueError(f'cluster_sequences: max_clusters must be >= 1 or None (got {max_clusters!r})')
    if seqs.dim() != 2 or seqs.shape[0] < 1 or seqs.shape[1] < 1:
        raise ValueError(f'cluster_sequences: expected (S, n) sequences with S, n >= 1, got {tuple(seqs.shape)}')
    out = hip.cluster_sequences_grouped(seqs, seqs.shape[0], m, int(max_clusters or 0))
    C = int(out['count'][0])
    return dict(label=out['label'].long(), centre=out['centre'][0, :C].long(), size=out['size'][0, :C].long())


def profile_summary(counts):
    """counts (..., n, 21) of hip.sequence_profile_grouped -> (consensus (..., n) int64: the most frequent of the 20 types, lowest type on a tie;
    entropy (..., n) fp32: -sum p ln p over the 21 bins, p = counts / S, computed in float64).  Pure torch, no host read."""
    # argmax does not promise the first maximum: take the lowest type that reaches the largest count instead
    top = counts[..., :20].amax(-1, keepdim=True)
    types = torch.arange(20, device=counts.device).expand_as(counts[..., :20])
    consensus = torch.where(counts[..., :20] == top, types, 20).amin(-1)
    c = counts.double()
    p = c / c.sum(-1, keepdim=True)
    entropy = -(torch.where(p > 0, p * torch.log(p.clamp_min(1e-300)), torch.zeros_like(p))).sum(-1)
    return consensus, entropy.float()


def sequence_profile(seqs):
    """Per-position composition of S designed sequences (include/abopt.h: abopt_sequence_profile_grouped).  seqs (S, n), any integer dtype.
    -> dict(counts (n, 21) int32: bin t < 20 counts type t, bin 20 everything else; consensus (n,) int64 and entropy (n,) fp32 of `profile_summary`), on the
    device, no host read.  Raises on CPU tensors (no fallback)."""
    from . import hip
    if seqs.dim() != 2 or seqs.shape[0] < 1 or seqs.shape[1] < 1:
        raise ValueError(f'sequence_profile: expected (S, n) sequences with S, n >= 1, got {tuple(seqs.shape)}')
    counts = hip.sequence_profile_grouped(seqs, seqs.shape[0])[0]
    consensus, entropy = profile_summary(counts)
    return dict(counts=counts, consensus=consensus, entropy=entropy)


def backbone_links(chain_nb, res_nb):
    """(..., L) bool: residue r is peptide-bonded to r + 1 as far as the numbering says -- same chain and consecutive residue numbers; the last entry is False.
    Pure torch, any device."""
    link = torch.zeros_like(chain_nb, dtype=torch.bool)
    link[..., :-1] = (chain_nb[..., :-1] == chain_nb[..., 1:]) & (res_nb[..., 1:] == res_nb[..., :-1] + 1)
    return link


def _sides(name, batch, groups):
    """group (G, L) of the two sides a scorer compares: groups='chains': antibody (1) against antigen (2), as DockQ sees them (screen.chain_groups); 'generated':
    the generated residues (1) against every other real residue (2)."""
    from . import screen
    ft = batch['fragment_type']
    if groups == 'chains':
        return screen.chain_groups(ft)
    if groups == 'generated':
        return torch.where(batch['generate_flag'].bool(), 1, torch.where(ft > 0, 2, 0))
    raise ValueError(f"{name}: groups must be 'chains' or 'generated', not {groups!r}")


def interface_geometry(batch, pos, mask, groups='chains', **cutoffs):
    """Clashes, contacts, interface residues and chain breaks of candidate structures of the complexes of `batch` (hip.interface_geometry_grouped; DESIGN.md
    section 6.3).  batch: G complexes (fragment_type, chain_nb, res_nb, generate_flag (G, L)); pos (G*S, L, A, 3), mask (G*S, L, A) or (G, L, A): S candidates of
    each, candidate c belongs to complex c // S.
    groups='chains': antibody (side 1) against antigen (side 2), as DockQ sees them (screen.chain_groups); 'generated': the generated residues (side 1) against
    every other real residue (side 2), bonded neighbours excluded.  cutoffs: clash_cutoff, contact_cutoff, bond_max, want_freq of hip.interface_geometry_grouped;
    the links are those of `backbone_links` (passed with 'generated', and whenever bond_max asks for the breaks)."""
    from . import hip
    grp = _sides('interface_geometry', batch, groups)
    link = None
    if groups == 'generated' or cutoffs.get('bond_max') is not None:
        link = backbone_links(batch['chain_nb'], batch['res_nb'])
    return hip.interface_geometry_grouped(pos, mask, grp, link=link, **cutoffs)


def relax_candidates(batch, pos, mask, move='generated', bond_max=2.0, **knobs):
    """Relax candidate structures of the complexes of `batch` and say what it did in the units the screen reports (hip.relax_grouped).
    batch, pos, mask as for `interface_geometry`.  move: 'generated' -- the residues of generate_flag move; 'antibody' -- every antibody residue moves
    (screen.chain_groups == 1); or a (G, L) bool tensor.  The links are those of `backbone_links`.  knobs: w_bond, w_ca, w_clash, w_tether, clash_cutoff, step,
    max_shift, max_angle, iters, out, max_moved of hip.relax_grouped -- conventional defaults, not tuned ones.
    -> dict of device tensors, N = G*S: pos (N, L, A, 3) and energy (N, 2, 4) of hip.relax_grouped; clashes_before / clashes_after / breaks_before / breaks_after
    (N,) int32 from two `interface_geometry` calls with groups='generated', the same clash_cutoff and bond_max (Angstrom): the generated residues against every
    other real residue, whichever set moved.  A candidate with more moved residues than the bound (max_moved, by default min(L, 256): an antibody of more than 256
    residues with move='antibody') is NOT relaxed and raises nothing -- the count lives on the device; it comes back unchanged with NaN in all of its `energy`:
    check `energy` for NaN.  The screen does not call this: apply it to what optimize_antibody / sample_grouped return.
    No host synchronisation."""
    from . import hip, screen
    if isinstance(move, str):
        if move == 'generated':
            mv = batch['generate_flag'].bool()
        elif move == 'antibody':
            mv = screen.chain_groups(batch['fragment_type']) == 1
        else:
            raise ValueError(f"relax_candidates: move must be 'generated', 'antibody' or a (G, L) tensor, not {move!r}")
    else:
        mv = move
    geom = dict(clash_cutoff=knobs.get('clash_cutoff', 3.0), bond_max=bond_max)
    before = interface_geometry(batch, pos, mask, groups='generated', **geom)              # before the relax: `out` may be pos itself
    res = hip.relax_grouped(pos, mask, mv, link=backbone_links(batch['chain_nb'], batch['res_nb']), **knobs)
    after = interface_geometry(batch, res['pos'], mask, groups='generated', **geom)
    return dict(res, clashes_before=before['clash'], clashes_after=after['clash'], breaks_before=before['breaks'], breaks_after=after['breaks'])


BONDI_RADII = (1.55, 1.70, 1.70, 1.52, 1.70)                    # N, CA, C, O, CB (Bondi 1964: N 1.55, C 1.70, O 1.52 Angstrom)


def slot_radii(A, atoms=5):
    """The default van der Waals radius of each of the A atom slots of a residue, in Angstrom -> (A,) fp32 on the CPU: slots 0-4 are N, CA, C, O, CB with Bondi
    radii 1.55, 1.70, 1.70, 1.52, 1.70; slots >= `atoms` (at most 5) get 0 and so take no part in `buried_surface`.  A rebuilt residue has backbone + CB only
    (geometry.reconstruct_backbone_partially) and the package holds no per-type side-chain atom table, so by default EVERY residue is scored on those five slots:
    a coarse-grained area, comparable between candidates of one complex, not an all-atom SASA.  A caller with a full-atom radius table passes radius= instead."""
    A, atoms = int(A), int(atoms)
    if A < 1 or not 0 <= atoms <= len(BONDI_RADII):
        raise ValueError(f'slot_radii: need A >= 1 and 0 <= atoms <= {len(BONDI_RADII)} (got A={A}, atoms={atoms})')
    r = torch.zeros(A, dtype=torch.float32)
    n = min(A, atoms)
    r[:n] = torch.tensor(BONDI_RADII[:n], dtype=torch.float32)
    return r


def buried_surface(batch, pos, mask, groups='chains', probe=1.4, points=128, radius=None):
    """Buried solvent-accessible surface area (Shrake-Rupley) of candidate structures of the complexes of `batch` (hip.sasa_grouped).
    batch, pos, mask and groups ('chains': antibody against antigen; 'generated': the generated residues against every other real residue) as for
    `interface_geometry`; probe in Angstrom, points = test points per atom; radius (optional; (A,), (L, A) or (G, L, A)): the van der Waals radius per atom slot,
    default `slot_radii(A)` -- five backbone + CB slots for every residue, see there.
    -> dict of device tensors, N = G*S: sasa_res (N, L) fp32, the exposed area of each residue in the complex; bsa_res (N, L) fp32 = its exposed area with the other
    side taken away minus that, >= 0: the paratope and the epitope in A^2; bsa (N,) and sasa (N,) fp32, their sums over the residues (taken in float64, rounded
    once) -- bsa is the buried area of BOTH sides together (some tools report half of it, the "interface area"); pts (N, 4) int32, the point counts of
    hip.sasa_grouped.  No host synchronisation."""
    from . import hip
    grp = _sides('buried_surface', batch, groups)
    if radius is None:
        radius = slot_radii(pos.shape[2] if pos.dim() == 4 else 1)
    return surface_summary(hip.sasa_grouped(pos, mask, grp, radius, probe=probe, points=points))


def surface_summary(sa):
    """pts / area of hip.sasa_grouped -> the dict `buried_surface` returns.  Pure torch, no host read."""
    free, cplx = sa['area'][..., 0], sa['area'][..., 1]
    bsa_res = free - cplx                                                              # free >= complex per atom, so per residue, in the same order of summation
    return dict(sasa_res=cplx, bsa_res=bsa_res, bsa=bsa_res.sum(-1, dtype=torch.float64).float(), sasa=cplx.sum(-1, dtype=torch.float64).float(), pts=sa['pts'])


def liability_summary(out):
    """flags / counts / hyd10 of hip.sequence_liabilities_grouped -> the dict `sequence_liabilities` returns: flags; one count per class under its name of
    model.LIABILITY_NAMES; flagged, positive (K + R), negative (D + E), his, scored (the scored rows that hold a type) and hyd10, all int32; net_charge =
    positive - negative (int32); gravy = hyd10 / (10 scored), one float64 division, NaN where nothing is scored.  Pure torch, no host read."""
    from .model import LIABILITY_NAMES
    counts = out['counts']
    res = dict(flags=out['flags'], **{name: counts[..., k] for k, name in enumerate(LIABILITY_NAMES)})
    res.update(flagged=counts[..., 7], positive=counts[..., 8], negative=counts[..., 9], his=counts[..., 10], scored=counts[..., 11], hyd10=out['hyd10'])
    res['net_charge'] = counts[..., 8] - counts[..., 9]
    scored = counts[..., 11].double()
    res['gravy'] = torch.where(scored > 0, out['hyd10'].double() / (10.0 * scored.clamp_min(1.0)), float('nan'))
    if 'freq' in out:
        res['freq'] = out['freq']
    return res


def sequence_liabilities(seqs, rows=None, link=None, run_min=5):
    """Sequence liabilities of S designed sequences on the device (include/abopt.h: abopt_sequence_liabilities_grouped): N-glycosylation
    sequons (N, not P, S/T), deamidation (N then G/S), isomerisation (D then G/S), Asp-Pro cleavage, Cys, Met and runs of run_min hydrophobic residues (F, I, L,
    M, V, W, Y; 0 = off), with the charged residues and the Kyte-Doolittle hydropathy of the scored rows.  seqs (S, n), any integer dtype, type k =
    model.AA_LETTERS[k]; rows (optional, (n,) bool): the scored positions, e.g. the designed ones -- a motif counts iff one of its residues is a scored row, so a
    sequon completed beside a framework Asn is a liability of the design; link (optional, (n,) bool, `backbone_links`): a motif does not reach over a chain break.
    -> the dict of `liability_summary` (each entry (S,), flags (S, n)), on the device, no host read.  Raises on CPU tensors (no fallback)."""
    from . import hip
    if seqs.dim() != 2 or seqs.shape[0] < 1 or seqs.shape[1] < 1:
        raise ValueError(f'sequence_liabilities: expected (S, n) sequences with S, n >= 1, got {tuple(seqs.shape)}')
    for what, t in (('rows', rows), ('link', link)):
        if t is not None and tuple(t.shape) != (seqs.shape[1],):
            raise ValueError(f'sequence_liabilities: {what} {tuple(t.shape)} must be (n,) = {(seqs.shape[1],)}')
    one = lambda t: None if t is None else t[None]
    return liability_summary(hip.sequence_liabilities_grouped(seqs, seqs.shape[0], rows=one(rows), link=one(link), run_min=run_min))


def patch_summary(patch, nbr, area, group, seqs, weight):
    """patch / nbr of hip.surface_patches_grouped, the area (N, L) they were formed on, group (G, L), seqs (N or G, L) and weight (21,) -> dict: patch_res, nbr;
    sap (N,) = sum of max(patch_i, 0) and patch_max (N,) = the largest patch among the residues that take part (NaN if none does), float64 rounded to fp32 once;
    patch_argmax (N,) int64: its residue, the lowest index on a tie, -1 if nobody takes part; apolar_area / polar_area (N,): the area of the side-1 residues
    whose weight is positive / not positive (a NaN weight is in neither), float64 sums rounded once.  Pure torch, no host read."""
    N, L = patch.shape
    G = group.shape[0]
    part = nbr > 0                                                                     # a residue that takes part is its own neighbour
    sap = patch.clamp_min(0.0).sum(-1, dtype=torch.float64).float()
    masked = torch.where(part, patch, float('-inf'))
    top = masked.amax(-1, keepdim=True)
    idx = torch.arange(L, device=patch.device).expand(N, L)
    arg = torch.where(part & (masked == top), idx, L).amin(-1)                         # argmax does not promise the first maximum
    none = ~part.any(-1)
    w = weight.to(patch.device)[seqs.long().clamp(0, 20)]
    side1 = (group == 1)
    per = lambda t: t if t.shape[0] == N else t.view(G, 1, L).expand(G, N // G if G else 0, L).reshape(N, L)
    w, side1 = per(w), per(side1)
    a64 = area.double()
    zero = torch.zeros_like(a64)
    return dict(patch_res=patch, nbr=nbr, sap=sap, patch_max=torch.where(none, float('nan'), top[:, 0]), patch_argmax=torch.where(none, -1, arg),
                apolar_area=torch.where(side1 & (w > 0), a64, zero).sum(-1).float(), polar_area=torch.where(side1 & (w <= 0), a64, zero).sum(-1).float())


def developability(batch, seqs, pos, mask, rows='generated', probe=1.4, points=128, radius=10.0, run_min=5, weight=None):
    """What a designed antibody is, chemically, and where it lies on the surface: the first scorer that reads a candidate's sequence and
    its structure together.  batch, pos (G*S, L, A, 3) and mask as for `interface_geometry`; seqs (G*S, L), or (G, L) when the S candidates of a complex share
    their sequence (the re-docks of one design), type k = model.AA_LETTERS[k].  Three calls in a chain:
      1. hip.sasa_grouped, antibody (side 1) against antigen (side 2) with `slot_radii` (probe, points as for `buried_surface`);
      2. hip.surface_patches_grouped of the antibody on its FREE area (column 0, the antigen taken away): an aggregation-prone patch matters on the unbound
         antibody, in the vial, whether or not the antigen later covers it (radius in Angstrom; weight (21,), default Kyte-Doolittle);
      3. hip.sequence_liabilities_grouped on `rows` -- 'generated' (generate_flag), 'antibody' (every antibody residue) or a (G, L) mask -- with the links of
         `backbone_links`, one row of results per row of seqs.
    -> dict of device tensors: pts, area of (1); the entries of `patch_summary` (patch_res, nbr, sap, patch_max, patch_argmax, apolar_area, polar_area: per
    candidate); the entries of `liability_summary` (per row of seqs).  The area is that of five backbone + CB slots, so this is a coarse-grained patch score
    comparable between candidates of one complex, NOT a published SAP value; Kyte-Doolittle, 10 A and run_min = 5 are conventional values, not tuned ones, and
    their distribution for trained weights is unmeasured.  No host synchronisation.  The screen does not call this: apply it to what optimize_antibody /
    sample_grouped return."""
    from . import hip, screen
    grp = _sides('developability', batch, 'chains')
    if isinstance(rows, str):
        if rows == 'generated':
            scored = batch['generate_flag'].bool()
        elif rows == 'antibody':
            scored = screen.chain_groups(batch['fragment_type']) == 1
        else:
            raise ValueError(f"developability: rows must be 'generated', 'antibody' or a (G, L) tensor, not {rows!r}")
    else:
        scored = rows
    sa = hip.sasa_grouped(pos, mask, grp, slot_radii(pos.shape[2] if pos.dim() == 4 else 1), probe=probe, points=points)
    free = sa['area'][..., 0].contiguous()
    weight = hip.default_patch_weight(pos.device) if weight is None else weight
    pt = hip.surface_patches_grouped(pos, mask, grp, free, seqs, weight=weight, radius=radius)
    link =backbone_links(batch['chain_nb'], batch['res_nb'])
    per_group = seqs.shape[0] // max(1, grp.shape[0])                                  # rows of seqs per complex: S, or 1 when the sequence is shared
    lb = hip.sequence_liabilities_grouped(seqs, max(1, per_group), rows=scored, link=link, run_min=run_min)
    return dict(sa, **patch_summary(pt['patch'], pt['nbr'], free, grp, seqs, weight), **liability_summary(lb))


def energy_summary(out, group):
    """energy / count of hip.interface_energy_grouped and the group (G, L) they were formed on -> dict: per candidate (N,), each pair counted ONCE (the kernel
    gives a pair's energy to both of its residues, so everything is summed over side 1): hbonds (donor + acceptor), salt_bridges, like_pairs, pair_contacts,
    int32; e_hb, e_elec, e_pair and their sum e_total, float64 sums over side 1 rounded to fp32 once.  freq (G, L) int32: in how many of a group's candidates each
    residue, of either side, holds a hydrogen bond or a salt bridge.  energy_res (N, L, 3) and count_res (N, L, 5): the per-residue arrays.  Pure torch, no host
    read."""
    energy, count = out['energy'], out['count']
    N, L = count.shape[:2]
    G = group.shape[0]
    S = N // G if G else 0
    side1 = (group == 1).view(G, 1, L).expand(G, S, L).reshape(N, L)
    c1 = torch.where(side1[..., None], count, 0).sum(1, dtype=torch.int32)
    e1 = torch.where(side1[..., None], energy.double(), 0.0).sum(1)
    held = (count[..., 0] + count[..., 1] + count[..., 2]) > 0
    return dict(hbonds=c1[:, 0] + c1[:, 1], salt_bridges=c1[:, 2], like_pairs=c1[:, 3], pair_contacts=c1[:, 4], e_hb=e1[:, 0].float(), e_elec=e1[:, 1].float(),
                e_pair=e1[:, 2].float(), e_total=e1.sum(-1).float(), freq=held.view(G, S, L).sum(1, dtype=torch.int32), energy_res=energy, count_res=count)


def interface_energy(batch, seqs, pos, mask, groups='chains', charge=None, pair_table=None, **knobs):
    """Interface energetics of candidate structures of the complexes of `batch` (hip.interface_energy_grouped): whether the contacts
    across an interface are backbone hydrogen bonds and salt bridges or like charges pressed together.  batch, pos (G*S, L, A, 3), mask and groups as for
    `interface_geometry` (A >= 4); seqs (G*S, L), or (G, L) when the candidates of a complex share their sequence, type k = model.AA_LETTERS[k]; charge (21,),
    default model.RESIDUE_CHARGE; pair_table (21, 21), default None = off; the links are those of `backbone_links`; knobs: hb_cutoff, elec_cutoff, salt_cutoff,
    pair_cutoff, eps, d_min of hip.check_interface_energy.
    -> the dict of `energy_summary`, on the device, no host synchronisation.  A score on five backbone + CB slots: no side chains, no water, no screening --
    comparable between candidates of one complex, NOT a binding free energy; the constants are conventional values, not tuned ones, and their distribution for
    trained weights is unmeasured.  The screen does not call this: apply it to what optimize_antibody / sample_grouped return."""
    from . import hip
    grp = _sides('interface_energy', batch, groups)
    out = hip.interface_energy_grouped(pos, mask, grp, seqs, charge=charge, pair_table=pair_table, link=backbone_links(batch['chain_nb'], batch['res_nb']), **knobs)
    return energy_summary(out, grp)


def conformation_summary(out, groups=1):
    """The dict of hip.backbone_conformation_grouped -> it, plus per candidate (N,): scored (int32, the scored rows that take part), helix (H + G + I), strand
    (E) and coil (T + C) as float64 shares of `scored` (NaN where nothing is scored), outliers, cis, cis_nonpro, twisted, hbonds (those whose donor is a scored
    row) as int32; and freq (G, L) int32: in how many of the N / G candidates of each of G = `groups` groups a residue is H or E (with the default every
    candidate is of one group).  Pure torch, no host read."""
    from .hip import BACKBONE_COUNTS
    col = {name: k for k, name in enumerate(BACKBONE_COUNTS)}
    n = out['count']
    scored = n[:, col['part']]
    share = lambda v: torch.where(scored > 0, v.double() / scored.clamp_min(1).double(), float('nan'))
    res = dict(out, scored=scored, helix=share(n[:, col['H']] + n[:, col['G']] + n[:, col['I']]), strand=share(n[:, col['E']]),
               coil=share(n[:, col['T']] + n[:, col['C']]), outliers=n[:, col['outliers']], cis=n[:, col['cis']], cis_nonpro=n[:, col['cis_nonpro']],
               twisted=n[:, col['twisted']], hbonds=n[:, col['hb_donor']])
    N, L = out['state'].shape
    G = int(groups)
    if G < 0 or (N % G if G else N):
        raise ValueError(f'conformation_summary: {N} candidates are not whole groups of {groups} groups')
    res['freq'] = (out['state'] <= 1).view(G, N // G if G else 0, L).sum(1, dtype=torch.int32)      # H or E
    return res


def backbone_conformation(batch, pos, mask, rows='generated', seqs=None, regions=None, hb_cutoff=-0.5):
    """Whether the backbones of candidate structures of the complexes of `batch` are plausible polypeptides (hip.backbone_conformation_grouped; DESIGN.md
    section 6.13): Ramachandran classes, cis / twisted peptides, the peptide bond's geometry and DSSP-LIKE states (NOT DSSP: no ladders or sheets, no B / E
    distinction, no bends, no helix trimming).  batch, pos (G*S, L, A, 3), mask as for `interface_geometry` (A >= 4, L <= 512); rows: 'generated'
    (generate_flag), 'antibody' (every antibody residue) or a (G, L) mask -- the scored residues; every real residue is a hydrogen-bond partner; seqs (G*S, L) or
    (G, L), type k = model.AA_LETTERS[k] (None: no residue is Pro or Gly); the links are those of `backbone_links`; regions: a table of hip.rama_regions, default
    model.RAMA_REGIONS -- this library's coarse three boxes, not a published contour.
    -> the dict of `conformation_summary` with freq (G, L) int32 -- in how many of a group's candidates a residue is H or E -- and phi, psi, omega (G*S, L) in
    degrees, NaN where undefined: torch.atan2 of the kernel's (sin, cos), a convenience that is NOT pinned bitwise (the kernel's cos and sin are).  On the
    device, no host synchronisation.  The default hb_cutoff and regions are conventional values, not tuned ones; what trained weights give is unmeasured.  The
    screen does not call this: apply it to what optimize_antibody / sample_grouped return."""
    from . import hip, screen
    if isinstance(rows, str):
        if rows == 'generated':
            scored = batch['generate_flag'].bool()
        elif rows == 'antibody':
            scored = screen.chain_groups(batch['fragment_type']) == 1
        else:
            raise ValueError(f"backbone_conformation: rows must be 'generated', 'antibody' or a (G, L) tensor, not {rows!r}")
    else:
        scored = rows
    out = hip.backbone_conformation_grouped(pos, mask, scored, seqs=seqs, link=backbone_links(batch['chain_nb'], batch['res_nb']), regions=regions,
                                            hb_cutoff=hb_cutoff)
    res = conformation_summary(out, groups=scored.shape[0])
    t, have = out['torsion'], out['have']
    for k, name in enumerate(('phi', 'psi', 'omega')):
        res[name] = torch.where((have & (1 << k)) != 0, torch.rad2deg(torch.atan2(t[..., 2 * k + 1], t[..., 2 * k])), float('nan'))
    return res


def _front_rows(name, flags, *tensors):
    """The kernels of `similarity` take rows of at most 256 elements.  flags (N, L) bool and tensors (N, L, ...): returned as they are when L <= 256; else each
    row's flagged elements are moved to the front, in order, and the rows cut to 256 -- which costs one host read, to refuse a row with more than 256 of them."""
    from . import hip
    W = hip.SIMILARITY_MAX_LEN
    if flags.shape[1] <= W:
        return (flags,) + tensors
    if int(flags.sum(1).max()) > W:
        raise ValueError(f'{name}: a row selects more than {W} residues')
    order = torch.sort((~flags).to(torch.uint8), dim=1, stable=True)[1][:, :W]
    take = lambda t: torch.gather(t, 1, order.view(order.shape + (1,) * (t.dim() - 2)).expand(order.shape + t.shape[2:]))
    return (take(flags),) + tuple(take(t) for t in tensors)


def similarity(batch, seqs, pos, mask, rows='generated', ref_seqs=None, ref_ca=None, ref_mask=None, table=None, gap_open=-20, gap_extend=-1):
    """How close candidates are to reference sequences and loops of ANY length: the `seqid` and `rmsd` of the reference's eval stage
    (tools/eval/similarity.py), by hip.align_sequences and hip.gapped_rmsd.  batch: G complexes; seqs (G*S, L), type k = model.AA_LETTERS[k]; pos (G*S, L, A, 3)
    with CA in slot 1 and mask (G*S, L, A): S candidates of each, candidate c belongs to complex c // S.  rows: the compared residues of a candidate --
    'generated' (generate_flag), 'antibody' (every antibody residue) or a (G, L) mask; a residue whose CA is masked out is left out of the rmsd.
    Without references every candidate is compared with the NATIVE residues of its own complex on the same rows (batch['aa'], batch['pos_heavyatom']): the
    reference's two eval numbers, every entry (G*S,) -- the launch compares every candidate with every complex's natives and keeps its own, G times the pairs
    kept.  With ref_seqs (R, nb) and / or ref_ca (R, nb, 3), and ref_mask (R, nb) (None = all), every candidate is compared with every reference: every entry
    (G*S, R) -- a panel of known binders, germlines, the designs themselves.  table: default model.identity_table(); the default gaps are the reference's
    -10 / -0.5 in the half units of model.substitution_table(..., scale=2) (no BLOSUM62 is shipped).
    -> dict of device tensors: seqid fp32 (100 matches / columns, -1 at 0 columns), score, matches, columns int32 [with sequences]; rmsd, sd fp32 and m int32
    [with coordinates].  End gaps are free, so sequences whose best overlap scores below 0 are not paired at all (score 0, seqid 0).  No superposition: the
    rmsd is that of the frames pos is given in.  Rows wider than 256 cost one host read, otherwise none.  The screen does not call this: apply it to what
    optimize_antibody / sample_grouped return."""
    from . import hip, screen
    from .model import identity_table
    name = 'similarity'
    G, L = batch['aa'].shape
    if isinstance(rows, str):
        if rows == 'generated':
            scored = batch['generate_flag'].bool()
        elif rows == 'antibody':
            scored = screen.chain_groups(batch['fragment_type']) == 1
        else:
            raise ValueError(f"{name}: rows must be 'generated', 'antibody' or a (G, L) tensor, not {rows!r}")
    else:
        scored = rows.bool()
    if seqs.dim() != 2 or pos.dim() != 4 or mask.dim() != 3 or tuple(scored.shape) != (G, L) or seqs.shape[1] != L or tuple(pos.shape[1:]) != (L, pos.shape[2], 3) \
            or pos.shape[2] < 2 or tuple(mask.shape) != tuple(pos.shape[:3]) or seqs.shape[0] != pos.shape[0] or (seqs.shape[0] % G if G else seqs.shape[0]):
        raise ValueError(f'{name}: expected seqs (G*S, L), pos (G*S, L, A >= 2, 3), mask (G*S, L, A) and rows (G, L) with G = {G}, L = {L}; got '
                         f'{tuple(seqs.shape)}, {tuple(pos.shape)}, {tuple(mask.shape)} and {tuple(scored.shape)}')
    N = seqs.shape[0]
    S = N // G if G else 0
    own = ref_seqs is None and ref_ca is None
    crow = scored.repeat_interleave(S, 0) if S != 1 else scored
    cflag, cseq, cca, cok = _front_rows(name, crow, seqs, pos[:, :, 1], mask[:, :, 1].bool())
    if own:
        rflag, ref_seqs, ref_ca, rok = _front_rows(name, scored, batch['aa'], batch['pos_heavyatom'][:, :, 1], batch['mask_heavyatom'][:, :, 1].bool())
        ref_ca_mask = rflag & rok
    else:
        rflag = ref_mask
        ref_ca_mask = ref_mask
    out = {}
    if ref_seqs is not None:
        al = hip.align_sequences(cseq, ref_seqs, identity_table() if table is None else table, gap_open, gap_extend, qmask=cflag, rmask=rflag)
        cols = al['columns']
        out.update(al, seqid=torch.where(cols > 0, 100.0 * al['matches'].float() / cols.clamp(min=1).float(), torch.full_like(cols, -1, dtype=torch.float32)))
    if ref_ca is not None:
        out.update(hip.gapped_rmsd(cca, ref_ca, qmask=cflag & cok, rmask=ref_ca_mask))
    if own and G:                                                   # a candidate's own complex is column c // S
        col = (torch.arange(N, device=seqs.device) // S)[:, None]
        out = {k: v.gather(1, col)[:, 0] for k, v in out.items()}
    elif own:
        out = {k: v.reshape(0) for k, v in out.items()}
    return out


def aligned_rmsd(batch, seqs, pos, mask, rows='generated', ref_seqs=None, ref_ca=None, ref_mask=None, table=None, gap_open=-20, gap_extend=-1,
                 want_transform=False):
    """How close in SHAPE candidates are to loops of another length, in any frame: the sequences are aligned, the alignment is traced
    (hip.align_traceback) and the CA atoms are superposed on the aligned pairs and measured on them (hip.superposed_rmsd_mapped) -- the twin of `similarity`,
    whose rmsd depends on the frame.  batch, seqs (G*S, L), pos (G*S, L, A, 3), mask (G*S, L, A) and rows as for `similarity`; a residue whose CA is masked out
    leaves the rows, on either side.
    Without references every candidate is compared with the NATIVE residues of its own complex on the same rows: every entry (G*S, ...) -- G*S pairs are
    traced, not G*S x G.  With ref_seqs (R, nb), ref_ca (R, nb, 3) (both) and ref_mask (R, nb) (None = all) every candidate is compared with every reference:
    every entry (G*S, R, ...).  table and gaps as for `similarity`.
    -> dict of device tensors: seqid fp32 (100 matches / columns of THE alignment, -1 at 0 columns), score, matches, columns int32, n_pairs int32 (the aligned
    pairs), rmsd fp32 (-1 with fewer than 3 pairs), qmap (..., L') int16 and ops (..., L' + nb) uint8 as hip.align_traceback returns them [, rot (..., 3, 3)
    and trans (..., 3) with want_transform: reference ~ rot candidate + trans].  L' = L and qmap indexes residues; rows wider than 256 are packed to the front
    first (one host read) and qmap indexes the packed rows.  The screen does not call this: apply it to what optimize_antibody / sample_grouped return."""
    from . import hip, screen
    from .model import identity_table
    name = 'aligned_rmsd'
    G, L = batch['aa'].shape
    if isinstance(rows, str):
        if rows == 'generated':
            scored = batch['generate_flag'].bool()
        elif rows == 'antibody':
            scored = screen.chain_groups(batch['fragment_type']) == 1
        else:
            raise ValueError(f"{name}: rows must be 'generated', 'antibody' or a (G, L) tensor, not {rows!r}")
    else:
        scored = rows.bool()
    if seqs.dim() != 2 or pos.dim() != 4 or mask.dim() != 3 or tuple(scored.shape) != (G, L) or seqs.shape[1] != L or tuple(pos.shape[1:]) != (L, pos.shape[2], 3) \
            or pos.shape[2] < 2 or tuple(mask.shape) != tuple(pos.shape[:3]) or seqs.shape[0] != pos.shape[0] or (seqs.shape[0] % G if G else seqs.shape[0]):
        raise ValueError(f'{name}: expected seqs (G*S, L), pos (G*S, L, A >= 2, 3), mask (G*S, L, A) and rows (G, L) with G = {G}, L = {L}; got '
                         f'{tuple(seqs.shape)}, {tuple(pos.shape)}, {tuple(mask.shape)} and {tuple(scored.shape)}')
    own = ref_seqs is None and ref_ca is None
    if not own and (ref_seqs is None or ref_ca is None):
        raise ValueError(f'{name}: references need both ref_seqs (R, nb) and ref_ca (R, nb, 3)')
    if own and ref_mask is not None:
        raise ValueError(f'{name}: ref_mask selects residues of the references, which are None')
    if not own and (ref_seqs.dim() != 2 or ref_ca.dim() != 3 or tuple(ref_ca.shape) != tuple(ref_seqs.shape) + (3,)):
        raise ValueError(f'{name}: expected ref_seqs (R, nb) and ref_ca (R, nb, 3); got {tuple(ref_seqs.shape)} and {tuple(ref_ca.shape)}')
    N = seqs.shape[0]
    S = N // G if G else 0
    crow = scored.repeat_interleave(S, 0) if S != 1 else scored
    cflag, cseq, cca = _front_rows(name, crow & mask[:, :, 1].bool(), seqs, pos[:, :, 1])
    pairs = None
    if own:
        rflag, ref_seqs, ref_ca = _front_rows(name, scored & batch['mask_heavyatom'][:, :, 1].bool(), batch['aa'], batch['pos_heavyatom'][:, :, 1])
        c = torch.arange(N, device=seqs.device)
        pairs = torch.stack([c, c // max(S, 1)], 1).to(torch.int32)         # a candidate's own complex is c // S
    else:
        rflag = ref_mask
    tb = hip.align_traceback(cseq, ref_seqs, identity_table() if table is None else table, gap_open, gap_extend, qmask=cflag, rmask=rflag, pairs=pairs)
    sr = hip.superposed_rmsd_mapped(cca, ref_ca, tb['qmap'], pairs=pairs, want_transform=want_transform)
    cols = tb['columns']
    out = dict(seqid=torch.where(cols > 0, 100.0 * tb['matches'].float() / cols.clamp(min=1).float(), torch.full_like(cols, -1, dtype=torch.float32)),
               score=tb['score'], matches=tb['matches'], columns=cols, n_pairs=(tb['qmap'] >= 0).sum(1).to(torch.int32), rmsd=sr['rmsd'], qmap=tb['qmap'],
               ops=tb['ops'])
    if want_transform:
        out.update(rot=sr['rot'], trans=sr['trans'])
    if not own:
        out = {k: v.reshape((N, ref_seqs.shape[0]) + tuple(v.shape[1:])) for k, v in out.items()}
    return out


def _residue_set(name, what, batch, sel):
    """(G, L) bool: 'generated' (generate_flag), 'context' (the antibody residues that are not generated), 'antibody' (screen.chain_groups == 1) or a (G, L) mask"""
    from . import screen
    if isinstance(sel, str):
        gen = batch['generate_flag'].bool()
        if sel == 'generated':
            return gen
        if sel == 'antibody':
            return screen.chain_groups(batch['fragment_type']) == 1
        if sel == 'context':
            return (screen.chain_groups(batch['fragment_type']) == 1) & ~gen
        raise ValueError(f"{name}: {what} must be 'generated', 'context', 'antibody' or a (G, L) tensor, not {sel!r}")
    return sel.bool()


def superposed_rmsd(batch, pos, mask, fit='generated', score=None, ref_ca=None, ref_fit=None, ref_score=None, want_transform=False):
    """CA RMSD of candidates AFTER best-fit superposition, fitted on one residue set and measured on another (hip.superposed_rmsd).
    batch: G complexes; pos (G*S, L, A, 3) with CA in slot 1 and mask (G*S, L, A): S candidates of each, candidate c belongs to complex c // S.  fit / score:
    'generated' (generate_flag), 'context' (the antibody residues that are not generated), 'antibody' (every antibody residue) or a (G, L) mask; score=None
    means the fit set.  A residue whose CA is masked out leaves both sets.
    Without references every candidate is compared with the NATIVE of its own complex on the same rows (batch['pos_heavyatom'], batch['mask_heavyatom']; a
    residue whose native CA is missing leaves both sets too): every entry (G*S,).  fit='context', score='generated' is the framework-aligned CDR RMSD of loop
    modelling; fit='generated' is the loop's own shape deviation.  The launch compares every candidate with every complex's native and keeps its own, G times
    the pairs kept.  With ref_ca (R, nb, 3), ref_fit and ref_score (R, nb) (None = all / = ref_fit) every candidate is compared with every reference: every
    entry (G*S, R) -- a known binder's loop, canonical-class representatives, the designs themselves.  Points pair by rank, so the sets of a candidate and of
    a reference must be equally large: a pair whose counts differ, with fewer than 3 fit residues or no score residue has rmsd -1 and counts 0.
    -> dict of device tensors: rmsd fp32, n_fit, n_score int32 [, rot (..., 3, 3) and trans (..., 3) with want_transform: reference ~ rot candidate + trans].
    Rows wider than 256 cost one host read, otherwise none (a row may select at most 256 residues, fit and score together).  The screen does not call this:
    apply it to what optimize_antibody / sample_grouped return."""
    from . import hip
    name = 'superposed_rmsd'
    G, L = batch['aa'].shape
    fsel = _residue_set(name, 'fit', batch, fit)
    ssel = fsel if score is None else _residue_set(name, 'score', batch, score)
    if pos.dim() != 4 or mask.dim() != 3 or tuple(fsel.shape) != (G, L) or tuple(ssel.shape) != (G, L) or tuple(pos.shape[1:]) != (L, pos.shape[2], 3) \
            or pos.shape[2] < 2 or tuple(mask.shape) != tuple(pos.shape[:3]) or (pos.shape[0] % G if G else pos.shape[0]):
        raise ValueError(f'{name}: expected pos (G*S, L, A >= 2, 3), mask (G*S, L, A) and fit / score (G, L) with G = {G}, L = {L}; got '
                         f'{tuple(pos.shape)}, {tuple(mask.shape)}, {tuple(fsel.shape)} and {tuple(ssel.shape)}')
    own = ref_ca is None
    if own and (ref_fit is not None or ref_score is not None):
        raise ValueError(f'{name}: ref_fit / ref_score select residues of ref_ca, which is None')
    N = pos.shape[0]
    S = N // G if G else 0
    per = (lambda t: t.repeat_interleave(S, 0)) if S != 1 else (lambda t: t)
    cok = mask[:, :, 1].bool()
    if own:
        nok = batch['mask_heavyatom'][:, :, 1].bool()
        cok = cok & per(nok)
    cfit, cscore = per(fsel) & cok, per(ssel) & cok
    _, cfit, cscore, cca = _front_rows(name, cfit | cscore, cfit, cscore, pos[:, :, 1])
    if own:
        rfit, rscore = fsel & nok, ssel & nok
        _, ref_fit, ref_score, ref_ca = _front_rows(name, rfit | rscore, rfit, rscore, batch['pos_heavyatom'][:, :, 1])
    out = hip.superposed_rmsd(cca, ref_ca, qfit=cfit, rfit=ref_fit, qscore=None if score is None else cscore,
                              rscore=ref_score if (not own or score is not None) else None, want_transform=want_transform)
    if own and G:                                                   # a candidate's own complex is column c // S
        rows = torch.arange(N, device=pos.device)
        out = {k: v[rows, rows // S] for k, v in out.items()}
    elif own:
        out = {k: v.reshape((0,) + tuple(v.shape[2:])) for k, v in out.items()}
    return out


def _lddt_group(name, fragment_type, interface, G):
    """group (G, L) of the interface form from fragment_type (G, L) or (L,) (screen.chain_groups), or None."""
    from . import screen
    if not interface:
        return None
    if fragment_type is None:
        raise ValueError(f'{name}: interface=True takes the two sides from fragment_type')
    ft = fragment_type if fragment_type.dim() == 2 else fragment_type[None]
    return screen.chain_groups(ft.expand(G, ft.shape[1]))


def lddt_scores(model_pos, model_mask, ref_pos, ref_mask, rows=None, fragment_type=None, interface=False, cutoff=15.0):
    """lDDT-CA of candidate structures against reference structures, per residue and pooled (hip.lddt_ca_grouped): bounded in [0, 1],
    no superposition.  model_pos (G*S, L, A, 3), model_mask (G*S, L, A) or (G, L, A): S candidates of each of G references ref_pos (G, L, A, 3) / ref_mask
    (G, L, A) (or one reference (L, A, 3) / (L, A)); candidate c belongs to reference c // S.  rows (optional, (G, L) or (L,) bool): the residues that are
    scored.  interface=True: only pairs across the interface count, antibody against antigen as DockQ sees them (screen.chain_groups of fragment_type (G, L) or
    (L,)).  -> dict(num, den, lddt_res (G*S, L), lddt (G*S,)); -1 where nothing was scored (the reference's lddt() gives 1.0 there)."""
    from . import hip
    if ref_pos.dim() == 3:
        ref_pos, ref_mask = ref_pos[None], ref_mask[None]
    G = ref_pos.shape[0]
    if rows is not None and rows.dim() == 1:
        rows = rows[None].expand(G, -1)
    return hip.lddt_ca_grouped(model_pos, model_mask, ref_pos, ref_mask, rows=rows, group=_lddt_group('lddt_scores', fragment_type, interface, G), cutoff=cutoff)


def lddt_consistency(pos, mask, group_size, rows=None, fragment_type=None, interface=False, cutoff=15.0):
    """How well the S = group_size structures of each group agree with each other (hip.lddt_ca_ensemble): the lDDT counterpart of
    `commonness_score`.  pos (G*S, L, A, 3), mask (G*S, L, A) or (G, L, A); rows / fragment_type / interface / cutoff as for `lddt_scores`.
    -> dict(num, den, lddt (G, S, S): structure a as the reference, b as the model; consistency (G, S): the mean lDDT of each structure against its peers)."""
    from . import hip
    S = int(group_size)
    G = pos.shape[0] // S if S > 0 else 0
    if rows is not None and rows.dim() == 1:
        rows = rows[None].expand(G, -1)
    return hip.lddt_ca_ensemble(pos, mask, S, rows=rows, group=_lddt_group('lddt_consistency', fragment_type, interface, G), cutoff=cutoff)


def dockq_scores(model_pos, model_mask, native_pos, native_mask, fragment_type=None, group=None):
    """DockQ of candidate structures against the native complex, on the device (the reference writes every candidate to a PDB
    file and shells out: AbDock/src/tools/runner/design_for_pdb.py:316-321, AbDock/DockQ/DockQ.py:98-385).

    model_pos (S,L,A,3), model_mask (S,L,A) or (L,A), native_pos (L,A,3), native_mask (L,A).  The two chains are given either as
    `group` (L,) in {0: not scored, 1, 2} or through `fragment_type` (antibody chains 1/2 -> group 1, antigen 3 -> group 2).
    -> dict of (S,) tensors: fnat, irms, Lrms, DockQ."""
    from . import hip
    if group is None:
        group = torch.where(fragment_type == 3, 2, torch.where(fragment_type > 0, 1, 0))
    out = hip.dockq_lite(model_pos, model_mask, native_pos, native_mask, group)
    return dict(fnat=out[:, 0], irms=out[:, 1], Lrms=out[:, 2], DockQ=out[:, 3])


@torch.no_grad()
def sample_sharded(model, batch, sample_opt, k=1, group=None, seed=None):
    """Every rank samples its shard of `batch`; returns (local traj, (start, end), global top-k indices, all candidates)."""
    world, rank = (dist.get_world_size(group), dist.get_rank(group)) if dist.is_initialized() else (1, 0)
    n = batch['aa'].shape[0]
    sub, (a, b) = shard_batch(batch, world, rank)
    opt = dict(sample_opt)
    opt.setdefault('rng_offset', a * batch['aa'].shape[1])      # distinct Philox counters per global sample index
    if seed is not None:
        opt['seed'] = seed
    n_gen = int(batch['generate_flag'][0].sum()) if n > 0 else 0
    if b > a:
        traj = model.sample(sub, sample_opt=opt)
        cand = candidates_from_positions(traj[0][1], sub['generate_flag'])
    else:                                   # more ranks than samples: nothing to denoise here, but every rank still joins the gather
        traj = {}
        cand = batch['pos_heavyatom'].new_zeros((0, n_gen, 3))
    if world > 1:
        counts = [shard_range(n, world, r)[1] - shard_range(n, world, r)[0] for r in range(world)]
        cand = all_gather_candidates(cand, counts, group)
    top = rank_commoness(cand, min(k, cand.shape[0]))
    return traj, (a, b), top, cand


@torch.no_grad()
def sample_replicated(model, complex_batch, num_samples, sample_opt=None, optimize_step=None):
    """N samples of ONE complex without replicating it.

    The reference's runners build the batch by repeating one crop `num_samples` times on the host
    (AbDock/src/tools/runner/design_for_pdb.py:141-147), so encode() runs N times and N identical copies of pair_feat
    (17 MB each at L=256) are streamed from HBM at every step.  Here `complex_batch` holds the complex once (batch dim 1):
    it is encoded once and the sampler shares res_feat / pair_feat across the N samples.  Returns the same trajectory
    dict as `model.sample` (batch dim `num_samples`).  `optimize_step` selects `model.optimize`-style partial denoising."""
    from . import hip
    sample_opt = dict(sample_opt or {'sample_structure': True, 'sample_sequence': True})
    sample_opt.pop('contig', None)
    one = {k: (v[:1] if torch.is_tensor(v) else v) for k, v in complex_batch.items()}
    res_feat, pair_feat, R_0, p_0 = model.encode(one, remove_structure=sample_opt.get('sample_structure', True),
                                                remove_sequence=sample_opt.get('sample_sequence', True))
    rep = lambda a: a.expand(num_samples, *a.shape[1:]).contiguous()
    v_0 = rep(hip.so3_log(R_0, grad_mode=False))
    args = (v_0, rep(p_0), rep(one['aa']))
    masks = (rep(one['generate_flag']), rep(one['mask']))
    if one.get('aa_allowed') is not None:                       # the complex's allowed residue types: replicated like generate_flag
        sample_opt['aa_allowed'] = rep(one['aa_allowed'])
    if one.get('guide_role') is not None:                       # the complex's hotspots and repellers (model.guide_roles): the knobs ride in sample_opt
        sample_opt['guide_role'] = rep(one['guide_role'])
    if optimize_step is None:
        return model.diffusion.sample(*args, res_feat, pair_feat, *masks, **sample_opt)
    return model.diffusion.optimize(*args, optimize_step, res_feat, pair_feat, *masks, **sample_opt)


def complexes_of_rank(n_complexes, world_size, rank):
    """By-complex partition of a test set (BASELINE config 4): contiguous, balanced blocks of complexes per rank
    (64 complexes over 8 ranks: rank r owns 8 r .. 8 r + 7), so every sample of a complex -- and therefore its whole commonness ranking --
    stays on one GPU, nothing is exchanged per complex, and the global sample indices of a rank's launch are contiguous (one Philox
    offset per launch keeps the draws independent of the number of ranks)."""
    a, b = shard_range(n_complexes, world_size, rank)
    return list(range(a, b))


def pad_complex(one, L):
    """A batch dict with batch dim 1 padded to L residues the way the reference's PaddingCollate does (AbDock/src/utils/data.py:60-76:
    zeros, `aa` with the padding token 21, masks False)."""
    L0 = one['aa'].shape[1]
    if L0 == L:
        return one
    out = {}
    for k, v in one.items():
        if torch.is_tensor(v) and v.dim() >= 2 and v.shape[1] == L0:
            pad = v.new_full((v.shape[0], L - L0) + tuple(v.shape[2:]), 21 if k == 'aa' else 0)
            out[k] = torch.cat([v, pad], 1)
        else:
            out[k] = v
    return out


@torch.no_grad()
def sample_grouped(model, complexes, num_samples, sample_opt=None, optimize_step=None, pad_to=None):
    """`num_samples` samples of EACH of G complexes in one launch (BASELINE config 4: a rank's leg of a test set).

    The reference designs a test set one structure at a time (AbDock/src/tools/runner/design_for_testset.py:556-589), each with its
    crop replicated `num_samples` times on the host.  Here the G complexes (a list of batch dicts with batch dim 1; padded to a common
    length like PaddingCollate does) are encoded ONCE each as a batch of G, and the sampler runs G x num_samples samples as one batch
    whose samples share the pair features of their complex (`abopt_eps_net_forward(pair_feat_shared = num_samples)`): the kernels see
    full-size launches instead of G small ones, and z is read from HBM once per complex and query block, not once per sample.
    Sample g * num_samples + s is sample s of complex g.  pad_to: pad to this length instead of the longest complex of the launch (the
    test-set driver passes the longest complex of the whole set, see `launch_rng_offset`).  Returns the trajectory dict of `model.sample`
    (batch dim G * num_samples)."""
    from . import hip
    sample_opt = dict(sample_opt or {'sample_structure': True, 'sample_sequence': True})
    sample_opt.pop('contig', None)
    L = max(max(int(c['aa'].shape[1]) for c in complexes), int(pad_to or 0))
    if any(c.get('aa_allowed') is not None for c in complexes):      # allowed residue types of some complexes: the others allow every type
        complexes = [c if c.get('aa_allowed') is not None else dict(c, aa_allowed=torch.full_like(c['aa'], -1, dtype=torch.int32)) for c in complexes]
    if any(c.get('guide_role') is not None for c in complexes):      # roles of some complexes: the others have neither hotspots nor repellers, nothing moves there
        complexes = [c if c.get('guide_role') is not None else dict(c, guide_role=torch.zeros_like(c['aa'], dtype=torch.int32)) for c in complexes]
    padded = [pad_complex(c, L) for c in complexes]
    batch = {k: (torch.cat([c[k][:1] for c in padded], 0) if torch.is_tensor(v) else v) for k, v in padded[0].items()}
    res_feat, pair_feat, R_0, p_0 = model.encode(batch, remove_structure=sample_opt.get('sample_structure', True),
                                                remove_sequence=sample_opt.get('sample_sequence', True))
    rep = lambda a: a.repeat_interleave(num_samples, dim=0).contiguous()
    v_0 = rep(hip.so3_log(R_0, grad_mode=False))
    args = (v_0, rep(p_0), rep(batch['aa']))
    masks = (rep(batch['generate_flag']), rep(batch['mask']))
    if batch.get('aa_allowed') is not None:
        sample_opt['aa_allowed'] = rep(batch['aa_allowed'])
    if batch.get('guide_role') is not None:
        sample_opt['guide_role'] = rep(batch['guide_role'])
    if optimize_step is None:
        return model.diffusion.sample(*args, res_feat, pair_feat, *masks, **sample_opt)
    return model.diffusion.optimize(*args, optimize_step, res_feat, pair_feat, *masks, **sample_opt)


def launch_rng_offset(first_complex, samples_per_complex, L_pad):
    """Philox counter base of the launch whose first complex is `first_complex`.  The kernels read counter base + n L + l for sample n,
    residue l of a launch padded to L (distinct sub-sequence tags for sample_init / add_noise / the loop's steps, csrc/denoise.hip), so
    when EVERY launch of a test set is padded to the same L_pad (the longest complex of the whole set) the launches' ranges
    [c0 S L_pad, (c0 + G) S L_pad) tile the counter space: no two samples share a draw, and sample s of complex c reads
    (c S + s) L_pad + l however the complexes are grouped into launches or spread over ranks.  (With each launch padded to its OWN longest
    complex a later, shorter launch started inside an earlier, longer one's range: identical draws for samples of different complexes.)"""
    return int(first_complex) * int(samples_per_complex) * int(L_pad)


@torch.no_grad()
def design_testset_sharded(model, complexes, samples_per_complex, sample_opt=None, k=1, group=None, seed=0, optimize_step=None,
                           complexes_per_launch=8, native=None):
    """BASELINE config 4: a test set of complexes x `samples_per_complex` samples over the ranks of `group`, partitioned BY COMPLEX.

    The reference fans this out as one subprocess per structure through Ray and collects files
    (AbDock/optimize_ab.py:21-31,66-72; AbDock/src/tools/runner/design_for_testset.py:556-589 ranks each structure's samples).
    Here every rank designs its own block of complexes, `complexes_per_launch` of them at a time as ONE batch (`sample_grouped`:
    every complex encoded once, its samples share its pair features inside the kernels), ranks each complex's candidates locally with
    the commonness score, optionally scores them against the native structure (DockQ on the device), and the per-complex summaries
    (a few hundred bytes each) are exchanged once at the end with all_gather_object.

    complexes: list of batch dicts with batch dim 1.  Every launch is padded to the longest complex of the WHOLE test set, so the Philox
    stream position of a sample depends on its global index (complex x samples_per_complex + sample) alone (`launch_rng_offset`): no two
    samples share a draw, and positions / sequences do not depend on the number of ranks or on `complexes_per_launch` (padding never
    reaches a real residue; AbDock's prmsd score averages over the padded length like a PaddingCollate batch does, dpm_full.py:110).
    native (optional): dict(pos (L,A,3), mask (L,A)) per complex, or True to score against the complex's own input coordinates.
    -> list (one entry per complex, in input order, identical on every rank) of
    dict(complex=index, rank=owner, top=LongTensor(k), score=Tensor(S), ca=final CA positions of the generated residues (S, n_gen, 3)
    [, dockq=dict of (S,) tensors])."""
    world, rank = (dist.get_world_size(group), dist.get_rank(group)) if dist.is_initialized() else (1, 0)
    sample_opt = dict(sample_opt or {'sample_structure': True, 'sample_sequence': True})
    S = int(samples_per_complex)
    mine = []
    own = complexes_of_rank(len(complexes), world, rank)
    G = max(1, int(complexes_per_launch))
    L_all = max(int(c['aa'].shape[1]) for c in complexes)            # the same on every rank: `complexes` is the whole test set
    for lo in range(0, len(own), G):
        ids = own[lo:lo + G]
        chunk = [complexes[c] for c in ids]
        L = L_all
        opt = dict(sample_opt, seed=int(seed), rng_offset=launch_rng_offset(ids[0], S, L_all))
        traj = sample_grouped(model, chunk, S, opt, optimize_step=optimize_step, pad_to=L_all)
        p_fin = traj[0][1]
        for g, c in enumerate(ids):
            one = pad_complex(complexes[c], L)
            gen = one['generate_flag'][:1].expand(S, -1)
            pc = p_fin[g * S:(g + 1) * S]
            cand = candidates_from_positions(pc, gen)
            score = commonness_score(cand)
            top = torch.topk(score, k=min(k, S), largest=False)[1]
            rec = dict(complex=c, rank=rank, top=top.cpu(), score=score.cpu(), ca=cand.cpu())
            if native is not None:
                rec['dockq'] = {kk: v.cpu() for kk, v in _dockq_of_samples(model, one, traj, g * S, S, native if native is not True else None, c).items()}
            mine.append(rec)
    if world > 1:
        everyone = [None] * world
        dist.all_gather_object(everyone, mine, group=group)
        mine = [e for part in everyone for e in part]
    return sorted(mine, key=lambda e: e['complex'])


def _dockq_of_samples(model, one, traj, lo, S, native, c):
    """DockQ (CA-only flavour the runner uses, design_for_pdb.py:316-321) of samples lo .. lo + S - 1 of a finished trajectory against the
    native complex: the generated residues' backbone is rebuilt from the final frames (reconstruct_backbone_partially), everything on
    the device."""
    from . import geometry, hip
    v, p, s = traj[0][0][lo:lo + S], traj[0][1][lo:lo + S], traj[0][2][lo:lo + S]
    rep = lambda a: a[:1].expand(S, *a.shape[1:]).contiguous()
    R = hip.so3_exp(v)
    gen = rep(one['generate_flag'])
    pos, mask = geometry.reconstruct_backbone_partially(rep(one['pos_heavyatom']), R, p, torch.where(gen, s, rep(one['aa'])), rep(one['chain_nb']),
                                                        rep(one['res_nb']), rep(one['mask_heavyatom']), gen)
    if native is None:
        npos, nmask = one['pos_heavyatom'][0], one['mask_heavyatom'][0]
    else:
        nat = native[c] if isinstance(native, (list, tuple)) else native
        npos, nmask = nat['pos'].to(pos.device), nat['mask'].to(pos.device)
    return dockq_scores(pos, mask, npos, nmask, fragment_type=one['fragment_type'][0])


def wrap_ddp(model, device=None, **kw):
    """Data-parallel training (BASELINE config 5 at N GPUs): one process per GPU, gradients averaged by bucketed all-reduce over
    RCCL (backend 'nccl') overlapped with backward.  The reference's train.py (AbDock/train.py:70-114) is single-process; this is
    the wrapper a multi-GPU launch adds around `get_model(cfg)`.  The custom autograd functions of the training path are ordinary
    torch.autograd.Function nodes, so DistributedDataParallel's hooks see their parameter gradients like any other."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    kw.setdefault('find_unused_parameters', True)      # the prmsd loss touches no parameter when mask_generate[:, 0] is all False
    return DDP(model.to(dev), device_ids=[dev.index] if dev.type == 'cuda' else None, **kw)
