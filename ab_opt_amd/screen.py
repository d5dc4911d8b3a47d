"""The antibody optimisation screen of AbDock/optimize_ab.py on the device: dock, redesign, re-dock.

The reference runs three programs per antibody, fanned out as Ray subprocesses that each reload a checkpoint and exchange PDB files
(AbDock/optimize_ab.py:12-98, driven by ab_opt.ipynb / ab_opt_analysis_4mutations.ipynb):
  1. dock       dock_pdb.py -c configs/test/dock_cdr.yml -n P: P poses of the docked residues (structure only, sequence fixed)
  2. redesign   seq_design_batch: the sequence-design model (configs/test/seq_design.yml, backbone+CB) samples S designs on every fixed
                pose backbone, optionally limited by a contig; AAR and PPL per design (design_for_pdb.py:241-290)
  3. re-dock    dock_seqs: the first design of every pose (.../H_CDR3/0000.pdb) docked again D times; CA-only DockQ against that design's
                complex and the prmsd of every sample (design_for_pdb.py:311-321); the notebook keeps the designs at or below the medians
                of DockQ_std, prmsd_std and prmsd_avg (`screen_filter`).
Here the complex stays a batch dict on the device from start to end: the poses and designs are rebuilt with
`geometry.reconstruct_backbone_partially`, every stage walks its poses in chunks of `poses_per_launch` (each pose encoded once, its samples
share its pair features: `sampler.sample_replicated` / `sampler.sample_grouped`), and a chunk's re-docks are scored by ONE grouped DockQ
launch and ONE grouped commonness launch (hip.dockq_lite_grouped, hip.commonness_score_grouped).  No relax stage (the reference's
--no_rosetta path), no PDB write / re-parse; the residues to dock, redesign and re-dock are given as masks instead of by renumbering files.

Randomness: stage k draws from Philox seed `stage_seed(seed, k)`, and sample i of a stage (i = its GLOBAL index: pose, pose x S + design,
(pose x k + screened design) x D + re-dock) reads the counters from i L on, as `sampler.launch_rng_offset` lays them out.  Results
therefore do not depend on `poses_per_launch` or on the number of ranks (bit for bit where the launches of different sizes take the same
kernel forms: DESIGN.md section 3.1b).  Multi-GPU: rank r owns the poses `sampler.shard_range(P, world, r)` through all three stages;
one tensor all_gather per result field at the end.

Pose clustering (optional, off by default): a docking sampler returns a few binding modes many times over, and the two expensive
stages spend P S + P k D trajectories on those near-duplicates.  With `cluster_cutoff` the P poses are clustered on the device after stage 1
(`sampler.cluster_poses`: greedy, RMSD of the docked residues' CA without superposition -- the distance of the commonness score) and stages 2 and 3 run on
the C cluster centres only, in cluster order: cluster c takes the place pose c has above for `launch_plan`, `sampler.shard_range(C, world, rank)` and the
Philox layout (global sample index c S + design, ...).  With several ranks the poses and their rebuilt coordinates are gathered before the clustering, so
every rank clusters the same array and owns the centres of its shard.  With `redock_cutoff` the D re-docks of every screened design are clustered as well
(ONE grouped launch pair per chunk, hip.cluster_poses_grouped): the largest cluster's share of D is the convergence measure DockQ_std approximates.
How many clusters trained weights produce, and what a cutoff costs in hit rate, is unmeasured: no trained checkpoint exists here.

Interface geometry (optional, off by default): without a relax stage nothing above looks at whether a pose is physically possible.  With any
of `clash_cutoff`, `contact_cutoff`, `bond_max` every pose (per chunk, right after it is rebuilt) and every re-dock (ONE grouped call per chunk,
hip.interface_geometry_grouped, beside the grouped DockQ and commonness calls) is scored for steric clashes and contacts between antibody and antigen
(`chain_groups`) and for broken peptide bonds, and the D re-docks of a design give the share of them that contacts each residue: the consensus epitope.
The counts steer nothing and draw nothing; `screen_filter(max_clashes=, min_contacts=)` can use them afterwards.  3.0 / 5.0 / 2.0 A are conventional values,
not tuned ones, and the distribution of the counts for trained weights is unmeasured.

Sequence clustering (optional, off by default): the sequence side of the same waste.  With `seq_mismatch` the S designs of every pose are
clustered by the number of differing positions and their composition is counted (two grouped calls per design launch); `screen_by='diverse'` re-docks one design per
family instead of k near-copies, and `share_redocks` re-docks every distinct chosen sequence once, whichever poses chose it.  How many duplicates trained weights
produce is unmeasured.

lDDT-CA (optional, off by default): DockQ, commonness and prmsd say how well the D re-docks of a design agree, not WHERE they disagree.  With
`lddt_cutoff` every re-dock is scored by the lDDT-CA of its re-docked residues against its design complex, per residue and pooled (ONE hip.lddt_ca_grouped call per
chunk, with the groups of the grouped DockQ call), and among the D re-docks of its design (ONE hip.lddt_ca_ensemble call per chunk): bounded in [0, 1], no
superposition, -1 where nothing is scored.  The scores steer nothing and draw nothing; `screen_filter(min_lddt=)` can use them afterwards.  What values trained
weights produce is unmeasured.
"""
import time

import torch
import torch.distributed as dist

from . import geometry, hip, sampler
from .model import generate_mask_from_str

STAGES = ('dock', 'design', 'redock')


def stage_seed(seed, stage):
    """Philox seed of a stage ('dock', 'design', 'redock'): distinct per stage and per screen seed."""
    return int(seed) * len(STAGES) + STAGES.index(stage)


def samples_per_pose(stage, designs_per_pose, screened_per_pose, redocks_per_design):
    return {'dock': 1, 'design': int(designs_per_pose), 'redock': int(screened_per_pose) * int(redocks_per_design)}[stage]


def stage_rng_offset(stage, first_pose, L, designs_per_pose, screened_per_pose, redocks_per_design):
    """Philox counter base of the launch of `stage` whose first pose is `first_pose` (complex length L): its samples are poses x
    samples_per_pose in global order, so the launches of all chunks and ranks tile [0, P x samples_per_pose x L)."""
    return sampler.launch_rng_offset(first_pose, samples_per_pose(stage, designs_per_pose, screened_per_pose, redocks_per_design), L)


def launch_plan(num_poses, poses_per_launch, world=1, rank=0):
    """[(lo, hi), ...]: the global pose ranges of rank `rank`'s launches (its shard, in chunks of poses_per_launch)."""
    a, b = sampler.shard_range(int(num_poses), int(world), int(rank))
    step = max(1, int(poses_per_launch))
    return [(lo, min(lo + step, b)) for lo in range(a, b, step)]


def design_mask(design_flag, contig=''):
    """The residues the design stage redesigns: design_flag, limited to the contig 'start-end' (1-based along L, inclusive) the way
    model.sample applies it for AbDock (diffab.py:114-140)."""
    if not contig:
        return design_flag.bool()
    return torch.logical_and(design_flag.bool(), generate_mask_from_str(contig, design_flag))


def chain_groups(fragment_type):
    """DockQ's two chains from fragment_type: antibody chains (1, 2) -> 1, antigen (3) -> 2, anything else 0 (sampler.dockq_scores)."""
    return torch.where(fragment_type == 3, 2, torch.where(fragment_type > 0, 1, 0))


def diverse_choice(centre, k):
    """The k designs of every pose that screen_by='diverse' re-docks, from centre (G, S) of hip.cluster_sequences_grouped (cluster order, -1 padded): the centres
    of the pose's first min(k, clusters) sequence clusters in the kernel's discovery order, then -- a pose with fewer than k clusters -- the designs of lowest
    index not yet chosen, ascending.  -> (G, k) int64.  Pure torch, no host read: design i sorts by its cluster's number if it is one of the first k centres,
    by S + i otherwise."""
    G, S = centre.shape
    dev = centre.device
    key = (S + torch.arange(S + 1, device=dev)).repeat(G, 1)                             # column S takes the writes of the padding
    cen = centre[:, :k].long()
    key.scatter_(1, torch.where(cen >= 0, cen, S), torch.arange(cen.shape[1], device=dev).expand(G, -1))
    return torch.sort(key[:, :S], dim=1, stable=True)[1][:, :k]


def _with(one, **kw):
    out = dict(one)
    out.update(kw)
    return out


def _rebuild(pos, mask, traj0, lo, hi, aa, flag, one):
    """Samples lo .. hi - 1 of a finished trajectory -> (pos, mask) with the residues of `flag` rebuilt from their final frames and types,
    everything else copied from `pos` / `mask` (per-sample contexts, (hi - lo, L, A, 3) / (hi - lo, L, A)); aa (hi - lo, L) input types."""
    v, p, s = traj0[0][lo:hi], traj0[1][lo:hi], traj0[2][lo:hi]
    n = hi - lo
    rep = lambda a: a[:1].expand(n, *a.shape[1:]).contiguous()
    gen = flag[None].expand(n, -1).contiguous()
    return geometry.reconstruct_backbone_partially(pos, hip.so3_exp(v), p, torch.where(gen, s, aa), rep(one['chain_nb']), rep(one['res_nb']),
                                                   mask, gen)


def _scored_mean_std(t, dim):
    """Mean and population standard deviation of the lDDT values t along `dim`, over the entries that were scored (>= 0; -1 marks "no scored pair"), computed in
    float64 and rounded to fp32 once; -1 where no entry was scored.  Pure torch, no host read."""
    ok = t >= 0
    cnt = ok.sum(dim)
    div = cnt.clamp_min(1).double()
    v = torch.where(ok, t.double(), 0.0)
    mean = v.sum(dim) / div
    var = (torch.where(ok, (t.double() - mean.unsqueeze(dim)) ** 2, 0.0)).sum(dim) / div
    none = cnt == 0
    return torch.where(none, -1.0, mean).float(), torch.where(none, -1.0, var.sqrt()).float()


@torch.no_grad()
def optimize_antibody(dock_model, design_model, complex_, num_poses, designs_per_pose, redocks_per_design, design_flag=None, redock_flag=None,
                      contig='', screened_per_pose=1, seed=0, poses_per_launch=8, group=None, screen_by='first', timings=None, allowed_aa=None,
                      dock_steps=None, design_steps=None, cluster_cutoff=None, max_clusters=None, redock_cutoff=None, clash_cutoff=None, contact_cutoff=None,
                      bond_max=None, seq_mismatch=None, share_redocks=False, lddt_cutoff=None, design_temperature=None, dock_noise_scale=None,
                      hotspots=None, dock_guide=None):
    """Dock -> redesign -> re-dock screen of one antibody-antigen complex (module docstring).

    complex_: batch dict with batch dim 1 (cropped, as sample_replicated takes it); its generate_flag marks the residues to dock.
    design_flag / redock_flag (L,) or (1, L) bool: residues to redesign / re-dock (default: generate_flag; the reference's
    --label_heavy_as_cdr re-dock corresponds to every heavy-chain residue).  contig limits design_flag ('start-end', 1-based).
    screened_per_pose k designs of every pose go on to the re-dock: the first k (screen_by='first', as the reference takes 0000.pdb) or the
    k of lowest PPL (screen_by='ppl', stable order), or one per sequence cluster (screen_by='diverse', below).  num_poses >= 2 and redocks_per_design >= 2 (commonness needs two structures).
    allowed_aa (optional, (L,) or (1, L) int32 / int64; default: complex_['aa_allowed'] if it has one): the residue types each redesigned residue may take, bit k of a
    word = type k (model.aa_allowed_mask).  It constrains the redesign stage alone -- the docking stages draw no types -- inside the sampler, so no design is thrown away:
    seqs, the re-docked designs and everything downstream hold allowed types only; aar still counts recovery of the input sequence.
    dock_steps / design_steps (optional; default: every trained step): the network evaluations of every dock and re-dock trajectory / of every design trajectory,
    over the evenly respaced sub-sequence of the model's steps (FullDPM.sample(steps=K)) -- the screen spends P + P S + P k D trajectories per
    antibody, and this trades their depth for breadth.  Sample quality against K is unmeasured.
    design_temperature (optional, 0 or >= 1e-3; default None: nothing changes, bit for bit): the temperature of the design stage's residue
    types (FullDPM.sample(seq_temperature=tau)) -- below 1 every design trajectory draws from a sharper distribution of the network's prediction, 0 takes its most
    probable allowed type at every step: "confident, conservative designs" from the sampler instead of oversampling and keeping the designs of lowest PPL.  ppl is
    then the perplexity of the tempered distribution: comparable between designs of one call, not with a call at another temperature.  allowed_aa holds as ever.
    dock_noise_scale (optional, >= 0; default None: nothing changes, bit for bit): the scale of the structure noise of every dock and re-dock step
    (FullDPM.sample(noise_scale=lambda)); below 1 the ensembles tighten, 0 leaves the initial draw as a trajectory's only randomness.  What either does to hit
    rates is unmeasured.
    hotspots / dock_guide (optional; default None: nothing changes, bit for bit): guided docking.  dock_guide is a dict of the guide_* knobs
    of FullDPM.sample (guide_attract, guide_attract_radius, guide_repel, guide_repel_radius, guide_max_shift, guide_decay) and, optionally, repel = 'context' /
    'antigen' / a bool mask (model.guide_roles); hotspots are 1-based positions like `contig`, or a bool mask (L,): the epitope the docked residues are pulled to.
    Every dock and re-dock step is followed by the nudge; the design stage, which keeps the structure, is not guided.  hotspots without dock_guide is an error.  No
    result key is added.  What guidance does to DockQ or to hit rates is unmeasured.
    cluster_cutoff (optional, Angstrom; default None: every pose goes on, nothing below changes): cluster the P poses after stage 1 and run stages 2 and 3 on the
    C cluster centres only (module docstring); max_clusters (optional, >= 1; needs cluster_cutoff) caps C -- poses left over at the cap keep label -1 and
    are not screened.  The result gains cluster_label (P,), cluster_centre (C,) (pose indices) and cluster_size (C,), all int64; pose_ca / pose_score
    stay (P, ...), and every field of stages 2 and 3 below has leading dimension C instead of P: row c belongs to pose cluster_centre[c].  Costs one host read
    (C) between stage 1 and stage 2.
    redock_cutoff (optional, Angstrom): cluster the D re-docks of every screened design; the result gains redock_cluster_frac (., k) fp32, the largest cluster's
    share of D, and redock_clusters (., k) int64, the number of clusters.
    clash_cutoff / contact_cutoff / bond_max (optional, Angstrom; default None: nothing below changes, bit for bit): if any is given, score the interface geometry
    of every pose and every re-dock (module docstring; the others default to 3.0, 5.0 and "breaks are not counted").  The result gains pose_geom (P, 5) int64 --
    always P rows, like pose_score --, redock_geom (., k, D, 5) int64 (columns: clash, contacts, iface1, iface2, breaks of hip.interface_geometry_grouped; side 1 =
    antibody, side 2 = antigen) and epitope_freq (., k, L) fp32: the share of a design's D re-docks in which each residue is in a contact.
    seq_mismatch (optional, int >= 0; default None: nothing below exists): after every design launch cluster the S designs of each pose (two
    designs are neighbours iff they differ at no more than seq_mismatch positions; hip.cluster_sequences_grouped) and count their composition
    (hip.sequence_profile_grouped).  The result gains seq_label (., S), seq_centre (., S) (-1 padded), seq_size (., S) (0 padded), seq_clusters (.,) and
    seq_counts (., n_design, 21), all int64.  screen_by='diverse' (needs seq_mismatch): the k re-docked designs of a pose are the centres of its first
    min(k, clusters) sequence clusters in order of discovery, then the designs of lowest index not yet chosen (`diverse_choice`).
    share_redocks (default False; needs redock_flag to cover generate_flag and P k <= 16384): the chosen designs of ALL poses are clustered by identity after stage 2
    (one group, gathered over ranks first) and every distinct sequence -- a unit -- is re-docked once, from its lowest-index owner's complex: with the docked residues
    regenerated and their input structure hidden from the network, the re-dock trajectories of a design do not depend on the pose it was designed on.  Stage 3 runs
    over the U units as it runs over poses with one screened design each (launches, shards, Philox: global sample index unit D + re-dock); prmsd, redock_score and
    the optional re-dock cluster / geometry / epitope fields are computed per unit and copied to every owner (pose, slot), dockq is computed for every owner against
    its own design complex.  Every field keeps its shape; the result gains design_unit (., k), unit_owner (U,) (flat index pose k + slot of the unit's centre) and
    unit_size (U,), int64.  Costs one host read (the units) between stage 2 and stage 3.
    lddt_cutoff (optional, Angstrom, 15.0 is the reference's; default None: nothing below exists, no other field changes): score every re-dock
    by lDDT-CA of the re-docked residues (rows = redock_flag, pairs with every residue of the complex within lddt_cutoff in the design) -- against its design complex
    (ONE hip.lddt_ca_grouped call per chunk, beside the grouped DockQ call and with its groups) and among the D re-docks of its design (ONE hip.lddt_ca_ensemble call
    per chunk).  The result gains redock_lddt (., k, D) fp32, the pooled lDDT of each re-dock against its design; redock_lddt_res (., k, D, n_redock) fp32, the same per
    re-docked residue; lddt_mean / lddt_std (., k) over the D re-docks and lddt_res_mean (., k, n_redock), the per-residue "where do they disagree" answer, each
    ignoring the -1 of a re-dock or residue without a scored pair (-1 if all are); redock_consistency (., k, D) fp32, the mean lDDT of each re-dock against its D - 1
    peers.  Leading dimension, gathering and cluster_cutoff as for dockq; with share_redocks the versus-design fields follow dockq (per owner) and
    redock_consistency follows redock_score (per unit, copied to every owner).  The scores steer nothing and draw nothing.
    timings (optional dict): receives the seconds each stage took on this rank (device-synchronised) and of the final gather ('cluster': the gather and
    clustering between stage 1 and stage 2, with cluster_cutoff; 'units': the gather and clustering between stage 2 and stage 3, with share_redocks).

    -> dict of device tensors in global pose order (P poses, S designs, k screened, D re-docks; n_* = residues in the mask):
      (with cluster_cutoff: C cluster centres in place of the P poses in every field from seqs on, see above)
      pose_ca (P, n_dock, 3), pose_score (P,)           CA of the docked residues of every pose, its commonness among the P poses
      seqs (P, S, n_design) int64, aar (P, S), ppl (P, S)  designed residues, recovery of the input sequence on them, perplexity
      chosen (P, k) int64                                 the designs that were re-docked
      dockq (P, k, D, 4)                                  fnat, irms, Lrms, DockQ of every re-dock against its design (-1: empty selection)
      prmsd (P, k, D), redock_score (P, k, D)             prmsd of every re-dock (traj[0][3]: the head's per-sample value, which the
                                                          reference's prmsd[i].mean() returns, design_for_pdb.py:241); commonness of its
                                                          re-docked residues' CA among the D
      dockq_mean / dockq_std / prmsd_mean / prmsd_std (P, k)   over the D re-docks (np.mean / np.std, as the notebook)"""
    world, rank = (dist.get_world_size(group), dist.get_rank(group)) if dist.is_initialized() else (1, 0)
    one = {k: (v[:1] if torch.is_tensor(v) else v) for k, v in complex_.items()}
    P, S, D, k = int(num_poses), int(designs_per_pose), int(redocks_per_design), int(screened_per_pose)
    if P < 2 or D < 2 or S < 1 or not 1 <= k <= S:
        raise ValueError(f'optimize_antibody: need num_poses >= 2, redocks_per_design >= 2 and 1 <= screened_per_pose <= designs_per_pose '
                         f'(got P={P}, S={S}, k={k}, D={D})')
    if screen_by not in ('first', 'ppl', 'diverse'):
        raise ValueError(f"screen_by must be 'first', 'ppl' or 'diverse', not {screen_by!r}")
    if seq_mismatch is not None:
        seq_mismatch = hip.check_max_mismatch('optimize_antibody: seq_mismatch', seq_mismatch)
    if screen_by == 'diverse' and seq_mismatch is None:
        raise ValueError("optimize_antibody: screen_by='diverse' re-docks the centres of the sequence clusters and needs seq_mismatch")
    if share_redocks and P * k > 16384:
        raise ValueError(f'optimize_antibody: share_redocks clusters the P k chosen designs as one group of at most 16384 (got P={P}, k={k})')
    if cluster_cutoff is not None:
        cluster_cutoff = hip.check_cluster_cutoff('optimize_antibody: cluster_cutoff', cluster_cutoff)
    if redock_cutoff is not None:
        redock_cutoff = hip.check_cluster_cutoff('optimize_antibody: redock_cutoff', redock_cutoff)
    geom = None
    if clash_cutoff is not None or contact_cutoff is not None or bond_max is not None:
        geom = dict(clash_cutoff=hip.check_distance_cutoff('optimize_antibody: clash_cutoff', 3.0 if clash_cutoff is None else clash_cutoff),
                    contact_cutoff=hip.check_distance_cutoff('optimize_antibody: contact_cutoff', 5.0 if contact_cutoff is None else contact_cutoff),
                    bond_max=None if bond_max is None else hip.check_distance_cutoff('optimize_antibody: bond_max', bond_max))
    if lddt_cutoff is not None:
        lddt_cutoff = hip.check_lddt_cutoff('optimize_antibody: lddt_cutoff', lddt_cutoff)
    if max_clusters is not None and (cluster_cutoff is None or int(max_clusters) < 1):
        raise ValueError(f'optimize_antibody: max_clusters must be >= 1 and needs cluster_cutoff (got max_clusters={max_clusters!r}, cluster_cutoff={cluster_cutoff!r})')
    L = int(one['aa'].shape[1])
    dev = one['aa'].device
    given = one.pop('aa_allowed', None)
    allowed_aa = given if allowed_aa is None else allowed_aa
    design_extra = {} if allowed_aa is None else dict(aa_allowed=allowed_aa.reshape(1, L).to(dev))
    gen = one['generate_flag'][0].bool()
    dflag = design_mask((gen if design_flag is None else design_flag.reshape(-1).to(dev)), contig)
    rflag = gen if redock_flag is None else redock_flag.reshape(-1).to(dev).bool()
    n_dock, n_design, n_redock = int(gen.sum()), int(dflag.sum()), int(rflag.sum())
    if min(n_dock, n_design, n_redock) == 0:
        raise ValueError('optimize_antibody: the dock, design and re-dock masks must each select at least one residue')
    if share_redocks and bool((gen & ~rflag).any()):
        raise ValueError('optimize_antibody: share_redocks needs redock_flag to cover every docked residue (generate_flag): a docked residue that is not '
                         're-docked keeps the coordinates of its own pose in the re-dock input, so designs of different poses would no longer share trajectories')
    plan = launch_plan(P, poses_per_launch, world, rank)
    a, b = sampler.shard_range(P, world, rank)
    mine = b - a
    depth = dict(dock=dock_steps, design=design_steps, redock=dock_steps)
    noise = {} if dock_noise_scale is None else dict(noise_scale=hip.check_noise_scale('optimize_antibody: dock_noise_scale', dock_noise_scale))
    guide_extra = {}
    if dock_guide is not None:
        from . import model as model_
        dg = dict(dock_guide)
        repel = dg.pop('repel', None)
        if hotspots is not None or repel is not None or one.get('guide_role') is None:
            guide_extra = dict(guide_role=model_.guide_roles(one, hotspots=hotspots, repel=one['mask'].bool() if isinstance(repel, str) and repel == 'context' else repel))
        noise = dict(noise, **hip.check_guidance(**dg))                 # the dock and re-dock stages' options: the knobs ride beside noise_scale
    elif hotspots is not None:
        raise ValueError('optimize_antibody: hotspots need dock_guide (e.g. dict(guide_attract=0.5)): without a weight nothing is pulled')
    knobs = dict(dock=noise, redock=noise,          # None adds no key: the stage's options, and so its loop, are those of a call without the argument
                 design={} if design_temperature is None else dict(seq_temperature=hip.check_temperature('optimize_antibody: design_temperature', design_temperature)))
    rngs = lambda stage, lo, kk=k: dict(seed=stage_seed(seed, stage), rng_offset=stage_rng_offset(stage, lo, L, S, kk, D),
                                        **({} if depth[stage] is None else dict(steps=int(depth[stage]))), **knobs[stage])
    aa = one['aa'][0]
    f32 = dict(dtype=torch.float32, device=dev)
    clock = {}

    def tick(name, t0):
        if timings is not None:
            torch.cuda.synchronize(dev)
            clock[name] = time.perf_counter() - t0
        return time.perf_counter()

    # ---- stage 1: P poses of the docked residues (structure only), one complex encoded once per launch
    t0 = tick('start', time.perf_counter())
    pose_pos = torch.empty(mine, L, *one['pos_heavyatom'].shape[2:], **f32)
    pose_mask = torch.empty(mine, L, one['mask_heavyatom'].shape[2], dtype=torch.bool, device=dev)
    pose_ca = torch.empty(mine, n_dock, 3, **f32)
    pose_geom = torch.empty(mine, 5, dtype=torch.int64, device=dev) if geom is not None else None
    grp = chain_groups(one['fragment_type'][0])
    links = sampler.backbone_links(one['chain_nb'], one['res_nb']) if geom is not None and geom['bond_max'] is not None else None       # (1, L)
    geom_cols = ('clash', 'contacts', 'iface1', 'iface2', 'breaks')
    for lo, hi in plan:
        n = hi - lo
        traj = sampler.sample_replicated(dock_model, _with(one, **guide_extra), n, dict(sample_structure=True, sample_sequence=False, **rngs('dock', lo)))
        rep = lambda t: t.expand(n, *t.shape[1:]).contiguous()
        pos, mask = _rebuild(rep(one['pos_heavyatom']), rep(one['mask_heavyatom']), traj[0], 0, n, rep(one['aa']), gen, one)
        pose_pos[lo - a:hi - a], pose_mask[lo - a:hi - a] = pos, mask
        pose_ca[lo - a:hi - a] = traj[0][1][:, gen]
        if geom is not None:                                                             # the chunk's poses: one group of n candidates of the complex
            ig = hip.interface_geometry_grouped(pos, mask, grp[None], link=links, **geom)
            pose_geom[lo - a:hi - a] = torch.stack([ig[c] for c in geom_cols], 1).long()
    t0 = tick('dock', t0)

    # ---- optional: cluster the P poses (every rank the same gathered array); from here on "pose" c is the centre of cluster c, and a / mine / plan are the
    # shard and launches of this rank over the C centres
    pose_counts = [e - s_ for s_, e in (sampler.shard_range(P, world, r) for r in range(world))]
    clusters = None
    if cluster_cutoff is not None:
        if world > 1:
            pose_ca = sampler.all_gather_candidates(pose_ca, pose_counts, group)
            pose_pos = sampler.all_gather_candidates(pose_pos, pose_counts, group)
            pose_mask = sampler.all_gather_candidates(pose_mask.to(torch.uint8), pose_counts, group).bool()
            if geom is not None:
                pose_geom = sampler.all_gather_candidates(pose_geom, pose_counts, group)
        clusters = sampler.cluster_poses(pose_ca, cluster_cutoff, max_clusters)
        Q = int(clusters['centre'].shape[0])
        plan = launch_plan(Q, poses_per_launch, world, rank)
        a, b = sampler.shard_range(Q, world, rank)
        mine = b - a
        own = clusters['centre'][a:b]
        pose_pos, pose_mask = pose_pos[own], pose_mask[own]
        t0 = tick('cluster', t0)
    else:
        Q = P

    # ---- stage 2: S designs per pose on the fixed pose backbone, each pose encoded once, its designs share its pair features
    seqs = torch.empty(mine, S, n_design, dtype=torch.int64, device=dev)
    aar, ppl = torch.empty(mine, S, **f32), torch.empty(mine, S, **f32)
    chosen = torch.empty(mine, k, dtype=torch.int64, device=dev)
    des_pos = torch.empty(mine, k, *pose_pos.shape[1:], **f32)
    des_mask = torch.empty(mine, k, *pose_mask.shape[1:], dtype=torch.bool, device=dev)
    des_aa = torch.empty(mine, k, L, dtype=torch.int64, device=dev)
    native = aa[dflag]
    if seq_mismatch is not None:
        i64 = dict(dtype=torch.int64, device=dev)
        seq_label, seq_centre, seq_size = torch.empty(mine, S, **i64), torch.empty(mine, S, **i64), torch.empty(mine, S, **i64)
        seq_clusters, seq_counts = torch.empty(mine, **i64), torch.empty(mine, n_design, 21, **i64)
    for lo, hi in plan:
        G = hi - lo
        cx = [_with(one, pos_heavyatom=pose_pos[i - a:i - a + 1], mask_heavyatom=pose_mask[i - a:i - a + 1], generate_flag=dflag[None], **design_extra)
              for i in range(lo, hi)]
        traj = sampler.sample_grouped(design_model, cx, S, dict(sample_structure=False, sample_sequence=True, **rngs('design', lo)), pad_to=L)
        s_fin = traj[0][2]
        sq = s_fin[:, dflag]                                                             # (G*S, n_design)
        seqs[lo - a:hi - a] = sq.view(G, S, n_design)
        aar[lo - a:hi - a] = ((sq == native).sum(-1).float() / n_design).view(G, S)
        pp = traj[0][4].to(dev).view(G, S)
        ppl[lo - a:hi - a] = pp
        if seq_mismatch is not None:                                                     # the launch's poses: G groups of S designs, two grouped calls
            cl = hip.cluster_sequences_grouped(sq, S, seq_mismatch)
            seq_label[lo - a:hi - a], seq_centre[lo - a:hi - a] = cl['label'].view(G, S).long(), cl['centre'].long()
            seq_size[lo - a:hi - a], seq_clusters[lo - a:hi - a] = cl['size'].long(), cl['count'].long()
            seq_counts[lo - a:hi - a] = hip.sequence_profile_grouped(sq, S).long()
        if screen_by == 'first':
            ch = torch.arange(k, device=dev).expand(G, k)
        elif screen_by == 'diverse':
            ch = diverse_choice(cl['centre'], k)
        else:
            ch = torch.sort(pp, dim=1, stable=True)[1][:, :k]
        chosen[lo - a:hi - a] = ch
        rows = (torch.arange(G, device=dev)[:, None] * S + ch).reshape(-1)               # (G*k,) rows of the launch, pose-major
        src = (torch.arange(G, device=dev) + (lo - a)).repeat_interleave(k)
        sub = [t[rows] for t in traj[0][:3]]
        pos, mask = _rebuild(pose_pos[src], pose_mask[src], sub, 0, G * k, aa.expand(G * k, L), dflag, one)
        des_pos[lo - a:hi - a] = pos.view(G, k, *pos.shape[1:])
        des_mask[lo - a:hi - a] = mask.view(G, k, *mask.shape[1:])
        des_aa[lo - a:hi - a] = torch.where(dflag, sub[2], aa).view(G, k, L)
    t0 = tick('design', t0)

    def redock(npos, nmask, naa, rng):
        """D re-docks of each of the n given design complexes -> their rebuilt coordinates and everything that depends on the trajectories alone."""
        n = npos.shape[0]
        cx = [_with(one, pos_heavyatom=npos[i:i + 1], mask_heavyatom=nmask[i:i + 1], aa=naa[i:i + 1], generate_flag=rflag[None], **guide_extra) for i in range(n)]
        traj = sampler.sample_grouped(dock_model, cx, D, dict(sample_structure=True, sample_sequence=False, **rng), pad_to=L)
        rep = lambda t: t.repeat_interleave(D, dim=0)
        pos, mask = _rebuild(rep(npos), rep(nmask), traj[0], 0, n * D, rep(naa), rflag, one)
        out = dict(pos=pos, mask=mask, prmsd=traj[0][3].to(dev).view(n, D))
        ca = traj[0][1][:, rflag].contiguous()                                          # (n*D, n_redock, 3)
        out['redock_score'] = hip.commonness_score_grouped(ca, D).view(n, D)
        if redock_cutoff is not None:
            cl = hip.cluster_poses_grouped(ca, D, redock_cutoff)
            out['redock_cluster_frac'] = cl['size'].amax(1).float() / D
            out['redock_clusters'] = cl['count'].long()
        if geom is not None:
            ig = hip.interface_geometry_grouped(pos, mask, grp[None].expand(n, L), link=None if links is None else links.expand(n, L), want_freq=True, **geom)
            out['redock_geom'] = torch.stack([ig[c] for c in geom_cols], 1).long().view(n, D, 5)
            out['epitope_freq'] = ig['freq'].float() / D
        if lddt_cutoff is not None:                                                      # the D re-docks of every design among each other
            out['redock_consistency'] = hip.lddt_ca_ensemble(pos, mask, D, rows=rflag[None].expand(n, L), cutoff=lddt_cutoff)['consistency']
        return out

    def versus_design(rpos, rmask, dpos, dmask):
        """The D re-docks of each of n owners against the owner's design complex: one grouped DockQ launch [+ one grouped lDDT call] -> the owner fields."""
        n = dpos.shape[0]
        out = dict(dockq=hip.dockq_lite_grouped(rpos, rmask, dpos, dmask, grp[None].expand(n, L), check=False).view(n, D, 4))
        if lddt_cutoff is not None:
            ld = hip.lddt_ca_grouped(rpos, rmask, dpos, dmask, rows=rflag[None].expand(n, L), cutoff=lddt_cutoff)
            out['redock_lddt'] = ld['lddt'].view(n, D)
            out['redock_lddt_res'] = ld['lddt_res'][:, rflag].view(n, D, n_redock)
        return out

    unit_fields = ('prmsd', 'redock_score') + (('redock_cluster_frac', 'redock_clusters') if redock_cutoff is not None else ()) + \
                  (('redock_geom', 'epitope_freq') if geom is not None else ()) + (('redock_consistency',) if lddt_cutoff is not None else ())
    owner_fields = ('dockq',) + (('redock_lddt', 'redock_lddt_res') if lddt_cutoff is not None else ())      # scored against the owner's own design complex
    tail = dict(dockq=(D, 4), prmsd=(D,), redock_score=(D,), redock_cluster_frac=(), redock_clusters=(), redock_geom=(D, 5), epitope_freq=(L,),
                redock_consistency=(D,), redock_lddt=(D,), redock_lddt_res=(D, n_redock))                     # per design
    kind = dict(redock_clusters=torch.int64, redock_geom=torch.int64)
    counts = [e - s_ for s_, e in (sampler.shard_range(Q, world, r) for r in range(world))]
    shared = None
    # ---- optional: the chosen designs of all poses fall into units of identical sequence; a unit is re-docked once, from its lowest-index member's complex
    if share_redocks:
        all_pos, all_mask, all_aa = des_pos, des_mask, des_aa
        if world > 1:
            all_pos = sampler.all_gather_candidates(des_pos, counts, group)
            all_mask = sampler.all_gather_candidates(des_mask.to(torch.uint8), counts, group).bool()
            all_aa = sampler.all_gather_candidates(des_aa, counts, group)
        all_pos, all_mask, all_aa = (t.reshape(Q * k, *t.shape[2:]) for t in (all_pos, all_mask, all_aa))
        units = sampler.cluster_sequences(all_aa[:, dflag], 0)                          # identity is an equivalence: a unit's centre is its lowest-index member
        U = int(units['centre'].shape[0])
        owners = [[] for _ in range(U)]
        for i, u in enumerate(units['label'].tolist()):                                 # every rank holds the same gathered array: the same units everywhere
            owners[u].append(i)
        t0 = tick('units', t0)

        # ---- stage 3 over the U units: unit u takes the place of pose u with ONE screened design (launches, shards, Philox: global sample index u D + re-dock)
        got = {name: [] for name in unit_fields + owner_fields}
        for lo, hi in launch_plan(U, poses_per_launch, world, rank):
            own = units['centre'][lo:hi]
            r = redock(all_pos[own], all_mask[own], all_aa[own], rngs('redock', lo, 1))
            for name in unit_fields:
                got[name].append(r[name])
            # DockQ of every owner against its own design complex, from its unit's D re-docks: groups = owners, unit-major, owners ascending
            ow = torch.tensor([i for u in range(lo, hi) for i in owners[u]], dtype=torch.int64, device=dev)
            src = torch.tensor([u - lo for u in range(lo, hi) for _ in owners[u]], dtype=torch.int64, device=dev)
            rows = (src[:, None] * D + torch.arange(D, device=dev)).reshape(-1)
            vs = versus_design(r['pos'][rows], r['mask'][rows], all_pos[ow], all_mask[ow])
            for name in owner_fields:
                got[name].append(vs[name])
        got = {name: (torch.cat(v, 0) if v else torch.empty(0, *tail[name], dtype=kind.get(name, torch.float32), device=dev)) for name, v in got.items()}
        if world > 1:
            ucounts = [e - s_ for s_, e in (sampler.shard_range(U, world, r) for r in range(world))]
            ocounts = [sum(len(owners[u]) for u in range(*sampler.shard_range(U, world, r))) for r in range(world)]
            got = {name: sampler.all_gather_candidates(t, ocounts if name in owner_fields else ucounts, group) for name, t in got.items()}
        order = torch.tensor([i for u in range(U) for i in owners[u]], dtype=torch.int64, device=dev)
        shared = {name: got[name][units['label']].view(Q, k, *got[name].shape[1:]) for name in unit_fields}      # a unit's rows, copied to every owner (pose, slot)
        for name in owner_fields:
            shared[name] = torch.empty(Q * k, *tail[name], **f32).index_copy_(0, order, got[name]).view(Q, k, *tail[name])
        shared.update(design_unit=units['label'].view(Q, k), unit_owner=units['centre'], unit_size=units['size'])
        plan = []                                                                        # stage 3 is done

    # ---- stage 3: D re-docks of every screened design, one grouped DockQ + one grouped commonness launch per chunk
    owner3 = {name: torch.empty(mine, k, *tail[name], **f32) for name in owner_fields}
    stage3 = {name: torch.empty(mine, k, *tail[name], dtype=kind.get(name, torch.float32), device=dev) for name in unit_fields}
    for lo, hi in plan:
        Gk = (hi - lo) * k
        npos, nmask, naa = (t[lo - a:hi - a].reshape(Gk, *t.shape[2:]) for t in (des_pos, des_mask, des_aa))
        r = redock(npos, nmask, naa, rngs('redock', lo))
        vs = versus_design(r['pos'], r['mask'], npos, nmask)
        for name in owner_fields:
            owner3[name][lo - a:hi - a] = vs[name].view(hi - lo, k, *tail[name])
        for name in unit_fields:
            stage3[name][lo - a:hi - a] = r[name].view(hi - lo, k, *r[name].shape[1:])
    t0 = tick('redock', t0)

    res = dict(pose_ca=pose_ca, seqs=seqs, aar=aar, ppl=ppl, chosen=chosen)
    if shared is None:
        res.update(**owner3, **stage3)
    if geom is not None:
        res.update(pose_geom=pose_geom)
    if seq_mismatch is not None:
        res.update(seq_label=seq_label, seq_centre=seq_centre, seq_size=seq_size, seq_clusters=seq_clusters, seq_counts=seq_counts)
    pose_fields = ('pose_ca', 'pose_geom')                                               # P rows whatever the clustering does
    if world > 1:
        gathered = {} if clusters is None else {name: res.pop(name) for name in pose_fields if name in res}     # the clustered poses were gathered before stage 2
        res = {name: sampler.all_gather_candidates(t, pose_counts if name in pose_fields else counts, group) for name, t in res.items()}
        res.update(gathered)
    if shared is not None:                                                               # gathered over the units' ranks above
        res.update(shared)
    if clusters is not None:
        res.update(cluster_label=clusters['label'], cluster_centre=clusters['centre'], cluster_size=clusters['size'])
    res['pose_score'] = hip.commonness_score(res['pose_ca'])
    q, pr = res['dockq'][..., 3], res['prmsd']
    res.update(dockq_mean=q.mean(-1), dockq_std=q.std(-1, unbiased=False), prmsd_mean=pr.mean(-1), prmsd_std=pr.std(-1, unbiased=False))
    if lddt_cutoff is not None:
        res['lddt_mean'], res['lddt_std'] = _scored_mean_std(res['redock_lddt'], -1)
        res['lddt_res_mean'] = _scored_mean_std(res['redock_lddt_res'], 2)[0]
    tick('gather', t0)
    if timings is not None:
        clock.pop('start', None)
        timings.update(clock)
    return res


def screen_filter(res, max_clashes=None, min_contacts=None, min_lddt=None):
    """The notebook's median rule (ab_opt_analysis_4mutations.ipynb, cell 7): keep the designs whose DockQ_std, prmsd_std and prmsd_avg
    are each at or below the median over all screened designs (pandas' quantile(0.5): the mean of the two middle values for an even count).
    max_clashes / min_contacts (optional; need the redock_geom of optimize_antibody(clash_cutoff=...)): additionally require, per design, that the MEDIAN over
    its D re-docks (the same quantile) of the clash count is <= max_clashes and of the contact count is >= min_contacts.
    min_lddt (optional; needs the redock_lddt of optimize_antibody(lddt_cutoff=...)): additionally require that the MEDIAN over a design's D re-docks of the pooled
    lDDT against the design is >= min_lddt (a re-dock without a scored pair enters with its -1).
    -> bool (P, k)."""
    med = lambda t: torch.quantile(t.reshape(-1).double(), 0.5)
    keep = torch.ones_like(res['dockq_std'], dtype=torch.bool)
    for name in ('dockq_std', 'prmsd_std', 'prmsd_mean'):
        t = res[name]
        keep &= t.double() <= med(t)
    if max_clashes is not None or min_contacts is not None:
        if 'redock_geom' not in res:
            raise ValueError('screen_filter: max_clashes / min_contacts need redock_geom (run optimize_antibody with clash_cutoff, contact_cutoff or bond_max)')
        over_d = torch.quantile(res['redock_geom'].double(), 0.5, dim=2)                  # (., k, 5)
        if max_clashes is not None:
            keep &= over_d[..., 0] <= float(max_clashes)
        if min_contacts is not None:
            keep &= over_d[..., 1] >= float(min_contacts)
    if min_lddt is not None:
        if 'redock_lddt' not in res:
            raise ValueError('screen_filter: min_lddt needs redock_lddt (run optimize_antibody with lddt_cutoff)')
        keep &= torch.quantile(res['redock_lddt'].double(), 0.5, dim=-1) >= float(min_lddt)
    return keep
