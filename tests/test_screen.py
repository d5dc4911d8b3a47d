"""The dock -> redesign -> re-dock screen (ab_opt_amd/screen.py) and its grouped scoring kernels (abopt_dockq_lite_grouped,
abopt_commonness_score_grouped).  The planning and filtering tests run on the CPU; the rest need an MI355X."""
import numpy as np
import pytest
import torch

import cases
import screen_workers
from ab_opt_amd import screen
from ab_opt_amd.model import generate_mask_from_str
from ab_opt_amd.utils import synth

DEV = torch.device('cuda:0')
STAGE_KW = dict(designs_per_pose=3, screened_per_pose=2, redocks_per_design=4)


# ------------------------------------------------------------------------------------------ CPU: partition, counters, masks, filter
@pytest.mark.parametrize('P', [1, 7, 12])
@pytest.mark.parametrize('per_launch', [1, 3, 100])
def test_pose_partition_covers_every_pose_once(P, per_launch):
    for world in range(1, 6):
        seen = []
        for rank in range(world):
            plan = screen.launch_plan(P, per_launch, world, rank)
            a, b = screen.launch_plan(P, 10 ** 9, world, rank)[0] if plan else (None, None)
            for lo, hi in plan:
                assert 0 < hi - lo <= per_launch and a <= lo < hi <= b
                seen += range(lo, hi)
        assert sorted(seen) == list(range(P)), (P, per_launch, world)


def test_stage_rng_offsets_tile_the_counter_space():
    """Every launch of every rank reads [offset, offset + poses x samples_per_pose x L): over all launches and ranks these ranges tile
    [0, P x samples_per_pose x L) without gap or overlap, and sample j of a launch sits at (its global index) x L."""
    L = 37
    for stage in screen.STAGES:
        spp = screen.samples_per_pose(stage, **STAGE_KW)
        for P in (5, 11):
            for per_launch in (1, 2, 4, P):
                for world in range(1, 6):
                    ranges = []
                    for rank in range(world):
                        for lo, hi in screen.launch_plan(P, per_launch, world, rank):
                            off = screen.stage_rng_offset(stage, lo, L, **STAGE_KW)
                            assert off == lo * spp * L
                            ranges.append((off, off + (hi - lo) * spp * L))
                    ranges.sort()
                    assert ranges[0][0] == 0 and ranges[-1][1] == P * spp * L
                    assert all(x[1] == y[0] for x, y in zip(ranges, ranges[1:])), (stage, P, per_launch, world)
    seeds = {screen.stage_seed(s, st) for s in range(5) for st in screen.STAGES}
    assert len(seeds) == 15


def test_contig_mask_is_generate_mask_from_str_and_design_flag():
    flag = torch.zeros(40, dtype=torch.bool)
    flag[10:22] = True
    for contig in ('3-7', '1-40', '12-30', '25-31'):
        want = torch.logical_and(generate_mask_from_str(contig, flag), flag)
        assert torch.equal(screen.design_mask(flag, contig), want), contig
    assert torch.equal(screen.design_mask(flag, ''), flag)
    assert screen.design_mask(flag, '25-31').sum() == 0


def test_screen_filter_applies_the_notebooks_median_rule():
    """ab_opt_analysis_4mutations.ipynb: rows with DockQ_std, prmsd_std and prmsd_avg each <= its median (pandas quantile(0.5))."""
    dq_std = torch.tensor([[0.10, 0.30], [0.05, 0.20], [0.15, 0.08]])
    pr_std = torch.tensor([[0.20, 0.01], [0.02, 0.30], [0.10, 0.05]])
    pr_avg = torch.tensor([[1.5, 1.2], [1.3, 1.9], [1.4, 1.1]])
    keep = screen.screen_filter(dict(dockq_std=dq_std, prmsd_std=pr_std, prmsd_mean=pr_avg))
    # medians over the 6 designs: DockQ_std 0.125, prmsd_std 0.075, prmsd_avg 1.35 -> rows (1, 0) and (2, 1) pass all three
    assert keep.tolist() == [[False, False], [True, False], [False, True]]
    g = torch.Generator().manual_seed(3)
    for n in (7, 10):
        t = {k: torch.rand(n, 1, generator=g) for k in ('dockq_std', 'prmsd_std', 'prmsd_mean')}
        keep = screen.screen_filter(t)
        a = {k: v.flatten().numpy().astype(np.float64) for k, v in t.items()}
        want = np.ones(n, dtype=bool)
        for k in a:
            want &= a[k] <= np.quantile(a[k], 0.5)
        assert keep.flatten().tolist() == want.tolist()


# ------------------------------------------------------------------------------------------ GPU: grouped scoring kernels
def _dockq_groups(G=3, S=5):
    cs = [cases.dockq_case(S=S, seed=31 + 7 * g) for g in range(G)]
    pos, mask, grp = (torch.stack([c[i] for c in cs]).to(DEV) for i in range(3))
    models = torch.cat([c[3] for c in cs]).to(DEV)
    return pos, mask, grp, models


@pytest.mark.gpu
def test_dockq_lite_grouped_equals_per_group_calls():
    """G = 3 natives x S = 5 candidates in one launch against three abopt_dockq_lite launches, bit for bit: per-candidate masks (one candidate
    with no CA atom at all -> -1 markers) and masks shared per native; and against oracle/dockq.py to the tolerance of
    test_dockq_lite_vs_reference."""
    from ab_opt_amd import hip
    from oracle import dockq as odq
    G, S = 3, 5
    pos, mask, grp, models = _dockq_groups(G, S)
    per_cand = mask.repeat_interleave(S, 0).clone()
    per_cand[1 * S + 2, :, 1] = False                                   # candidate 2 of native 1: no CA -> empty selections
    out = hip.dockq_lite_grouped(models, per_cand, pos, mask, grp, check=False)
    shared = hip.dockq_lite_grouped(models, mask, pos, mask, grp, check=False)
    assert out.shape == (G * S, 4)
    for g in range(G):
        sl = slice(g * S, (g + 1) * S)
        assert torch.equal(out[sl], hip.dockq_lite(models[sl], per_cand[sl], pos[g], mask[g], grp[g], check=False)), g
        assert torch.equal(shared[sl], hip.dockq_lite(models[sl], mask[g], pos[g], mask[g], grp[g], check=False)), g
    bad = 1 * S + 2
    assert out[bad, 1].item() == -1 and out[bad, 2].item() == -1 and out[bad, 3].item() == -1
    assert (out[torch.arange(G * S) != bad, 3] >= 0).all()
    with pytest.raises(ValueError, match='empty'):
        hip.dockq_lite_grouped(models, per_cand, pos, mask, grp)
    for c in range(G * S):
        g = c // S
        ref = odq.dockq(models[c].cpu().numpy(), mask[g].cpu().numpy(), pos[g].cpu().numpy(), mask[g].cpu().numpy(), grp[g].cpu().numpy())
        for j, k in enumerate(('fnat', 'irms', 'Lrms', 'DockQ')):
            assert abs(shared[c, j].item() - ref[k]) < 1e-4, (c, k)


@pytest.mark.gpu
def test_commonness_score_grouped_equals_per_group_calls():
    from ab_opt_amd import hip
    for G, S, n in ((4, 6, 36), (3, 2, 5), (2, 9, 101)):
        x = synth.hash_tensor((G * S, n, 3), 70 + S, scale=8.0).to(DEV)
        got = hip.commonness_score_grouped(x, S)
        for g in range(G):
            assert torch.equal(got[g * S:(g + 1) * S], hip.commonness_score(x[g * S:(g + 1) * S])), (G, S, n, g)


# ------------------------------------------------------------------------------------------ GPU: the screen
def _composition(dock, design, one, P, S, k, D, contig, seed):
    """The screen written out with the public calls (one launch per stage): sample_replicated -> reconstruct_backbone_partially ->
    sample_grouped -> rebuild -> dockq_lite / commonness_score per design."""
    from ab_opt_amd import geometry, hip, sampler
    rep = lambda t, n: t.expand(n, *t.shape[1:]).contiguous()
    aa, cn, rn = one['aa'], one['chain_nb'], one['res_nb']
    gen = one['generate_flag'][0]
    t1 = sampler.sample_replicated(dock, one, P, dict(sample_structure=True, sample_sequence=False, seed=screen.stage_seed(seed, 'dock'), rng_offset=0))[0]
    g1 = rep(gen[None], P)
    pose_pos, pose_mask = geometry.reconstruct_backbone_partially(rep(one['pos_heavyatom'], P), hip.so3_exp(t1[0]), t1[1], torch.where(g1, t1[2], rep(aa, P)),
                                                                  rep(cn, P), rep(rn, P), rep(one['mask_heavyatom'], P), g1)
    out = dict(pose_ca=t1[1][:, gen], pose_score=hip.commonness_score(t1[1][:, gen]))
    dflag = gen & generate_mask_from_str(contig, gen)
    cx = [dict(one, pos_heavyatom=pose_pos[i:i + 1], mask_heavyatom=pose_mask[i:i + 1], generate_flag=dflag[None]) for i in range(P)]
    t2 = sampler.sample_grouped(design, cx, S, dict(sample_structure=False, sample_sequence=True, seed=screen.stage_seed(seed, 'design'), rng_offset=0))[0]
    g2 = rep(dflag[None], P * S)
    aa2 = torch.where(g2, t2[2], rep(aa, P * S))
    des_pos, des_mask = geometry.reconstruct_backbone_partially(pose_pos.repeat_interleave(S, 0), hip.so3_exp(t2[0]), t2[1], aa2, rep(cn, P * S), rep(rn, P * S),
                                                                pose_mask.repeat_interleave(S, 0), g2)
    ppl = t2[4].to(DEV).view(P, S)
    chosen = torch.sort(ppl, dim=1, stable=True)[1][:, :k]
    out.update(seqs=t2[2][:, dflag].view(P, S, -1), ppl=ppl, chosen=chosen)
    rows = (torch.arange(P, device=DEV)[:, None] * S + chosen).reshape(-1)
    npos, nmask, naa = des_pos[rows], des_mask[rows], aa2[rows]
    cx = [dict(one, pos_heavyatom=npos[i:i + 1], mask_heavyatom=nmask[i:i + 1], aa=naa[i:i + 1], generate_flag=gen[None]) for i in range(P * k)]
    t3 = sampler.sample_grouped(dock, cx, D, dict(sample_structure=True, sample_sequence=False, seed=screen.stage_seed(seed, 'redock'), rng_offset=0))[0]
    g3 = rep(gen[None], P * k * D)
    rpos, rmask = geometry.reconstruct_backbone_partially(npos.repeat_interleave(D, 0), hip.so3_exp(t3[0]), t3[1], torch.where(g3, t3[2], naa.repeat_interleave(D, 0)),
                                                          rep(cn, P * k * D), rep(rn, P * k * D), nmask.repeat_interleave(D, 0), g3)
    grp = screen.chain_groups(one['fragment_type'][0])
    dq, sc = [], []
    for i in range(P * k):
        sl = slice(i * D, (i + 1) * D)
        dq.append(hip.dockq_lite(rpos[sl], rmask[sl], npos[i], nmask[i], grp, check=False))
        sc.append(hip.commonness_score(t3[1][sl][:, gen]))
    out.update(dockq=torch.stack(dq).view(P, k, D, 4), redock_score=torch.stack(sc).view(P, k, D), prmsd=t3[3].to(DEV).view(P, k, D))
    return out


@pytest.mark.gpu
def test_optimize_antibody_equals_the_composition_of_public_calls():
    """optimize_antibody (all poses in one launch per stage) against the same screen written out with the public calls, bit for bit: pose CA
    and commonness, designed sequences, PPL (= traj[0][4] of the design stage), the PPL-screened designs, DockQ and prmsd of every re-dock,
    the re-docks' commonness.  AAR is a recount of the returned sequences; every field is finite."""
    P, S, k, D, contig, seed = 4, 3, 2, 3, '33-39', 5
    dock, design = screen_workers.models(DEV)
    one = screen_workers.complex_(DEV)
    want = _composition(dock, design, one, P, S, k, D, contig, seed)
    res = screen.optimize_antibody(dock, design, one, P, S, D, contig=contig, screened_per_pose=k, seed=seed, poses_per_launch=P, screen_by='ppl')
    for name, v in want.items():
        assert res[name].shape == v.shape and torch.equal(res[name], v), name
    for name, v in res.items():
        assert v.is_cuda and torch.isfinite(v.float()).all(), name
    gen = one['generate_flag'][0]
    dflag = screen.design_mask(gen, contig)
    assert res['seqs'].shape == (P, S, int(dflag.sum())) and int(dflag.sum()) == 7
    assert torch.equal(res['aar'], (res['seqs'] == one['aa'][0][dflag]).sum(-1).float() / int(dflag.sum()))
    q = res['dockq'][..., 3]
    assert torch.equal(res['dockq_mean'], q.mean(-1)) and torch.equal(res['dockq_std'], q.std(-1, unbiased=False))
    assert (q >= 0).all() and (q <= 1).all()
    assert screen.screen_filter(res).shape == (P, k)


@pytest.mark.gpu
def test_optimize_antibody_does_not_depend_on_poses_per_launch(monkeypatch):
    """1, 2 and P poses per launch give the same screen bit for bit.  What this pins is one arithmetic form: launches of different sizes may
    otherwise take the 32-row fp16-term kernels or the 16-row fp32 ones (equal to fp32 noise only) and small launches
    the key-split IPA core (another summation order); ABOPT_PAIR_TERMS=0 and ABOPT_CORE_NO_SPLIT=1 keep every launch on the fp32 stream
    and the unsplit core, as test_config4_rank_leg_grouped_launch does."""
    monkeypatch.setenv('ABOPT_PAIR_TERMS', '0')
    monkeypatch.setenv('ABOPT_CORE_NO_SPLIT', '1')
    dock, design = screen_workers.models(DEV)
    one = screen_workers.complex_(DEV)
    kw = dict(screen_workers.SCREEN)
    runs = [screen.optimize_antibody(dock, design, one, poses_per_launch=n, **kw) for n in (kw['num_poses'], 1, 2)]
    for r in runs[1:]:
        for name, v in runs[0].items():
            assert torch.equal(r[name], v), name


@pytest.mark.gpu
def test_two_rank_screen_equals_one_rank(tmp_path, monkeypatch):
    """Two ranks sharing cuda:0 (gloo; 5 poses split 3 + 2, two poses per launch) gather the same result as one process, bit for bit
    (ABOPT_PAIR_TERMS=0 / ABOPT_CORE_NO_SPLIT=1, as in test_optimize_antibody_does_not_depend_on_poses_per_launch)."""
    from scorer_harness import spawn2
    monkeypatch.setenv('ABOPT_PAIR_TERMS', '0')
    monkeypatch.setenv('ABOPT_CORE_NO_SPLIT', '1')
    dock, design = screen_workers.models(DEV)
    ref = screen.optimize_antibody(dock, design, screen_workers.complex_(DEV), poses_per_launch=5, **screen_workers.SCREEN)
    spawn2(screen_workers.screen_worker, tmp_path)
    for r in range(2):
        got = torch.load(tmp_path / f'screen_{r}.pt')
        assert set(got) == set(ref)
        for name, v in ref.items():
            assert torch.equal(got[name], v.cpu()), (r, name)
