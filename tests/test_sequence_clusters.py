"""Sequence clustering and composition: abopt_cluster_sequences_grouped / abopt_sequence_profile_grouped, their bindings
(hip.cluster_sequences_grouped, hip.sequence_profile_grouped, sampler.cluster_sequences, sampler.sequence_profile) and the screen's sequence side
(screen.optimize_antibody(seq_mismatch=..., screen_by='diverse', share_redocks=True)).

The definition is restated below in integer numpy (`hamming`, `greedy`, `profile`, `diverse_rule`, `units_of`).  Everything is an integer, so every
comparison is exact equality; the float fields of the screen are compared bit for bit (torch.equal) with the composition of public calls."""
import functools

import numpy as np
import pytest
import torch

import scorer_harness as harness
import screen_workers
import sequence_cluster_workers as workers
from ab_opt_amd import screen
from ab_opt_amd.model import generate_mask_from_str
from scorer_harness import screen_models                           # noqa: F401 (the fixture)

DEV = torch.device('cuda:0')
S_LIST = (1, 2, 63, 64, 65, 130)
N_LIST = (1, 3, 4, 5, 63, 64, 65, 200)        # the kernel packs 4 residues per word and stages 64 residues per LDS chunk; 200 takes four chunks
BYTES = np.array(list(range(20)) + [20, 21, 255], dtype=np.uint8)


# ------------------------------------------------------------------------------------------ the integer statement and the inputs
def hamming(x):
    """(S, n) -> (S, S) int64: the number of positions at which two sequences differ."""
    x = np.asarray(x)
    return (x[:, None, :] != x[None, :, :]).sum(-1).astype(np.int64)


def greedy(x, max_mismatch, max_clusters=0):
    """The definition (include/abopt.h: abopt_cluster_sequences_grouped) for ONE group x (S, n) -> (label [S], centre [C], size [C])."""
    S = len(x)
    adj = hamming(x) <= int(max_mismatch)
    adj[np.arange(S), np.arange(S)] = True
    alive = np.ones(S, dtype=bool)
    label, centre, size = -np.ones(S, dtype=np.int64), [], []
    while alive.any() and not (max_clusters and len(centre) >= max_clusters):
        cnt = (adj & alive[None]).sum(1)
        cnt[~alive] = -1
        c = int(np.argmax(cnt))                                     # the first maximum: ties go to the lowest index
        members = adj[c] & alive
        label[members] = len(centre)
        centre.append(c)
        size.append(int(members.sum()))
        alive &= ~members
    return label, np.array(centre, dtype=np.int64), np.array(size, dtype=np.int64)


def profile(x):
    """(S, n) -> (n, 21) int64: np.bincount per position, every byte >= 20 in bin 20."""
    x = np.minimum(np.asarray(x).astype(np.int64), 20)
    return np.stack([np.bincount(x[:, p], minlength=21) for p in range(x.shape[1])])


def diverse_rule(x, max_mismatch, k):
    """The designs screen_by='diverse' re-docks: the centres of the first min(k, C) clusters in order of discovery, then the lowest indices not yet chosen."""
    chosen = greedy(x, max_mismatch)[1][:k].tolist()
    for i in range(len(x)):
        if len(chosen) < k and i not in chosen:
            chosen.append(i)
    return chosen


def units_of(x):
    """Classes of identical sequences among x (N, n), in the kernel's order -> (unit of every sequence [N], lowest-index member [U], members [U])."""
    label, centre, size = greedy(x, 0)
    assert all(centre[u] == np.flatnonzero(label == u)[0] for u in range(len(centre)))
    return label, centre, size


@functools.lru_cache(maxsize=None)
def case(G, S, n):
    """Four random seed sequences over BYTES (the 20 types, 20, 21 and 255) and, per sequence of the case, a copy of one of them mutated at 0, 0, 1, 2 or 3
    positions: identical copies, near copies and strangers, so clusters of several sizes and equal counts occur.  -> (G*S, n) uint8 numpy, built once."""
    rng = np.random.default_rng(100000 * G + 1000 * S + n)
    seeds = BYTES[rng.integers(0, len(BYTES), size=(4, n))]
    x = seeds[rng.integers(0, 4, size=G * S)].copy()
    for i in range(G * S):
        for p in rng.choice(n, size=min(n, int(rng.choice([0, 0, 1, 2, 3]))), replace=False):
            x[i, p] = rng.choice(BYTES[BYTES != x[i, p]])
    x[0, 0] = 255
    if G * S > 1:
        x[1, n - 1] = 21
    if G * S > 2:
        x[2, n // 2] = 20
    return x


def _assert_equals_statement(out, x, G, S, m, cap, tag):
    label, centre, size, count = (out[k].cpu().numpy() for k in ('label', 'centre', 'size', 'count'))
    assert label.shape == (G * S,) and centre.shape == (G, S) and size.shape == (G, S) and count.shape == (G,), tag
    assert all(out[k].dtype == torch.int32 for k in ('label', 'centre', 'size', 'count')), tag
    for g in range(G):
        wl, wc, ws = greedy(x[g * S:(g + 1) * S], m, cap)
        C = len(wc)
        assert count[g] == C, (tag, g, count[g], C)
        assert np.array_equal(label[g * S:(g + 1) * S], wl), (tag, g)
        assert np.array_equal(centre[g, :C], wc) and (centre[g, C:] == -1).all(), (tag, g)
        assert np.array_equal(size[g, :C], ws) and (size[g, C:] == 0).all(), (tag, g)
        if cap:
            assert C <= cap and (wl == -1).sum() == S - ws.sum(), (tag, g)


# ------------------------------------------------------------------------------------------ CPU
def test_statement_on_a_hand_worked_example_with_a_tie():
    """Six sequences of four residues, max_mismatch 1.  Distances: d(0,1) = d(1,2) = d(3,4) = 1, d(0,2) = 2, everything else 3 or 4: neighbour counts
    2, 3, 2, 2, 2, 1.  Sequence 1 is picked first and takes {0, 1, 2}; 3 and 4 then tie at 2 and the lower index wins; 5 is a singleton.  With a cap of 2,
    sequence 5 keeps label -1.  The profile: position 2 holds types 0, 0, 1, 2, 2 and one byte 21 -- types 0 and 2 tie and the consensus is 0."""
    x = np.array([[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 1], [2, 2, 2, 2], [2, 2, 2, 3], [21, 21, 21, 21]], dtype=np.uint8)
    d = hamming(x)
    assert d[0].tolist() == [0, 1, 2, 4, 4, 4] and d[3].tolist() == [4, 4, 4, 0, 1, 4] and np.array_equal(d, d.T)
    label, centre, size = greedy(x, 1)
    assert label.tolist() == [0, 0, 0, 1, 1, 2] and centre.tolist() == [1, 3, 5] and size.tolist() == [3, 2, 1]
    label, centre, size = greedy(x, 1, max_clusters=2)
    assert label.tolist() == [0, 0, 0, 1, 1, -1] and centre.tolist() == [1, 3] and size.tolist() == [3, 2]
    label, centre, size = greedy(x, 0)
    assert label.tolist() == [0, 1, 2, 3, 4, 5] and centre.tolist() == [0, 1, 2, 3, 4, 5]
    assert greedy(x, 4)[1].tolist() == [0] and greedy(x, 4)[2].tolist() == [6]                  # max_mismatch >= n: one cluster, every count ties
    c = profile(x)
    assert c.shape == (4, 21) and (c.sum(1) == 6).all()
    assert c[2, :4].tolist() == [2, 1, 2, 0] and c[2, 20] == 1 and c[3, :4].tolist() == [1, 2, 1, 1] and c[0, :3].tolist() == [3, 0, 2]
    assert diverse_rule(x, 1, 2) == [1, 3] and diverse_rule(x, 1, 4) == [1, 3, 5, 0] and diverse_rule(x, 4, 3) == [0, 1, 2]
    dup = x[[0, 3, 0, 5, 3, 0]]
    label, owner, size = units_of(dup)
    assert label.tolist() == [0, 1, 0, 2, 1, 0] and owner.tolist() == [0, 1, 3] and size.tolist() == [3, 2, 1]
    from ab_opt_amd import sampler
    consensus, entropy = sampler.profile_summary(torch.from_numpy(c))
    assert consensus.tolist() == [0, 0, 0, 1] and entropy.dtype == torch.float32
    p = np.array([3, 2, 1]) / 6.0
    assert abs(entropy[0].item() - float(-(p * np.log(p)).sum())) < 1e-6
    assert screen.diverse_choice(torch.tensor([[1, 3, 5, -1, -1, -1], [0, -1, -1, -1, -1, -1]]), 4).tolist() == [[1, 3, 5, 0], [0, 1, 2, 3]]
    assert screen.diverse_choice(torch.tensor([[2, 0, 1]]), 2).tolist() == [[2, 0]]


def test_arguments_are_validated_without_a_device():
    """Negative max_mismatch, screen_by='diverse' without seq_mismatch, share_redocks with a redock_flag that misses a docked residue and P k > 16384 raise
    ValueError before anything touches a device (CPU tensors, the models are None); valid arguments reach the binding, which refuses CPU tensors."""
    from ab_opt_amd import hip, sampler
    from ab_opt_amd.utils import synth
    seqs = torch.zeros(4, 7, dtype=torch.int64)
    for bad in (-1, -7):
        with pytest.raises(ValueError, match='max_mismatch'):
            hip.cluster_sequences_grouped(seqs, 4, bad)
        with pytest.raises(ValueError, match='max_mismatch'):
            sampler.cluster_sequences(seqs, bad)
    with pytest.raises(ValueError, match='max_clusters'):
        hip.cluster_sequences_grouped(seqs, 4, 1, max_clusters=-1)
    with pytest.raises(ValueError, match='max_clusters'):
        sampler.cluster_sequences(seqs, 1, max_clusters=0)
    with pytest.raises(ValueError, match='whole groups'):
        hip.cluster_sequences_grouped(seqs, 3, 1)
    with pytest.raises(ValueError, match='whole groups'):
        hip.sequence_profile_grouped(seqs.float(), 4)
    for call in (lambda: hip.cluster_sequences_grouped(seqs, 4, 1), lambda: hip.sequence_profile_grouped(seqs, 4),
                 lambda: sampler.cluster_sequences(seqs, 1, max_clusters=2), lambda: sampler.sequence_profile(seqs)):
        with pytest.raises(RuntimeError, match='HIP device only'):
            call()
    one = synth.make_batch(1, synth.LAYOUT_128, seed=21)
    call = lambda P=4, S=2, D=2, **kw: screen.optimize_antibody(None, None, one, P, S, D, **kw)
    with pytest.raises(ValueError, match='seq_mismatch'):
        call(seq_mismatch=-1)
    with pytest.raises(ValueError, match='needs seq_mismatch'):
        call(screen_by='diverse')
    with pytest.raises(ValueError, match='screen_by'):
        call(screen_by='other', seq_mismatch=1)
    gen = one['generate_flag'][0].bool()
    short = gen.clone()
    short[int(torch.nonzero(gen)[0])] = False
    with pytest.raises(ValueError, match='every docked residue'):
        call(share_redocks=True, redock_flag=short)
    with pytest.raises(ValueError, match='16384'):
        call(P=8193, S=2, screened_per_pose=2, share_redocks=True)


# ------------------------------------------------------------------------------------------ GPU: the kernels
@pytest.mark.gpu
def test_clusters_equal_the_integer_statement():
    """label, centre, size and count of the device call are those of the numpy statement over S in {1, 2, 63, 64, 65, 130} x n on both sides of the word (4) and
    LDS chunk (64) boundaries x G in {1, 3} x max_mismatch in {0, 1, 2, n}; the inputs hold the bytes 20, 21 and 255, and int64 input equals uint8 input."""
    from ab_opt_amd import hip, sampler
    for G in (1, 3):
        for S in S_LIST:
            for n in N_LIST:
                x = case(G, S, n)
                xd = torch.from_numpy(x).to(DEV)
                for m in (0, 1, 2, n):
                    out = hip.cluster_sequences_grouped(xd, S, m)
                    _assert_equals_statement(out, x, G, S, m, 0, (G, S, n, m))
    x = case(1, 130, 5)
    _, _, size = greedy(x, 1)
    assert (size > 1).sum() >= 2 and (size == 1).sum() >= 1 and len(set(size[size > 1].tolist())) >= 2, size       # the inputs exercise clusters of several sizes
    assert {20, 21, 255} <= set(x.reshape(-1).tolist())
    wide = hip.cluster_sequences_grouped(torch.from_numpy(x.astype(np.int64)).to(DEV), 130, 1)
    narrow = hip.cluster_sequences_grouped(torch.from_numpy(x).to(DEV), 130, 1)
    for k in narrow:
        assert torch.equal(wide[k], narrow[k]), k
    got = sampler.cluster_sequences(torch.from_numpy(x).to(DEV), 1, max_clusters=3)
    wl, wc, ws = greedy(x, 1, 3)
    assert all(got[k].dtype == torch.int64 and got[k].is_cuda for k in ('label', 'centre', 'size'))
    assert got['label'].tolist() == wl.tolist() and got['centre'].tolist() == wc.tolist() and got['size'].tolist() == ws.tolist()


@pytest.mark.gpu
def test_cap_leaves_the_rest_unlabelled():
    """max_clusters 1 and 3: the first clusters of the uncapped run, everything else label -1, centre / size padded with -1 / 0."""
    from ab_opt_amd import hip
    for G, S, n in ((1, 65, 5), (3, 130, 64), (3, 2, 1), (1, 64, 65)):
        x = case(G, S, n)
        xd = torch.from_numpy(x).to(DEV)
        for m in (0, 1):
            for cap in (1, 3):
                _assert_equals_statement(hip.cluster_sequences_grouped(xd, S, m, max_clusters=cap), x, G, S, m, cap, (G, S, n, m, cap))
    out = hip.cluster_sequences_grouped(torch.from_numpy(case(1, 130, 5)).to(DEV), 130, 0, max_clusters=3)
    assert (out['label'] == -1).sum() > 0


@pytest.mark.gpu
def test_dist_matrix_equals_the_statement_and_is_symmetric():
    from ab_opt_amd import hip
    for G in (1, 3):
        for S in S_LIST:
            for n in N_LIST:
                x = case(G, S, n)
                xd = torch.from_numpy(x).to(DEV)
                out = hip.cluster_sequences_grouped(xd, S, 1, want_dist=True)
                d = out['dist']
                assert d.shape == (G, S, S) and d.dtype == torch.int32
                assert torch.equal(d, d.transpose(1, 2).contiguous()), (G, S, n)
                want = np.stack([hamming(x[g * S:(g + 1) * S]) for g in range(G)])
                assert np.array_equal(d.cpu().numpy(), want), (G, S, n)
                plain = hip.cluster_sequences_grouped(xd, S, 1)
                for k in plain:
                    assert torch.equal(out[k], plain[k]), (G, S, n, k)


@pytest.mark.gpu
def test_grouped_call_equals_per_group_calls():
    from ab_opt_amd import hip
    for S in S_LIST:
        for n in (1, 5, 64, 200):
            x = torch.from_numpy(case(3, S, n)).to(DEV)
            for cap in (0, 2):
                got = hip.cluster_sequences_grouped(x, S, 1, max_clusters=cap, want_dist=True)
                counts = hip.sequence_profile_grouped(x, S)
                for g in range(3):
                    one = hip.cluster_sequences_grouped(x[g * S:(g + 1) * S], S, 1, max_clusters=cap, want_dist=True)
                    assert torch.equal(got['label'][g * S:(g + 1) * S], one['label']), (S, n, cap, g)
                    for k in ('centre', 'size', 'count', 'dist'):
                        assert torch.equal(got[k][g:g + 1], one[k]), (S, n, cap, g, k)
                    assert torch.equal(counts[g:g + 1], hip.sequence_profile_grouped(x[g * S:(g + 1) * S], S)), (S, n, g)


@pytest.mark.gpu
def test_profile_counts_equal_bincount():
    """counts == np.bincount per position with every byte >= 20 in bin 20; each position sums to S; consensus and entropy of sampler.sequence_profile are
    profile_summary of those counts (the lowest type on a tie)."""
    from ab_opt_amd import hip, sampler
    for G in (1, 3):
        for S in S_LIST + (1025,):
            for n in N_LIST:
                x = case(G, S, n)
                c = hip.sequence_profile_grouped(torch.from_numpy(x).to(DEV), S)
                assert c.shape == (G, n, 21) and c.dtype == torch.int32
                want = np.stack([profile(x[g * S:(g + 1) * S]) for g in range(G)])
                assert np.array_equal(c.cpu().numpy(), want), (G, S, n)
                assert (c.sum(-1) == S).all(), (G, S, n)
    x = case(1, 130, 5)
    got = sampler.sequence_profile(torch.from_numpy(x.astype(np.int64)).to(DEV))
    want = profile(x)
    assert np.array_equal(got['counts'].cpu().numpy(), want)
    lowest = [min(t for t in range(20) if want[p, t] == want[p, :20].max()) for p in range(5)]
    assert got['consensus'].tolist() == lowest and got['consensus'].dtype == torch.int64
    consensus, entropy = sampler.profile_summary(torch.from_numpy(want))
    assert got['entropy'].dtype == torch.float32 and got['entropy'].shape == (5,)
    assert np.allclose(got['entropy'].cpu().numpy(), entropy.numpy(), rtol=0, atol=1e-6) and consensus.tolist() == lowest


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    """S = 16385 (ABOPT_EUNSUPPORTED), negative max_mismatch / max_clusters, n = 0, a NULL and a misaligned workspace (ABOPT_EINVAL), a short one
    (ABOPT_EWORKSPACE) and G = 0 (a no-op) through the C entry points: the return codes, and every output keeps the pattern it was filled with."""
    from ab_opt_amd import hip
    L_ = hip.lib()
    G, S, n = 2, 65, 5
    xd = torch.from_numpy(case(1, 130, 5)).to(DEV)                   # 130 sequences: two groups of 65
    fill = lambda *shape: torch.full(shape, 77, dtype=torch.int32, device=DEV)
    label, centre, size, count, dist, counts = fill(G * S), fill(G * S), fill(G * S), fill(G), fill(G, S, S), fill(G, n, 21)
    need = L_.abopt_cluster_ws_bytes(G, S)
    ws = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)

    def call(G=G, S=S, n=n, m=1, cap=0, ws_ptr=hip.ptr(ws), ws_bytes=need):
        return L_.abopt_cluster_sequences_grouped(hip.ptr(xd), G, S, n, m, cap, ws_ptr, ws_bytes, hip.ptr(label), hip.ptr(centre), hip.ptr(size),
                                                  hip.ptr(count), hip.ptr(dist), hip.stream())
    assert call(G=1, S=16385) == 3 and '16385' in L_.abopt_last_error().decode()
    assert call(m=-1) == 1 and 'max_mismatch' in L_.abopt_last_error().decode()
    assert call(n=0) == 1 and call(S=0) == 1 and call(cap=-1) == 1 and call(G=-1) == 1
    assert call(ws_ptr=None) == 1 and 'NULL' in L_.abopt_last_error().decode()
    import ctypes
    assert call(ws_ptr=ctypes.c_void_p(ws.data_ptr() + 4)) == 1 and 'aligned' in L_.abopt_last_error().decode()
    assert call(ws_bytes=need - 1) == 4 and 'workspace too small' in L_.abopt_last_error().decode()
    assert call(G=0) == 0                                            # a no-op
    prof = lambda G=G, S=S, n=n, out=hip.ptr(counts): L_.abopt_sequence_profile_grouped(hip.ptr(xd), G, S, n, out, hip.stream())
    assert prof(S=0) == 1 and prof(n=0) == 1 and prof(G=-1) == 1 and prof(out=None) == 1 and prof(G=0) == 0
    torch.cuda.synchronize()
    for t in (label, centre, size, count, dist, counts):
        assert (t == 77).all()
    assert call() == 0 and prof() == 0                               # ... and the same buffers are filled by good calls
    torch.cuda.synchronize()
    assert (label != 77).all() and (count != 77).all() and (dist != 77).all() and (counts != 77).all()
    with pytest.raises(RuntimeError, match='abopt error 3'):
        hip.cluster_sequences_grouped(torch.zeros(16385, 1, dtype=torch.uint8, device=DEV), 16385, 1)
    empty = hip.cluster_sequences_grouped(torch.zeros(0, 7, dtype=torch.int64, device=DEV), 5, 1, want_dist=True)
    assert empty['label'].shape == (0,) and empty['count'].shape == (0,) and empty['centre'].shape == (0, 5) and empty['dist'].shape == (0, 5, 5)
    assert hip.sequence_profile_grouped(torch.zeros(0, 7, dtype=torch.int64, device=DEV), 5).shape == (0, 7, 21)


# ------------------------------------------------------------------------------------------ GPU: the screen
def _rep(t, n):
    return t.expand(n, *t.shape[1:]).contiguous()


def _stage2(design, one, pose_pos, pose_mask, S, dflag, seed, allowed=None):
    """Stage 2 of the screen with the public calls -> (seqs (P, S, n), ppl (P, S), design complexes of all P S designs: pos, mask, aa)."""
    from ab_opt_amd import geometry, hip, sampler
    P = pose_pos.shape[0]
    extra = {} if allowed is None else dict(aa_allowed=allowed.reshape(1, -1))
    cx = [dict(one, pos_heavyatom=pose_pos[i:i + 1], mask_heavyatom=pose_mask[i:i + 1], generate_flag=dflag[None], **extra) for i in range(P)]
    t2 = sampler.sample_grouped(design, cx, S, dict(sample_structure=False, sample_sequence=True, seed=screen.stage_seed(seed, 'design'), rng_offset=0))[0]
    g2 = _rep(dflag[None], P * S)
    aa2 = torch.where(g2, t2[2], _rep(one['aa'], P * S))
    des_pos, des_mask = geometry.reconstruct_backbone_partially(pose_pos.repeat_interleave(S, 0), hip.so3_exp(t2[0]), t2[1], aa2, _rep(one['chain_nb'], P * S),
                                                                _rep(one['res_nb'], P * S), pose_mask.repeat_interleave(S, 0), g2)
    return t2[2][:, dflag].view(P, S, -1), t2[4].to(DEV).view(P, S), des_pos, des_mask, aa2


def _redock(dock, one, npos, nmask, naa, D, seed):
    """D re-docks of each of the given design complexes in one launch (sample i D + j is re-dock j of complex i) -> (trajectory end, rebuilt pos, mask)."""
    from ab_opt_amd import geometry, hip, sampler
    n = npos.shape[0]
    gen = one['generate_flag'][0]
    cx = [dict(one, pos_heavyatom=npos[i:i + 1], mask_heavyatom=nmask[i:i + 1], aa=naa[i:i + 1], generate_flag=gen[None]) for i in range(n)]
    t3 = sampler.sample_grouped(dock, cx, D, dict(sample_structure=True, sample_sequence=False, seed=screen.stage_seed(seed, 'redock'), rng_offset=0))[0]
    g3 = _rep(gen[None], n * D)
    rpos, rmask = geometry.reconstruct_backbone_partially(npos.repeat_interleave(D, 0), hip.so3_exp(t3[0]), t3[1], torch.where(g3, t3[2], naa.repeat_interleave(D, 0)),
                                                          _rep(one['chain_nb'], n * D), _rep(one['res_nb'], n * D), nmask.repeat_interleave(D, 0), g3)
    return t3, rpos, rmask


def _per_design(one, t3, rpos, rmask, natives, D):
    """dockq / redock_score / prmsd rows: trajectory group u scored for every (u, native complex index i) of `natives` -> three lists in that order."""
    from ab_opt_amd import hip
    gen = one['generate_flag'][0]
    grp = screen.chain_groups(one['fragment_type'][0])
    dq, sc, pr = [], [], []
    for u, (npos, nmask) in natives:
        sl = slice(u * D, (u + 1) * D)
        dq.append(hip.dockq_lite(rpos[sl], rmask[sl], npos, nmask, grp, check=False))
        sc.append(hip.commonness_score(t3[1][sl][:, gen]))
        pr.append(t3[3].to(DEV)[sl])
    return torch.stack(dq), torch.stack(sc), torch.stack(pr)


def _screen_kw(**extra):
    kw = dict(screen_workers.SCREEN)
    kw.update(extra)
    return kw


@pytest.mark.gpu
def test_screen_without_the_new_options_is_unchanged(screen_models):
    """No seq_mismatch / share_redocks: none of the new keys, and every field of the composition of public calls the screen has always equalled
    (tests/test_screen.py: _composition) is torch.equal.  seq_mismatch alone adds fields and changes none."""
    from test_screen import _composition
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    kw = _screen_kw()
    P, S, k, D = kw['num_poses'], kw['designs_per_pose'], kw['screened_per_pose'], kw['redocks_per_design']
    plain = screen.optimize_antibody(dock, design, one, poses_per_launch=P, **kw)
    new = {'seq_label', 'seq_centre', 'seq_size', 'seq_clusters', 'seq_counts', 'design_unit', 'unit_owner', 'unit_size'}
    assert not (set(plain) & new)
    assert set(plain) == {'pose_ca', 'pose_score', 'seqs', 'aar', 'ppl', 'chosen', 'dockq', 'prmsd', 'redock_score', 'dockq_mean', 'dockq_std', 'prmsd_mean', 'prmsd_std'}
    want = _composition(dock, design, one, P, S, k, D, kw['contig'], kw['seed'])
    for name, v in want.items():
        assert plain[name].shape == v.shape and torch.equal(plain[name], v), name
    with_seq = screen.optimize_antibody(dock, design, one, poses_per_launch=P, seq_mismatch=2, **kw)
    assert set(with_seq) == set(plain) | {'seq_label', 'seq_centre', 'seq_size', 'seq_clusters', 'seq_counts'}
    for name, v in plain.items():
        assert torch.equal(with_seq[name], v), name


@pytest.mark.gpu
def test_seq_mismatch_fields_equal_the_public_calls_and_the_statement(screen_models):
    from ab_opt_amd import hip
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    kw = _screen_kw()
    P, S = kw['num_poses'], kw['designs_per_pose']
    for m in (0, workers.SEQ_MISMATCH, 7):
        res = screen.optimize_antibody(dock, design, one, poses_per_launch=2, seq_mismatch=m, **kw)
        seqs = res['seqs']
        n = seqs.shape[2]
        assert n == 7
        cl = hip.cluster_sequences_grouped(seqs.reshape(P * S, n), S, m)
        assert torch.equal(res['seq_label'], cl['label'].view(P, S).long()) and torch.equal(res['seq_centre'], cl['centre'].long())
        assert torch.equal(res['seq_size'], cl['size'].long()) and torch.equal(res['seq_clusters'], cl['count'].long())
        assert torch.equal(res['seq_counts'], hip.sequence_profile_grouped(seqs.reshape(P * S, n), S).long())
        assert all(res[name].dtype == torch.int64 for name in ('seq_label', 'seq_centre', 'seq_size', 'seq_clusters', 'seq_counts'))
        x = seqs.cpu().numpy()
        for q in range(P):
            wl, wc, ws = greedy(x[q], m)
            C = len(wc)
            assert res['seq_clusters'][q].item() == C and res['seq_label'][q].tolist() == wl.tolist()
            assert res['seq_centre'][q].tolist() == wc.tolist() + [-1] * (S - C) and res['seq_size'][q].tolist() == ws.tolist() + [0] * (S - C)
            assert np.array_equal(res['seq_counts'][q].cpu().numpy(), profile(x[q]))
    assert (res['seq_clusters'] == 1).all()                          # max_mismatch = n: one family per pose


def _diverse_composition(dock, design, one, kw, m):
    from test_pose_clusters import _stage1
    P, S, k, D, seed = kw['num_poses'], kw['designs_per_pose'], kw['screened_per_pose'], kw['redocks_per_design'], kw['seed']
    gen = one['generate_flag'][0]
    dflag = gen & generate_mask_from_str(kw['contig'], gen)
    pose_ca, pose_pos, pose_mask = _stage1(dock, one, P, seed)
    seqs, ppl, des_pos, des_mask, aa2 = _stage2(design, one, pose_pos, pose_mask, S, dflag, seed)
    x = seqs.cpu().numpy()
    chosen = torch.tensor([diverse_rule(x[q], m, k) for q in range(P)], device=DEV)
    rows = (torch.arange(P, device=DEV)[:, None] * S + chosen).reshape(-1)
    npos, nmask, naa = des_pos[rows], des_mask[rows], aa2[rows]
    t3, rpos, rmask = _redock(dock, one, npos, nmask, naa, D, seed)
    dq, sc, pr = _per_design(one, t3, rpos, rmask, [(i, (npos[i], nmask[i])) for i in range(P * k)], D)
    return dict(pose_ca=pose_ca, seqs=seqs, ppl=ppl, chosen=chosen, dockq=dq.view(P, k, D, 4), redock_score=sc.view(P, k, D), prmsd=pr.view(P, k, D))


@pytest.mark.gpu
def test_diverse_screen_equals_the_rule_and_the_composition(screen_models):
    """screen_by='diverse': `chosen` is the rule evaluated in numpy from the returned seqs -- at max_mismatch = n every pose has ONE family, so the second slot is
    filled with the lowest index not yet chosen --, and every downstream field equals the composition of public calls with that choice."""
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    for m in (workers.SEQ_MISMATCH, 7):
        kw = _screen_kw(screen_by='diverse')
        want = _diverse_composition(dock, design, one, kw, m)
        res = screen.optimize_antibody(dock, design, one, poses_per_launch=kw['num_poses'], seq_mismatch=m, **kw)
        x = res['seqs'].cpu().numpy()
        assert res['chosen'].tolist() == [diverse_rule(x[q], m, kw['screened_per_pose']) for q in range(kw['num_poses'])]
        for name, v in want.items():
            assert res[name].shape == v.shape and torch.equal(res[name], v), (m, name)
    assert all(row[0] == 0 and row[1] == 1 for row in res['chosen'].tolist())          # one family: its centre 0 (every count ties), then the fill


@pytest.mark.gpu
def test_redock_inputs_of_one_sequence_on_two_poses_are_identical(screen_models):
    """The premise of share_redocks.  The same designed sequence put on two different stage-1 poses gives two re-dock inputs that differ only in the
    coordinates of the docked residues -- which the re-dock regenerates and encode() hides: res_feat and pair_feat are torch.equal, and sample_grouped with the
    same seed and offset returns torch.equal trajectories (every step, every field)."""
    from test_pose_clusters import _stage1
    from ab_opt_amd import geometry, hip, sampler
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    kw = _screen_kw()
    seed, D = kw['seed'], kw['redocks_per_design']
    gen = one['generate_flag'][0]
    dflag = gen & generate_mask_from_str(kw['contig'], gen)
    pose_ca, pose_pos, pose_mask = _stage1(dock, one, 2, seed)
    assert not torch.equal(pose_pos[0], pose_pos[1])
    cx = [dict(one, pos_heavyatom=pose_pos[i:i + 1], mask_heavyatom=pose_mask[i:i + 1], generate_flag=dflag[None]) for i in range(2)]
    t2 = sampler.sample_grouped(design, cx, 1, dict(sample_structure=False, sample_sequence=True, seed=screen.stage_seed(seed, 'design'), rng_offset=0))[0]
    naa = _rep(torch.where(dflag, t2[2][0], one['aa'][0])[None], 2)                       # the design of pose 0, put on both poses
    assert not torch.equal(naa[0], one['aa'][0])
    npos, nmask = geometry.reconstruct_backbone_partially(pose_pos, hip.so3_exp(t2[0]), t2[1], naa, _rep(one['chain_nb'], 2), _rep(one['res_nb'], 2), pose_mask,
                                                          _rep(dflag[None], 2))           # as the screen rebuilds a chosen design
    assert not torch.equal(npos[0], npos[1])
    cx = [dict(one, pos_heavyatom=npos[i:i + 1], mask_heavyatom=nmask[i:i + 1], aa=naa[i:i + 1], generate_flag=gen[None]) for i in range(2)]
    with torch.no_grad():
        feats = [dock.encode(c, remove_structure=True, remove_sequence=False) for c in cx]
    assert torch.equal(feats[0][0], feats[1][0]), 'res_feat'
    assert torch.equal(feats[0][1], feats[1][1]), 'pair_feat'
    opt = dict(sample_structure=True, sample_sequence=False, seed=screen.stage_seed(seed, 'redock'), rng_offset=0)
    trajs = [sampler.sample_grouped(dock, [c], D, dict(opt)) for c in cx]
    steps = lambda tr: list(tr.items()) if isinstance(tr, dict) else list(enumerate(tr))
    assert len(steps(trajs[0])) == len(steps(trajs[1])) >= 2
    compared = 0
    for (ta, sa), (tb, sb) in zip(steps(trajs[0]), steps(trajs[1])):
        assert ta == tb and len(sa) == len(sb)
        for i, (x, y) in enumerate(zip(sa, sb)):
            if torch.is_tensor(x):
                assert torch.equal(x, y), (ta, i)
                compared += 1
    assert compared >= 3 * len(steps(trajs[0]))


def _shared_composition(dock, design, one, kw, allowed):
    from test_pose_clusters import _stage1
    P, S, k, D, seed = kw['num_poses'], kw['designs_per_pose'], kw['screened_per_pose'], kw['redocks_per_design'], kw['seed']
    gen = one['generate_flag'][0]
    dflag = gen & generate_mask_from_str(kw['contig'], gen)
    pose_ca, pose_pos, pose_mask = _stage1(dock, one, P, seed)
    seqs, ppl, des_pos, des_mask, aa2 = _stage2(design, one, pose_pos, pose_mask, S, dflag, seed, allowed)
    chosen = torch.sort(ppl, dim=1, stable=True)[1][:, :k]
    rows = (torch.arange(P, device=DEV)[:, None] * S + chosen).reshape(-1)
    npos, nmask, naa = des_pos[rows], des_mask[rows], aa2[rows]
    unit, owner, size = units_of(naa[:, dflag].cpu().numpy())
    own = torch.from_numpy(owner).to(DEV)
    t3, rpos, rmask = _redock(dock, one, npos[own], nmask[own], naa[own], D, seed)              # one launch: unit u is "pose" u with one design
    dq, sc, pr = _per_design(one, t3, rpos, rmask, [(int(unit[i]), (npos[i], nmask[i])) for i in range(P * k)], D)
    return dict(pose_ca=pose_ca, seqs=seqs, ppl=ppl, chosen=chosen, dockq=dq.view(P, k, D, 4), redock_score=sc.view(P, k, D), prmsd=pr.view(P, k, D),
                design_unit=torch.from_numpy(unit).to(DEV).view(P, k), unit_owner=own, unit_size=torch.from_numpy(size).to(DEV))


@pytest.mark.gpu
def test_shared_redocks_equal_the_composition(screen_models):
    """share_redocks under allowed_aa that leaves at most 8 distinct designs for P k = 10 chosen ones: units, owners and sizes are the statement's; every
    (pose, slot) carries its unit's prmsd / redock_score rows and its OWN DockQ (the unit's re-docks against the owner's design complex).  The unshared run of the
    same screen shows that the chosen designs are not all one sequence."""
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    kw = _screen_kw()
    P, k = kw['num_poses'], kw['screened_per_pose']
    allowed = workers.allowed(DEV)
    plain = screen.optimize_antibody(dock, design, one, poses_per_launch=P, allowed_aa=allowed, **kw)
    picked = torch.gather(plain['seqs'], 1, plain['chosen'][:, :, None].expand(-1, -1, plain['seqs'].shape[2])).reshape(P * k, -1)
    distinct = len({tuple(r) for r in picked.tolist()})
    assert 2 <= distinct <= 8, distinct                              # a condition on the inputs: duplicates exist by counting, and so do two different designs
    want = _shared_composition(dock, design, one, kw, allowed)
    res = screen.optimize_antibody(dock, design, one, poses_per_launch=P * k, allowed_aa=allowed, share_redocks=True, **kw)      # every unit in one launch, as the composition
    assert set(res) == set(plain) | {'design_unit', 'unit_owner', 'unit_size'}
    for name, v in want.items():
        assert res[name].shape == v.shape and res[name].dtype == v.dtype and torch.equal(res[name], v), name
    U = res['unit_owner'].shape[0]
    assert U == distinct and int(res['unit_size'].sum()) == P * k
    unit = res['design_unit'].reshape(-1)
    for name in ('prmsd', 'redock_score'):
        flat = res[name].reshape(P * k, -1)
        for u in range(U):
            members = torch.nonzero(unit == u).reshape(-1)
            assert members[0] == res['unit_owner'][u] and members.numel() == res['unit_size'][u]
            assert all(torch.equal(flat[i], flat[members[0]]) for i in members), (name, u)
    for name in ('seqs', 'ppl', 'chosen', 'aar', 'pose_ca', 'pose_score'):      # sharing changes nothing before stage 3
        assert torch.equal(res[name], plain[name]), name
    q = res['dockq'][..., 3]
    assert torch.equal(res['dockq_mean'], q.mean(-1)) and (q >= 0).all() and (q <= 1).all()
    # the optional per-unit fields (re-dock clusters, interface geometry, epitope) change nothing else and are the owner's rows on every member of a unit
    more = screen.optimize_antibody(dock, design, one, poses_per_launch=P * k, allowed_aa=allowed, share_redocks=True, redock_cutoff=2.0, clash_cutoff=3.0, **kw)
    extra = ('redock_cluster_frac', 'redock_clusters', 'redock_geom', 'epitope_freq', 'pose_geom')
    assert set(more) == set(res) | set(extra)
    for name, v in res.items():
        assert torch.equal(more[name], v), name
    D, L = kw['redocks_per_design'], one['aa'].shape[1]
    assert more['redock_geom'].shape == (P, k, D, 5) and more['epitope_freq'].shape == (P, k, L) and more['redock_clusters'].shape == (P, k)
    for name in extra[:4]:
        flat = more[name].reshape(P * k, -1)
        assert torch.equal(flat, flat[res['unit_owner']][unit]), name


@pytest.mark.gpu
def test_sequence_screens_do_not_depend_on_poses_per_launch_or_ranks(tmp_path, monkeypatch, screen_models):
    """The diverse screen and the shared screen with all, 1 and 2 poses (units) per launch, and on two gloo ranks sharing cuda:0, bit for bit --
    ABOPT_PAIR_TERMS=0 / ABOPT_CORE_NO_SPLIT=1 pin one arithmetic form, as in tests/test_screen.py."""
    harness.pin_denoiser_form(monkeypatch)
    P = screen_workers.SCREEN['num_poses']
    refs = {name: harness.screen_is_launch_size_invariant(screen_models, extra) for name, extra in workers.options(DEV).items()}
    assert 'unit_owner' in refs['shared'] and refs['shared']['unit_owner'].shape[0] < P * screen_workers.SCREEN['screened_per_pose']
    harness.two_ranks_return(workers.sequence_screen_worker, tmp_path, refs)
