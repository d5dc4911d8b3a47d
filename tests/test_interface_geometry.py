"""Interface geometry: abopt_interface_geometry_grouped / hip.interface_geometry_grouped / sampler.interface_geometry /
sampler.backbone_links and the screen's pose_geom, redock_geom, epitope_freq (screen.optimize_antibody(clash_cutoff=..., contact_cutoff=..., bond_max=...),
screen.screen_filter(max_clashes=..., min_contacts=...)).

The definition is restated below in numpy / float64 (`geometry_f64`).  Every result is an integer count, so the device call has to EQUAL the statement; fp32 and
float64 may disagree only on a distance that sits on a cutoff, so no test input has one: `case` builds the inputs and `cutoff_with_margin` moves each nominal
cutoff c into the widest gap between the float64 distances inside [0.9 c, 1.1 c] (atom-pair distances for the clash cutoff, residue-pair minima for the contact
cutoff, C-N distances of the links for bond_max); every use asserts that no distance lies within 1e-4 c of the cutoff actually used.  That is a condition on the
inputs, not a tolerance on the code: fp32's error on a distance of these magnitudes is below 1e-6 A (4 x 2^-24 relative, csrc/interface.hip)."""
import functools

import numpy as np
import pytest
import torch

import interface_geometry_workers
import scorer_harness as harness
import screen_workers
from ab_opt_amd import screen
from scorer_harness import DEV, dev, screen_models                 # noqa: F401 (screen_models: the fixture)

CLASH, CONTACT, BOND = 3.0, 5.0, 2.0                      # the conventional values the screen defaults to
COLS = ('clash', 'contacts', 'iface1', 'iface2', 'breaks')
GS = [(1, 1), (3, 2), (2, 5)]
LS = [2, 7, 63, 64, 65, 130]                              # lane-tile boundaries of the side-2 walk and the smallest sizes
AS = [1, 4, 15]


# ------------------------------------------------------------------------------------------ the float64 statement
def pair_tables_f64(pos, mask, group):
    """ONE candidate: pos (L, A, 3), mask (L, A), group (L,) -> (side-1 indices, side-2 indices, d [n1, n2, A, A] float64 distances of the atom pairs,
    valid [n1, n2, A, A]: both atoms masked in)."""
    pos = np.asarray(pos, dtype=np.float64)
    mask = np.asarray(mask).astype(bool)
    s1, s2 = np.nonzero(np.asarray(group) == 1)[0], np.nonzero(np.asarray(group) == 2)[0]
    diff = pos[s1][:, None, :, None, :] - pos[s2][None, :, None, :, :]
    with np.errstate(invalid='ignore'):
        d = np.sqrt((diff * diff).sum(-1))
    valid = mask[s1][:, None, :, None] & mask[s2][None, :, None, :]
    return s1, s2, d, valid


def geometry_f64(pos, mask, group, clash_d, contact_d, link=None, bond_max=None):
    """The definition (include/abopt.h: abopt_interface_geometry_grouped) for ONE candidate in float64 -> ([clash, contacts, iface1, iface2, breaks], hit [L] bool:
    the residue is in at least one contact).  Comparisons with a NaN distance are false."""
    pos = np.asarray(pos, dtype=np.float64)
    mask = np.asarray(mask).astype(bool)
    L = pos.shape[0]
    s1, s2, d, valid = pair_tables_f64(pos, mask, group)
    takes_part = np.ones((len(s1), len(s2)), dtype=bool)
    if link is not None:
        lk = np.asarray(link).astype(bool)
        a, b = s1[:, None], s2[None, :]
        takes_part = ~(((b == a + 1) & lk[np.minimum(a, L - 1)]) | ((a == b + 1) & lk[np.minimum(b, L - 1)]))
    with np.errstate(invalid='ignore'):
        clash = int((valid & (d < clash_d) & takes_part[:, :, None, None]).sum())
        contact = (valid & (d <= contact_d)).any((2, 3)) & takes_part          # min <= c  <=>  some pair <= c; a residue without atoms has no valid pair
    hit = np.zeros(L, dtype=bool)
    hit[s1[contact.any(1)]] = True
    hit[s2[contact.any(0)]] = True
    breaks = 0
    if link is not None and bond_max is not None:
        for r in range(L - 1):
            if lk[r] and mask[r, 2] and mask[r + 1, 0]:
                with np.errstate(invalid='ignore'):
                    breaks += not (np.sqrt(((pos[r, 2] - pos[r + 1, 0]) ** 2).sum()) <= bond_max)
    return [clash, int(contact.sum()), int(contact.any(1).sum()), int(contact.any(0).sum()), int(breaks)], hit


def statement(pos, mask, group, S, clash_d, contact_d, link=None, bond_max=None):
    """geometry_f64 over G groups of S candidates: pos (G*S, L, A, 3), mask (G*S, L, A) or (G, L, A), group / link (G, L) -> (out [G*S, 5], freq [G, L])."""
    N, G = pos.shape[0], group.shape[0]
    out, freq = np.zeros((N, 5), dtype=np.int64), np.zeros(group.shape, dtype=np.int64)
    for c in range(N):
        g = c // S
        m = mask[c] if mask.shape[0] == N else mask[g]
        out[c], hit = geometry_f64(pos[c], m, group[g], clash_d, contact_d, None if link is None else link[g], bond_max)
        freq[g] += hit
    return out, freq


def geometry_torch(pos, mask, group, clash_d, contact_d):
    """The plain torch statement on the device (one cdist per candidate over all L A atoms, fp32): what the kernel is compared with in DESIGN.md section 6.3.  No
    links, no breaks.  pos (N, L, A, 3), mask (N, L, A), group (L,) -> (N, 4) int64: clash, contacts, iface1, iface2."""
    N, L, A, _ = pos.shape
    g = group.repeat_interleave(A)
    cross = (g[:, None] == 1) & (g[None, :] == 2)
    out = []
    for c in range(N):
        x = pos[c].reshape(L * A, 3)
        m = mask[c].reshape(L * A)
        d = torch.cdist(x, x, compute_mode='donot_use_mm_for_euclid_dist')
        ok = cross & m[:, None] & m[None, :]
        clash = (ok & (d < clash_d)).sum()
        contact = (ok & (d <= contact_d)).view(L, A, L, A).any(3).any(1)
        out.append(torch.stack([clash, contact.sum(), contact.any(1).sum(), contact.any(0).sum()]))
    return torch.stack(out)


# ------------------------------------------------------------------------------------------ the inputs
def cutoff_with_margin(dist, c):
    """The midpoint of the widest gap between consecutive sorted values of `dist` inside [0.9 c, 1.1 c] (the window's ends close the first and the last gap)
    -> (cutoff, distance of the nearest value to it)."""
    r = np.sort(np.asarray(dist, dtype=np.float64).reshape(-1))
    r = r[np.isfinite(r)]
    pts = np.concatenate([[0.9 * c], r[(r > 0.9 * c) & (r < 1.1 * c)], [1.1 * c]])
    i = int(np.argmax(np.diff(pts)))
    cut = 0.5 * (pts[i] + pts[i + 1])
    return cut, (np.abs(r - cut).min() if r.size else np.inf)


def distances_f64(pos, mask, group, link, S):
    """Every float64 distance a cutoff is compared with, over all candidates (pairs that a link would skip included: the superset serves the runs with and
    without link) -> (atom-pair distances, residue-pair minima, C-N distances of the links)."""
    N, L, A = mask.shape
    atom, res, bond = [], [], []
    for c in range(N):
        g = c // S
        _, _, d, valid = pair_tables_f64(pos[c], mask[c], group[g])
        atom.append(d[valid])
        res.append(np.where(valid, d, np.inf).min((2, 3), initial=np.inf).reshape(-1))
        if A >= 3:
            p = pos[c].astype(np.float64)
            ok = link[g][:-1] & mask[c][:-1, 2] & mask[c][1:, 0]
            bond.append(np.sqrt(((p[:-1, 2] - p[1:, 0]) ** 2).sum(-1))[ok])
    cat = lambda v: np.concatenate(v) if v else np.zeros(0)
    return cat(atom), cat(res), cat(bond)


def placed_cutoffs(pos, mask, group, link, S, nominal):
    """{name: (cutoff, margin)} for nominal = {'clash': c, 'contact': c, 'bond': c}; a name with a suffix ('contact_wide') places another cutoff of its kind."""
    atom, res, bond = distances_f64(pos, mask, group, link, S)
    return {name: cutoff_with_margin(dict(clash=atom, contact=res, bond=bond)[name.split('_')[0]], c) for name, c in nominal.items()}


def _raw(G, S, L, A, seed):
    """Two CA random walks of 3.8 A steps per candidate, origins 6 A apart; atoms normal(1.2 A) around their CA; atoms 0-3 always masked in, the rest with
    probability 0.7.  A third of the residues are side 1, the first walk; in odd groups two residues of each walk change sides (the compacted lists are no
    index ranges, and links join residues of different sides).  From L = 7 on one residue has no atoms at all and two residues have group 0.  Links: every residue to the next but
    ~10 %; with A >= 3 the first two links of every candidate get C-N distances of 1.33 A and 3.5 A by hand."""
    rng = np.random.default_rng(seed)
    N, n1 = G * S, max(1, L // 3)
    group = np.full((G, L), 2, dtype=np.int32)
    for g in range(G):
        group[g, :n1] = 1
        if g % 2 and L >= 7:                                         # two residues of each walk change sides
            group[g, rng.permutation(n1)[:2]] = 2
            group[g, n1 + rng.permutation(L - n1)[:2]] = 1
        if L >= 7:
            group[g, rng.permutation(L)[:2]] = 0
    link = rng.random((G, L)) < 0.9
    link[:, :2] = True
    pos = np.zeros((N, L, A, 3))
    mask = rng.random((N, L, A)) < 0.7
    mask[:, :, :4] = True
    for c in range(N):
        first = np.arange(L) < n1
        step = rng.normal(size=(L, 3))
        step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
        ca = np.zeros((L, 3))
        for sel, origin in ((first, np.zeros(3)), (~first, np.array([6.0, 0.0, 0.0]))):
            ca[sel] = origin + np.cumsum(step[sel], 0)
        pos[c] = ca[:, None] + rng.normal(size=(L, A, 3)) * 1.2
        if L >= 7:
            mask[c, 3 + rng.integers(L - 3)] = False                    # not one of the residues whose links are set by hand below
        if A >= 3:
            for r, dist in ((0, 1.33), (1, 3.5)):
                if r + 1 < L:
                    u = rng.normal(size=3)
                    pos[c, r + 1, 0] = pos[c, r, 2] + dist * u / np.linalg.norm(u)
    return pos.astype(np.float32), mask, group, link


@functools.lru_cache(maxsize=None)
def case(G, S, L, A):
    """Inputs with a margin, built once per shape and shared by the tests -> dict(pos [G*S, L, A, 3] fp32, mask [G*S, L, A] bool, group [G, L] int32,
    link [G, L] bool, clash / contact / bond: the cutoffs used, out / freq: the float64 statement without link, out_link / freq_link: with link and bond).
    The seed is the first whose inputs leave every cutoff a margin of more than 1e-4 c and, from L = 48 on, give at least one clash and one contact."""
    nominal = dict(clash=CLASH, contact=CONTACT, bond=BOND)
    for seed in range(200):
        pos, mask, group, link = _raw(G, S, L, A, 1000 * seed + 31 * L + 7 * A + 3 * G + S)
        cuts = placed_cutoffs(pos, mask, group, link, S, nominal)
        if not all(m > 1e-4 * nominal[k] for k, (_, m) in cuts.items()):
            continue
        cl, ct, bd = (cuts[k][0] for k in ('clash', 'contact', 'bond'))
        out, freq = statement(pos, mask, group, S, cl, ct)
        if L < 48 or (out[:, 0].sum() > 0 and out[:, 1].sum() > 0):
            break
    for k, (cut, margin) in cuts.items():
        assert margin > 1e-4 * nominal[k] and 0.9 * nominal[k] <= cut <= 1.1 * nominal[k], (G, S, L, A, k, cut, margin)   # a condition on the inputs, not on the code
    assert L < 48 or (out[:, 0].sum() > 0 and out[:, 1].sum() > 0), (G, S, L, A)
    res = dict(pos=pos, mask=mask, group=group, link=link, clash=cl, contact=ct, bond=bd, out=out, freq=freq)
    if A >= 3:
        res['out_link'], res['freq_link'] = statement(pos, mask, group, S, cl, ct, link, bd)
    return res


def _stack(res):
    return torch.stack([res[k] for k in COLS], 1).cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------------------------------ CPU
def test_statement_on_a_hand_worked_example():
    """Six one-atom residues on a line, clash cutoff 2.5 and contact cutoff 4.25, x = 0, 2 (side 1), 4.5, 7, 4.25 (side 2), 2 (group 0, on top of residue 1):
      (0, 2) 4.5 nothing   (0, 3) 7 nothing   (0, 4) 4.25 contact: <= holds with equality
      (1, 2) 2.5 contact, NOT a clash: < is strict   (1, 3) 5 nothing   (1, 4) 2.25 clash and contact
    -> clash 1, contacts 3, iface1 2, iface2 2 (residues 2, 4).  With link[1] the pair (1, 2) is skipped exactly: contacts 2, iface2 1, and residue 2 is in no
    contact any more.  link[4] joins residue 4 to residue 5 (group 0): it skips nothing.  Then three N-CA-C residues on a line for the breaks."""
    x = np.zeros((6, 1, 3))
    x[:, 0, 0] = [0.0, 2.0, 4.5, 7.0, 4.25, 2.0]
    mask = np.ones((6, 1), dtype=bool)
    group = np.array([1, 1, 2, 2, 2, 0])
    out, hit = geometry_f64(x, mask, group, 2.5, 4.25)
    assert out == [1, 3, 2, 2, 0] and hit.tolist() == [True, True, True, False, True, False]
    out, hit = geometry_f64(x, mask, group, 2.5, 4.25, link=np.array([0, 1, 0, 0, 1, 0]))
    assert out == [1, 2, 2, 1, 0] and hit.tolist() == [True, True, False, False, True, False]
    out, hit = geometry_f64(x, mask, np.array([2, 2, 1, 1, 1, 0]), 2.5, 4.25, link=np.array([0, 1, 0, 0, 1, 0]))     # the sides swapped: a == b + 1 with link[b]
    assert out == [1, 2, 1, 2, 0] and hit.tolist() == [True, True, False, False, True, False]
    masked = mask.copy()
    masked[4] = False                                               # residue 4 without atoms contacts nobody
    assert geometry_f64(x, masked, group, 2.5, 4.25)[0] == [0, 1, 1, 1, 0]
    nan = x.copy()
    nan[4, 0, 1] = np.nan                                           # ... and so does a NaN coordinate
    assert geometry_f64(nan, mask, group, 2.5, 4.25)[0] == [0, 1, 1, 1, 0]
    # breaks: N, CA, C at 3.8 r + (0, 1.4, 2.5), residue 2 moved 2 A on: C0-N1 = 1.3 (bonded), C1-N2 = 3.3 (a break at bond_max 2)
    bb = np.zeros((3, 3, 3))
    bb[:, :, 0] = 3.8 * np.arange(3)[:, None] + np.array([0.0, 1.4, 2.5])
    bb[2, :, 0] += 2.0
    m3, g3, lk = np.ones((3, 3), dtype=bool), np.array([1, 1, 2]), np.array([1, 1, 1])
    assert geometry_f64(bb, m3, g3, 0.5, 0.5, lk, 2.0)[0][4] == 1
    assert geometry_f64(bb, m3, g3, 0.5, 0.5, lk, 4.0)[0][4] == 0
    assert geometry_f64(bb, m3, g3, 0.5, 0.5, lk, None)[0][4] == 0 and geometry_f64(bb, m3, g3, 0.5, 0.5, None, 2.0)[0][4] == 0
    gone = m3.copy()
    gone[2, 0] = False                                              # a link with a missing atom is not counted
    assert geometry_f64(bb, gone, g3, 0.5, 0.5, lk, 2.0)[0][4] == 0
    bad = bb.copy()
    bad[1, 2, 2] = np.nan                                           # a NaN coordinate breaks its link
    assert geometry_f64(bad, m3, g3, 0.5, 0.5, lk, 4.0)[0][4] == 1


def test_backbone_links():
    """chain_nb[r] == chain_nb[r + 1] and res_nb[r + 1] == res_nb[r] + 1; a chain change, a numbering gap, an insertion-like repeat and the last residue give False."""
    from ab_opt_amd import sampler
    chain = torch.tensor([[0, 0, 0, 1, 1, 1, 1]])
    resnb = torch.tensor([[5, 6, 7, 8, 9, 11, 11]])
    got = sampler.backbone_links(chain, resnb)
    assert got.dtype == torch.bool and got.shape == (1, 7) and not got.is_cuda
    assert got.tolist() == [[True, True, False, True, False, False, False]]
    assert sampler.backbone_links(chain[0], resnb[0]).tolist() == got[0].tolist()
    assert sampler.backbone_links(torch.tensor([3]), torch.tensor([1])).tolist() == [False]


def test_cutoffs_are_validated_without_a_device():
    """hip.check_distance_cutoff, hip.interface_geometry_grouped, sampler.interface_geometry and optimize_antibody refuse negative / non-finite cutoffs and
    malformed shapes with ValueError before anything touches a device: the tensors here live on the CPU and the models are None."""
    from ab_opt_amd import hip, sampler
    from ab_opt_amd.utils import synth
    assert hip.check_distance_cutoff('x', 3) == 3.0 and hip.check_distance_cutoff('x', 0) == 0.0
    pos, mask, group = torch.zeros(4, 6, 4, 3), torch.ones(4, 6, 4, dtype=torch.bool), torch.ones(2, 6, dtype=torch.int32)
    for bad in (-1.0, float('nan'), float('inf'), -0.5):
        with pytest.raises(ValueError, match='finite and >= 0'):
            hip.check_distance_cutoff('x', bad)
        for name in ('clash_cutoff', 'contact_cutoff', 'bond_max'):
            with pytest.raises(ValueError, match=name):
                hip.interface_geometry_grouped(pos, mask, group, **{name: bad})
    with pytest.raises(ValueError, match='whole groups'):
        hip.interface_geometry_grouped(pos[:3], mask[:3], group)
    with pytest.raises(ValueError, match='neither per candidate nor per group'):
        hip.interface_geometry_grouped(pos, mask[:3], group)
    with pytest.raises(ValueError, match='1 .. 15'):
        hip.interface_geometry_grouped(torch.zeros(4, 6, 16, 3), torch.ones(4, 6, 16, dtype=torch.bool), group)
    for wrong in (mask[0], torch.tensor(True), mask[None]):             # a mask of another rank
        with pytest.raises(ValueError, match='expected pos'):
            hip.interface_geometry_grouped(pos, wrong, group)
    with pytest.raises(ValueError, match='A >= 3'):
        hip.interface_geometry_grouped(pos[:, :, :2], mask[:, :, :2], group, link=torch.ones(2, 6, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='HIP device only'):          # valid arguments reach the binding, which has no CPU path
        hip.interface_geometry_grouped(pos, mask, group)
    batch = dict(fragment_type=torch.ones(2, 6, dtype=torch.int64), generate_flag=torch.zeros(2, 6, dtype=torch.bool), chain_nb=torch.zeros(2, 6, dtype=torch.int64),
                 res_nb=torch.arange(6).expand(2, 6))
    with pytest.raises(ValueError, match='groups'):
        sampler.interface_geometry(batch, pos, mask, groups='sides')
    with pytest.raises(ValueError, match='clash_cutoff'):
        sampler.interface_geometry(batch, pos, mask, groups='generated', clash_cutoff=-1.0)
    one = synth.make_batch(1, synth.LAYOUT_128, seed=21)
    for name in ('clash_cutoff', 'contact_cutoff', 'bond_max'):
        for bad in (-1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError, match=name):
                screen.optimize_antibody(None, None, one, 4, 2, 2, **{name: bad})


def test_screen_filter_thresholds():
    """screen_filter on a hand-made result: with None / None it returns what the median rule alone returns on the same dict (computed here as in
    tests/test_screen.py); with thresholds it additionally asks the MEDIAN over the D re-docks: clash <= max_clashes, contacts >= min_contacts."""
    flat = torch.zeros(3, 2)                                         # every design sits on every median: the median rule keeps all
    geom = torch.zeros(3, 2, 3, 5, dtype=torch.int64)
    geom[..., 0] = torch.tensor([[[0, 9, 1], [4, 5, 6]], [[2, 2, 2], [0, 0, 50]], [[3, 1, 2], [7, 7, 0]]])        # clash medians  1 5 | 2 0 | 2 7
    geom[..., 1] = torch.tensor([[[10, 0, 12], [3, 3, 3]], [[0, 8, 9], [20, 1, 30]], [[5, 6, 4], [0, 0, 9]]])     # contact medians 10 3 | 8 20 | 5 0
    res = dict(dockq_std=flat, prmsd_std=flat.clone(), prmsd_mean=flat.clone(), redock_geom=geom)
    assert screen.screen_filter(res).all() and screen.screen_filter(res, None, None).all()
    assert screen.screen_filter(res, max_clashes=2).tolist() == [[True, False], [True, True], [True, False]]
    assert screen.screen_filter(res, min_contacts=5).tolist() == [[True, False], [True, True], [True, False]]
    assert screen.screen_filter(res, max_clashes=1, min_contacts=8).tolist() == [[True, False], [False, True], [False, False]]
    g = torch.Generator().manual_seed(3)
    rnd = {k: torch.rand(7, 2, generator=g) for k in ('dockq_std', 'prmsd_std', 'prmsd_mean')}
    want = torch.ones(7, 2, dtype=torch.bool)
    for t in rnd.values():
        want &= t.double() <= np.quantile(t.flatten().numpy().astype(np.float64), 0.5)
    assert torch.equal(screen.screen_filter(rnd), want) and torch.equal(screen.screen_filter(rnd, None, None), want)
    rnd['redock_geom'] = torch.zeros(7, 2, 4, 5, dtype=torch.int64)
    assert torch.equal(screen.screen_filter(rnd, max_clashes=0, min_contacts=0), want)
    assert not screen.screen_filter(rnd, min_contacts=1).any()
    with pytest.raises(ValueError, match='redock_geom'):
        screen.screen_filter(dict(dockq_std=flat, prmsd_std=flat, prmsd_mean=flat), max_clashes=3)


# ------------------------------------------------------------------------------------------ GPU: the kernels
def _assert_equals_statement(got, want_out, want_freq, tag):
    out = _stack(got)
    assert all(got[k].dtype == torch.int32 and got[k].is_cuda for k in COLS), tag
    assert np.array_equal(out, want_out), (tag, out.tolist(), want_out.tolist())
    if want_freq is not None:
        assert got['freq'].dtype == torch.int32 and np.array_equal(got['freq'].cpu().numpy(), want_freq), tag


@pytest.mark.gpu
@pytest.mark.parametrize('A', AS)
@pytest.mark.parametrize('L', LS)
@pytest.mark.parametrize('G,S', GS)
def test_counts_equal_the_float64_statement(G, S, L, A):
    """clash, contacts, iface1, iface2, breaks and freq of the device call are exactly those of the numpy / float64 statement, without link and (A >= 3) with
    link and bond_max: links join residues of different sides in the odd groups, so pairs are skipped, and the first two links of every candidate have C-N
    distances of 1.33 A and 3.5 A set by hand (one break each at least).  bond_max=None with link: the same counts, breaks 0."""
    from ab_opt_amd import hip
    c = case(G, S, L, A)
    pos, mask, group, link = dev(c, 'pos', 'mask', 'group', 'link')
    got = hip.interface_geometry_grouped(pos, mask, group, c['clash'], c['contact'], want_freq=True)
    print(f'(G, S, L, A) = {(G, S, L, A)}: clash {c["out"][:, 0].tolist()} contacts {c["out"][:, 1].tolist()}')
    _assert_equals_statement(got, c['out'], c['freq'], (G, S, L, A, 'no link'))
    plain = hip.interface_geometry_grouped(pos, mask, group, c['clash'], c['contact'])
    assert 'freq' not in plain and np.array_equal(_stack(plain), c['out'])
    if A >= 3:
        got = hip.interface_geometry_grouped(pos, mask, group, c['clash'], c['contact'], link=link, bond_max=c['bond'], want_freq=True)
        _assert_equals_statement(got, c['out_link'], c['freq_link'], (G, S, L, A, 'link'))
        if L >= 3:
            assert (c['out_link'][:, 4] >= 1).all(), 'the 3.5 A link is a break'
        if L >= 48 and G > 1:
            assert (c['out_link'][S:2 * S, 1] < c['out'][S:2 * S, 1]).all(), 'group 1 interleaves the sides: links skip contacts there'
        nobond = hip.interface_geometry_grouped(pos, mask, group, c['clash'], c['contact'], link=link)
        want = c['out_link'].copy()
        want[:, 4] = 0
        assert np.array_equal(_stack(nobond), want)


@pytest.mark.gpu
def test_torch_statement_equals_the_float64_statement():
    """geometry_torch (the cdist statement the kernel's time is compared with in DESIGN.md section 6.3) gives the same four counts on a case with a margin."""
    G, S, L, A = 1, 1, 65, 15
    c = case(G, S, L, A)
    pos, mask, group = dev(c, 'pos', 'mask', 'group')
    got = geometry_torch(pos, mask, group[0], c['clash'], c['contact'])
    assert np.array_equal(got.cpu().numpy(), c['out'][:, :4])


FAR = (900.0, -700.0, 500.0)
FARTHEST = (9900.0, -9900.0, 9900.0)                      # coordinates just under the 1e4 A the prune's slack is documented for (ulp 9.8e-4 A)


def far_case(G, S, L, A, shift):
    """case(G, S, L, A) rotated about a fixed axis and translated by `shift`, rounded to fp32 again; the cutoffs (nominal 3 / 5 / 2 A and a contact cutoff of
    12 A) are placed anew in the gaps of the MOVED fp32 inputs and the margin is asserted on them."""
    c = case(G, S, L, A)
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(1.1) * K + (1 - np.cos(1.1)) * K @ K
    pos = (c['pos'].astype(np.float64) @ R.T + np.array(shift)).astype(np.float32)
    nominal = dict(clash=CLASH, contact=CONTACT, bond=BOND, contact_wide=12.0)
    cuts = placed_cutoffs(pos, c['mask'], c['group'], c['link'], S, nominal)
    for k, (cut, margin) in cuts.items():
        assert margin > 1e-4 * nominal[k], (G, S, L, A, k, cut, margin)               # a condition on the inputs (ulp of a coordinate at 900 A: 6e-5 A)
    return dict(c, pos=pos, clash=cuts['clash'][0], contact=cuts['contact'][0], bond=cuts['bond'][0], wide=cuts['contact_wide'][0])


def _far_check(G, S, L, A, shift):
    from ab_opt_amd import hip
    c = far_case(G, S, L, A, shift)
    pos, mask, group, link = dev(c, 'pos', 'mask', 'group', 'link')
    lk = dict(link=link, bond_max=c['bond']) if A >= 3 else {}
    lk64 = dict(link=c['link'], bond_max=c['bond']) if A >= 3 else {}
    want, wfreq = statement(c['pos'], c['mask'], c['group'], S, c['clash'], c['contact'], **lk64)
    _assert_equals_statement(hip.interface_geometry_grouped(pos, mask, group, c['clash'], c['contact'], want_freq=True, **lk), want, wfreq, (G, S, L, A, 'far'))
    want, wfreq = statement(c['pos'], c['mask'], c['group'], S, 0.0, c['wide'], **lk64)
    assert (want[:, 0] == 0).all() and (L < 63 or want[:, 1].sum() > case(G, S, L, A)['out'][:, 1].sum())
    _assert_equals_statement(hip.interface_geometry_grouped(pos, mask, group, 0.0, c['wide'], want_freq=True, **lk), want, wfreq, (G, S, L, A, 'wide'))


@pytest.mark.gpu
@pytest.mark.parametrize('A', AS)
@pytest.mark.parametrize('L', LS)
@pytest.mark.parametrize('G,S', GS)
def test_far_from_the_origin_and_large_cutoffs(G, S, L, A):
    """The inputs of test_counts_equal_the_float64_statement rotated and translated by (900, -700, 500) A: the counts still equal the float64 statement on the
    moved fp32 inputs (the prune's slack has to cover the centres' arithmetic out there).  Then a contact cutoff of 12 A with a clash cutoff of 0: nearly every
    residue pair survives the prune, and no pair clashes (d < 0 never holds)."""
    _far_check(G, S, L, A, FAR)


@pytest.mark.gpu
def test_at_the_documented_coordinate_limit():
    """The same at (9900, -9900, 9900) A, just under the 1e4 A the prune's slack is derived for: one ulp of a coordinate is 9.8e-4 A there."""
    _far_check(3, 2, 65, 15, FARTHEST)
    _far_check(2, 5, 130, 4, FARTHEST)


@pytest.mark.gpu
def test_many_candidates_run_whole_tiles_per_workgroup():
    """Few candidates are split into so many slices that a workgroup owns one or two side-1 residues; the screen's large shapes run ONE slice per candidate: several
    side-1 tiles of 16 per workgroup, four residues per wave.  Here the ten candidates of case(2, 5, 130, 15) are repeated into G = 8 groups of S >= 128
    (S such that the call takes one slice on this device: N >= 4 x CUs) -- 43 side-1 residues, three tiles -- and again with the sides swapped: 83 or more side-1
    residues, six tiles, one side-2 tile.  Swapping the sides swaps iface1 and iface2 and changes nothing else; freq is the sum of the repeated candidates' marks."""
    from ab_opt_amd import hip
    c = case(2, 5, 130, 15)
    G = 8
    S = max(128, -(-4 * hip.device_info()['cu_count'] // G))
    assert min((c['group'][g] == 1).sum() for g in range(2)) > 32 and min((c['group'][g] == 2).sum() for g in range(2)) > 80
    hits = np.stack([geometry_f64(c['pos'][i], c['mask'][i], c['group'][i // 5], c['clash'], c['contact'], c['link'][i // 5], c['bond'])[1] for i in range(10)])
    pick = np.array([(g % 2) * 5 + s % 5 for g in range(G) for s in range(S)])                  # group g repeats the candidates of base group g % 2
    rows = [g % 2 for g in range(G)]
    pos, mask = torch.from_numpy(c['pos'][pick]).to(DEV), torch.from_numpy(c['mask'][pick]).to(DEV)
    group, link = torch.from_numpy(c['group'][rows]).to(DEV), torch.from_numpy(c['link'][rows]).to(DEV)
    want = c['out_link'][pick]
    wfreq = hits[pick].reshape(G, S, -1).sum(1)
    kw = dict(clash_cutoff=c['clash'], contact_cutoff=c['contact'], link=link, bond_max=c['bond'], want_freq=True)
    _assert_equals_statement(hip.interface_geometry_grouped(pos, mask, group, **kw), want, wfreq, 'one slice')
    swapped = torch.where(group == 1, 2, torch.where(group == 2, 1, group))
    _assert_equals_statement(hip.interface_geometry_grouped(pos, mask, swapped, **kw), want[:, [0, 1, 3, 2, 4]], wfreq, 'sides swapped')


@pytest.mark.gpu
def test_more_than_2_24_candidates():
    """G S = 65535 x 257 > 2^24 candidates of two one-atom residues 1 A apart (the candidates no longer fit one grid dimension of 256-thread workgroups): every
    candidate has one clash, one contact and one interface residue per side, every group's freq is S, S."""
    from ab_opt_amd import hip
    G, S = 65535, 257
    N = G * S
    assert N > 2 ** 24
    pos = torch.zeros(N, 2, 1, 3, device=DEV)
    pos[:, 1, 0, 0] = 1.0
    mask = torch.ones(1, 2, 1, dtype=torch.bool, device=DEV).expand(G, 2, 1).contiguous()
    group = torch.tensor([[1, 2]], dtype=torch.int32, device=DEV).expand(G, 2).contiguous()
    got = hip.interface_geometry_grouped(pos, mask, group, 3.0, 5.0, want_freq=True)
    for k, v in zip(COLS, (1, 1, 1, 1, 0)):
        assert got[k].shape == (N,) and bool((got[k] == v).all()), k
    assert bool((got['freq'] == S).all())


@pytest.mark.gpu
def test_degenerate_inputs():
    """One side empty: all zeros.  Every atom masked out: all zeros.  A NaN coordinate never clashes or contacts and breaks its link (the statement says the same,
    and the residue's other pairs are unchanged).  bond_max=None: breaks 0.  S = 0 and G = 0: empty results, freq zeros."""
    from ab_opt_amd import hip
    G, S, L, A = 2, 5, 65, 15
    c = case(G, S, L, A)
    pos, mask, group, link = dev(c, 'pos', 'mask', 'group', 'link')
    kw = dict(clash_cutoff=c['clash'], contact_cutoff=c['contact'], link=link, bond_max=c['bond'], want_freq=True)
    for side in (1, 2):
        empty = torch.where(group == side, 0, group)
        got = hip.interface_geometry_grouped(pos, mask, empty, **kw)
        assert (_stack(got)[:, :4] == 0).all() and (got['freq'] == 0).all(), side
        assert np.array_equal(_stack(got)[:, 4], c['out_link'][:, 4]), side                      # the breaks do not look at the sides
    got = hip.interface_geometry_grouped(pos, torch.zeros_like(mask), group, **kw)
    assert (_stack(got) == 0).all() and (got['freq'] == 0).all()
    bad = c['pos'].copy()
    hit = [r for r in np.nonzero(c['group'][0] == 1)[0] if c['freq_link'][0][r] > 0 and c['link'][0][r] and 3 <= r < L - 1]
    r = int(hit[0])                                                                              # a side-1 residue of group 0 in a contact, linked to r + 1
    bad[:, r, :, 1] = np.nan                                                                      # every atom of residue r, in every candidate
    for bond in (c['bond'], 1e3):                                                                 # 1e3 A: only links that touch a NaN are breaks
        want, wfreq = statement(bad, c['mask'], c['group'], S, c['clash'], c['contact'], c['link'], bond)
        got = hip.interface_geometry_grouped(torch.from_numpy(bad).to(DEV), mask, group, **dict(kw, bond_max=bond))
        _assert_equals_statement(got, want, wfreq, ('nan', bond))
    assert (wfreq[:, r] == 0).all() and (want[:, 1] <= c['out_link'][:, 1]).all()
    linked = c['mask'][:S, r, 2] & c['mask'][:S, r + 1, 0]
    assert linked.any() and (want[:S, 4] >= linked).all()                                         # the C of r is not a number: its link is broken
    got = hip.interface_geometry_grouped(pos, mask, group, c['clash'], c['contact'], link=link, bond_max=None)
    assert (got['breaks'] == 0).all()
    for g_, n in ((2, 0), (0, 0)):
        got = hip.interface_geometry_grouped(pos[:n], mask[:n], group[:g_], link=link[:g_], bond_max=2.0, want_freq=True)
        assert all(got[k].shape == (0,) for k in COLS) and got['freq'].shape == (g_, L) and (got['freq'] == 0).all()


@pytest.mark.gpu
def test_grouped_call_equals_per_group_calls():
    """G groups in one call against G single-group calls: torch.equal on the five counts and on freq."""
    from ab_opt_amd import hip
    for G, S in ((3, 2), (2, 5)):
        for L, A in ((7, 4), (65, 15), (130, 15)):
            c = case(G, S, L, A)
            kw = dict(clash_cutoff=c['clash'], contact_cutoff=c['contact'], bond_max=c['bond'], want_freq=True)
            inputs = dict(zip(('pos', 'mask', 'group', 'link'), dev(c, 'pos', 'mask', 'group', 'link')))
            harness.grouped_equals_per_group(lambda **t: hip.interface_geometry_grouped(**t, **kw), [((G, S, L, A), G, S, inputs)], {'group', 'link', 'freq'})


@pytest.mark.gpu
def test_shared_mask_equals_expanded_mask():
    """mask (G, L, A) shared by the S candidates of a group against the same mask repeated per candidate: torch.equal; and the float64 statement."""
    from ab_opt_amd import hip
    for G, S, L, A in ((3, 2, 65, 15), (2, 5, 63, 4)):
        c = case(G, S, L, A)
        pos, mask, group, link = dev(c, 'pos', 'mask', 'group', 'link')
        shared = mask[::S].contiguous()                                                         # the first candidate's mask of every group
        # another mask compares other atom pairs: the cutoffs are placed anew in the gaps of what this call compares, and the margin asserted on it
        exp = np.repeat(c['mask'][::S], S, 0)
        nominal = dict(clash=CLASH, contact=CONTACT, bond=BOND)
        cuts = placed_cutoffs(c['pos'], exp, c['group'], c['link'], S, nominal)
        assert all(m > 1e-4 * nominal[k] for k, (_, m) in cuts.items()), cuts
        c = dict(c, **{k: v[0] for k, v in cuts.items()})
        kw = dict(clash_cutoff=c['clash'], contact_cutoff=c['contact'], link=link, bond_max=c['bond'], want_freq=True)
        a = hip.interface_geometry_grouped(pos, shared, group, **kw)
        b = hip.interface_geometry_grouped(pos, shared.repeat_interleave(S, 0), group, **kw)
        for k in COLS + ('freq',):
            assert torch.equal(a[k], b[k]), (G, S, L, A, k)
        want, wfreq = statement(c['pos'], exp, c['group'], S, c['clash'], c['contact'], c['link'], c['bond'])
        _assert_equals_statement(a, want, wfreq, (G, S, L, A, 'shared'))


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    """Negative / NaN / infinite cutoffs, a NaN bond_max, A = 16, link with A = 2, L = 0, negative G and G > 65535 through the C entry point: ABOPT_EINVAL with a
    message, and out / freq keep the pattern they were filled with; a short workspace: ABOPT_EWORKSPACE.  The Python wrapper raises ValueError for the same and
    for candidates that are not whole groups."""
    from ab_opt_amd import hip
    L_ = hip.lib()
    G, S, L, A = 2, 5, 65, 15
    c = case(G, S, L, A)
    pos, mask, group, link = dev(c, 'pos', 'mask', 'group', 'link')
    out = torch.full((G * S, 5), 77, dtype=torch.int32, device=DEV)
    freq = torch.full((G, L), 77, dtype=torch.int32, device=DEV)
    need = L_.abopt_interface_geometry_ws_bytes(G, S, L)
    assert need == G * S * (3 + 4) * 4 and L_.abopt_interface_geometry_ws_bytes(0, S, L) == 0 and L_.abopt_interface_geometry_ws_bytes(G, 0, L) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def call(G=G, S=S, L=L, A=A, clash=3.0, contact=5.0, bond=2.0, link=link, ws_bytes=need):
        return L_.abopt_interface_geometry_grouped(hip.ptr(pos), hip.ptr(mask), 0, hip.ptr(group), hip.ptr(link, optional=True), G, S, L, A, clash, contact, bond,
                                                   hip.ptr(out), hip.ptr(freq), hip.ptr(ws), ws_bytes, hip.stream())
    for bad in (-1.0, float('nan'), float('inf')):
        assert call(clash=bad) == 1 and 'cutoffs' in L_.abopt_last_error().decode()
        assert call(contact=bad) == 1
    assert call(bond=float('nan')) == 1 and call(bond=float('inf')) == 1 and 'bond_max' in L_.abopt_last_error().decode()
    assert call(A=16) == 1 and '16' in L_.abopt_last_error().decode()
    assert call(A=2) == 1 and 'link' in L_.abopt_last_error().decode()
    assert call(A=0) == 1 and call(L=0) == 1 and call(G=-1) == 1 and call(S=-1) == 1
    assert call(G=65536, S=1) == 1 and '65535' in L_.abopt_last_error().decode()
    assert call(ws_bytes=need - 1) == 4 and 'workspace too small' in L_.abopt_last_error().decode()
    assert call(G=0) == 0 and call(S=0) == 0                          # no-ops
    torch.cuda.synchronize()
    assert (out == 77).all() and (freq == 77).all()
    assert call(clash=c['clash'], contact=c['contact'], bond=c['bond']) == 0     # ... and the same buffers are filled by a good call
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), c['out_link']) and np.array_equal(freq.cpu().numpy(), c['freq_link'])
    assert call(clash=c['clash'], contact=c['contact'], bond=-1.0) == 0         # a negative bond_max: breaks are not counted
    torch.cuda.synchronize()
    assert (out[:, 4] == 0).all() and np.array_equal(out[:, :4].cpu().numpy(), c['out_link'][:, :4])
    for name in ('clash_cutoff', 'contact_cutoff', 'bond_max'):
        for bad in (-2.0, float('nan')):
            with pytest.raises(ValueError, match=name):
                hip.interface_geometry_grouped(pos, mask, group, **{name: bad})
    with pytest.raises(ValueError, match='1 .. 15'):
        hip.interface_geometry_grouped(torch.zeros(2, 5, 16, 3, device=DEV), torch.ones(2, 5, 16, dtype=torch.bool, device=DEV), group[:, :5])
    with pytest.raises(ValueError, match='A >= 3'):
        hip.interface_geometry_grouped(pos[:, :, :2], mask[:, :, :2], group, link=link)
    with pytest.raises(ValueError, match='whole groups'):
        hip.interface_geometry_grouped(pos[:9], mask[:9], group)
    with pytest.raises(ValueError, match='whole groups'):
        hip.interface_geometry_grouped(pos, mask, group[:, :64])
    with pytest.raises(RuntimeError, match='HIP device only'):
        hip.interface_geometry_grouped(pos.cpu(), mask.cpu(), group.cpu())


@pytest.mark.gpu
def test_call_is_capturable():
    """One call recorded with torch.cuda.graph (three launches on one stream: a single chain, no parallel branch, no memset node) and replayed on OTHER inputs copied into
    the static tensors gives what the eager call gives on them."""
    from ab_opt_amd import hip
    G, S, L, A = 2, 5, 65, 15
    a = case(G, S, L, A)
    other = _raw(G, S, L, A, 4242)                                                # other inputs of the same shape; eager against captured, no float64 here
    names = ('pos', 'mask', 'group', 'link')
    kw = dict(clash_cutoff=a['clash'], contact_cutoff=a['contact'], bond_max=a['bond'], want_freq=True)
    first, held = harness.capture_replays_on_other_inputs(lambda **t: hip.interface_geometry_grouped(**t, **kw), dict(zip(names, dev(a, *names))),
                                                          {n: torch.from_numpy(src).to(DEV) for n, src in zip(names, other)})
    _assert_equals_statement(first, a['out_link'], a['freq_link'], 'replay on the captured inputs')
    assert not torch.equal(held['contacts'], torch.from_numpy(a['out_link'][:, 1]).to(DEV).int()), 'the other inputs give other counts'


# ------------------------------------------------------------------------------------------ GPU: the screen
GEOM = dict(interface_geometry_workers.GEOM)
assert GEOM == dict(clash_cutoff=CLASH, contact_cutoff=CONTACT, bond_max=BOND)


@pytest.mark.gpu
def test_screen_fields_do_not_change_with_geometry_on(screen_models):
    """Geometry draws nothing and steers nothing: every field the screen returns without the three cutoffs is torch.equal in a run with them, which adds exactly
    pose_geom (P, 5), redock_geom (P, k, D, 5) int64 and epitope_freq (P, k, L) fp32 in [0, 1]; one cutoff alone switches the scoring on with the defaults."""
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    kw = dict(screen_workers.SCREEN)
    P, k, D, L = kw['num_poses'], kw['screened_per_pose'], kw['redocks_per_design'], one['aa'].shape[1]
    plain = screen.optimize_antibody(dock, design, one, poses_per_launch=2, **kw)
    geom = screen.optimize_antibody(dock, design, one, poses_per_launch=2, **kw, **GEOM)
    new = {'pose_geom', 'redock_geom', 'epitope_freq'}
    assert set(geom) == set(plain) | new and not set(plain) & new
    for name, v in plain.items():
        assert torch.equal(geom[name], v), name
    assert geom['pose_geom'].shape == (P, 5) and geom['pose_geom'].dtype == torch.int64
    assert geom['redock_geom'].shape == (P, k, D, 5) and geom['redock_geom'].dtype == torch.int64
    assert geom['epitope_freq'].shape == (P, k, L) and geom['epitope_freq'].dtype == torch.float32
    assert ((geom['epitope_freq'] >= 0) & (geom['epitope_freq'] <= 1)).all() and (geom['pose_geom'] >= 0).all() and (geom['redock_geom'] >= 0).all()
    only = screen.optimize_antibody(dock, design, one, poses_per_launch=2, **kw, contact_cutoff=CONTACT)
    assert torch.equal(only['redock_geom'][..., :4], geom['redock_geom'][..., :4]) and (only['redock_geom'][..., 4] == 0).all()
    assert torch.equal(only['pose_geom'][:, :4], geom['pose_geom'][:, :4]) and torch.equal(only['epitope_freq'], geom['epitope_freq'])
    assert screen.screen_filter(geom, max_clashes=10 ** 9, min_contacts=0).equal(screen.screen_filter(plain))


@pytest.mark.gpu
def test_screen_geometry_equals_the_public_calls(screen_models):
    """pose_geom, and redock_geom / epitope_freq of the one chunk of a screen with all poses in one launch, against the same stages written out with the public
    calls and scored by sampler.interface_geometry(groups='chains') -- the poses as one group of P, the re-docks as P k groups of D -- and, design by design,
    by single-group calls of hip.interface_geometry_grouped.  The hash-filled models' poses touch the antigen: some count is non-zero."""
    from ab_opt_amd import hip, sampler
    P, S, k, D, contig, seed = 4, 3, 2, 3, '33-39', 5
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    L = one['aa'].shape[1]
    pose_pos, pose_mask, rpos, rmask = harness.stages(dock, design, one, P, S, k, D, contig, seed)
    res = screen.optimize_antibody(dock, design, one, P, S, D, contig=contig, screened_per_pose=k, seed=seed, poses_per_launch=P, screen_by='ppl', **GEOM)
    stack = lambda g: torch.stack([g[c] for c in COLS], 1).long()
    poses = sampler.interface_geometry(one, pose_pos, pose_mask, groups='chains', **GEOM)
    assert torch.equal(res['pose_geom'], stack(poses))
    many = {name: one[name].expand(P * k, L) for name in ('fragment_type', 'chain_nb', 'res_nb', 'generate_flag')}
    redocks = sampler.interface_geometry(many, rpos, rmask, groups='chains', want_freq=True, **GEOM)
    assert torch.equal(res['redock_geom'], stack(redocks).view(P, k, D, 5))
    assert torch.equal(res['epitope_freq'], (redocks['freq'].float() / D).view(P, k, L))
    grp = screen.chain_groups(one['fragment_type'])
    link = sampler.backbone_links(one['chain_nb'], one['res_nb'])
    for i in range(P * k):
        sl = slice(i * D, (i + 1) * D)
        alone = hip.interface_geometry_grouped(rpos[sl], rmask[sl], grp, CLASH, CONTACT, link=link, bond_max=BOND, want_freq=True)
        assert torch.equal(res['redock_geom'].view(P * k, D, 5)[i], stack(alone)), i
        assert torch.equal(res['epitope_freq'].view(P * k, L)[i], alone['freq'][0].float() / D), i
    assert res['pose_geom'].sum() > 0 and res['redock_geom'].sum() > 0
    assert (res['epitope_freq'][..., (grp[0] == 0)] == 0).all()
    # 'generated': the docked residues against everything else, their bonded neighbours excluded
    gen = sampler.interface_geometry(one, pose_pos, pose_mask, groups='generated', **GEOM)
    side = torch.where(one['generate_flag'].bool(), 1, torch.where(one['fragment_type'] > 0, 2, 0))
    want = hip.interface_geometry_grouped(pose_pos, pose_mask, side, CLASH, CONTACT, link=link, bond_max=BOND)
    for c in COLS:
        assert torch.equal(gen[c], want[c]), c
    assert (gen['iface1'] <= int(one['generate_flag'].sum())).all()


@pytest.mark.gpu
def test_screen_geometry_does_not_depend_on_poses_per_launch(monkeypatch, screen_models):
    """The screen with geometry on, with all, 1 and 2 poses per launch: every field, the three new ones included, bit for bit -- ABOPT_PAIR_TERMS=0 /
    ABOPT_CORE_NO_SPLIT=1 pin one arithmetic form of the denoiser, as DESIGN.md section 6.1 prescribes and tests/test_screen.py does."""
    harness.pin_denoiser_form(monkeypatch)
    harness.screen_is_launch_size_invariant(screen_models, GEOM, {'pose_geom', 'redock_geom', 'epitope_freq'})


@pytest.mark.gpu
def test_two_rank_screen_gathers_the_geometry_fields(tmp_path, monkeypatch, screen_models):
    """Two gloo ranks sharing cuda:0 (5 poses split 3 + 2, two per launch) return what one process returns, the three new fields included, bit for bit -- without
    clustering, where pose_geom travels in the final gather, and with cluster_cutoff = 0.0, where it is gathered with the poses before stage 2 and stays (P, 5).
    ABOPT_PAIR_TERMS=0 / ABOPT_CORE_NO_SPLIT=1 as in tests/test_screen.py."""
    harness.pin_denoiser_form(monkeypatch)
    dock, design = screen_models
    one = screen_workers.complex_(DEV)
    kw = dict(screen_workers.SCREEN)
    ref = {f'geometry_{tag}': screen.optimize_antibody(dock, design, one, poses_per_launch=kw['num_poses'], **kw, **GEOM, **extra)
           for tag, extra in interface_geometry_workers.RUNS.items()}
    plain, zero = ref['geometry_plain'], ref['geometry_zero']
    assert torch.equal(plain['pose_geom'], zero['pose_geom']) and torch.equal(plain['redock_geom'], zero['redock_geom'])
    harness.two_ranks_return(interface_geometry_workers.geometry_screen_worker, tmp_path, ref)
