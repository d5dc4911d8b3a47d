"""Carried fragments in the plan of a forward (ab_opt_amd/csrc/forward_plan.h: carry_next / carried / frag_slot) without a device.  tests/forward_plan_carry_table.cpp,
a host-only program, tabulates the decision over the grid of tests/forward_plan_table.cpp with the switch on, with the switch off (ABOPT_FUSE_NODE=0) and without a
second fragment pair in the workspace; a forward whose 32-row workgroups need more than one round of the CUs is not carried (measured: forward_plan.h); what the
kernels rely on -- who writes which fragment slot while who reads which -- is checked on every line, the columns of the older table are compared with that
program's own output, and two forwards are pinned."""
from collections import namedtuple

import pytest

from plan_tables import table_lines

Variant = namedtuple('Variant', 'fuse_node frag2 same blocks')        # blocks: [(carry_next, carried, frag_slot)]
Row = namedtuple('Row', 'legacy q ok tails node_kernel variants')


@pytest.fixture(scope='module')
def tables():
    old = table_lines('forward_plan_table')
    rows, pins = [], {}
    for line in table_lines('forward_plan_carry_table'):
        if line.startswith('pin '):
            head, _, body = line[4:].partition('|')
            h, b = list(map(int, head.split())), list(map(int, body.split()))
            pins[tuple(h[:3])] = (h[3], list(zip(b[0::3], b[1::3], b[2::3])))
            continue
        legacy, *vs = line.split(' || ')
        q, net, *blocks, _enc, _single = legacy.split(' | ')
        net = net.split()
        blocks = [b.split() for b in blocks]
        variants = []
        for v in vs:
            head, _, body = v.partition('|')
            h, b = list(map(int, head.split())), list(map(int, body.split()))
            variants.append(Variant(h[0], h[1], h[2], list(zip(b[0::3], b[1::3], b[2::3]))))
        rows.append(Row(legacy, tuple(map(int, q.split())), int(net[1]), [b[4] for b in blocks], [int(b[0]) for b in blocks], variants))
    return old, rows, pins


def test_older_columns_are_unchanged(tables):
    """the carry decision is additive: node, qk_terms, core, tail and the x-term slots are the older table's on every row, whatever fuse_node and frag2 are"""
    old, rows, _ = tables
    assert len(old) == len(rows) > 1000
    for o, r in zip(old, rows):
        assert o == r.legacy
        assert [(v.fuse_node, v.frag2) for v in r.variants] == [(1, 1), (0, 1), (1, 0)] and all(v.same for v in r.variants), r.legacy


def test_carry_rules_over_the_grid(tables):
    _, rows, _ = tables
    seen = set()
    for r in rows:
        N, L, cus, ask = r.q[0], r.q[1], r.q[2], r.q[6]
        for v in r.variants:
            nb = len(v.blocks)
            assert nb == len(r.tails)
            for i, (cn, cd, slot) in enumerate(v.blocks):
                assert slot in (0, 1), r.legacy
                assert cd == (v.blocks[i - 1][0] if i else 0), r.legacy                  # carried[i + 1] == carry_next[i]; nobody writes block 0's fragments for it
                # one round: the grid of a Core32 plan (CorePlan::grid = N ceil(L / 32) workgroups, tests/test_ipa_plan.py pins it) fits the CUs at once -- where the phase
                # was measured to pay (forward_plan.h; profiles/node_carry_shapes.txt).  The plan's own formula restated: a pin of the rule, not an independent reference.
                one_round = N * ((L + 31) // 32) <= cus
                want = bool(i and r.ok and r.tails[i - 1] == 'InCore' and r.node_kernel[i] and r.tails[i] == 'InCore' and v.fuse_node and v.frag2 and ask < 2 and one_round)
                assert bool(cd) == want, r.legacy
                if cd:
                    assert slot != v.blocks[i - 1][2], r.legacy                          # never the slot its producer's own core reads
                else:
                    assert slot == 0, r.legacy                                          # block 0 and every uncarried block: slot 0
                if cn:
                    assert i + 1 < nb and v.blocks[i + 1][2] != slot, r.legacy          # no block reads the slot it is writing for its successor
            assert not v.blocks or not v.blocks[-1][0], r.legacy                        # the last block never produces
            if not (v.fuse_node and v.frag2):
                assert all(b == (0, 0, 0) for b in v.blocks), r.legacy
            seen.add(tuple(v.blocks))
    assert {((0, 0, 0), (0, 0, 0), (0, 0, 0)), ((1, 0, 0), (1, 1, 1), (0, 1, 0)), ((0, 0, 0), (1, 0, 0), (0, 1, 1)), ((1, 0, 0), (0, 1, 1), (0, 0, 0))} <= seen


def _pinned(rows, N, L, wl):
    """256 CUs, cache + terms, the workspace's own scratch, no switches, mixer / heads packed with the blocks, a prmsd head"""
    (r,) = [r for r in rows if r.q == (N, L, 256, 0, 1, 1, 0, 1, -1, 0, 1, 1, 1, wl, int(wl == 0), int(wl == 0), 1)]
    return r


def test_pinned_bench_shape(tables):
    """(32, 256) with cache + terms: block 0 behind its own node_frags, blocks 1 and 2 carried; the fragment slots alternate 0 -> 1 -> 0"""
    r = _pinned(tables[1], 32, 256, 0)
    assert r.variants[0].blocks == [(1, 0, 0), (1, 1, 1), (0, 1, 0)]
    assert r.variants[1].blocks == r.variants[2].blocks == [(0, 0, 0)] * 3


def test_pinned_plain_block_in_the_middle(tables):
    """block 1 plain (GEMM node step, GEMM tail): it is not carried and it cannot produce, so nothing is carried"""
    r = _pinned(tables[1], 32, 256, 3)
    assert r.tails == ['InCore', 'Gemm', 'InCore']
    assert all(v.blocks == [(0, 0, 0)] * 3 for v in r.variants)


def test_shapes_of_the_gpu_test_are_carried(tables):
    """tests/test_node_carry.py compares the carried path with ABOPT_FUSE_NODE=0 bit for bit, which proves nothing where the plan falls back.  Its shapes under its
    switches on 256 CUs, with frag2 from the workspace's own fit rule (plan_frag2_fits, what carve_ga calls): every one carries blocks 1 and 2 over the slots 0, 1, 0,
    except L = 17, which is there because it does not fit.  The fit rule's edge: two padded row tiles (288 KB of fragments per sample) fit over proj | feat (15.1 KB per
    row) from L = 20 on; from L = 32 on every length fits."""
    pins = tables[2]
    chain = [(1, 0, 0), (1, 1, 1), (0, 1, 0)]
    for key in ((2, 33, 0), (2, 48, 0), (3, 70, 0), (8, 64, 0), (4, 48, 2), (32, 256, 0)):
        assert pins[key] == (1, chain), key
    assert pins[(2, 17, 0)] == (0, [(0, 0, 0)] * 3)
    assert pins[(2, 19, 0)][0] == 0 and pins[(2, 20, 0)] == (1, chain)
