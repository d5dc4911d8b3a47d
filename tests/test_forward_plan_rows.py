"""Masked query rows in the plan of a forward (ab_opt_amd/csrc/forward_plan.h: query_rows_masked) without a device.  tests/forward_plan_rows_table.cpp, a host-only
program, tabulates plan_network for both entries (abopt_eps_net_forward, abopt_eps_net_step), with and without the caller's context_unused, over geometries, CU counts,
operands, weight lists and the switches; here the rule is restated from the columns of every line: the flag is set on the LAST block and nowhere else, only for a step
whose tail is fused, whose last block is the fused 32-row kernel on a pair-bias cache, with ABOPT_STEP_ROWS not 0 -- and it moves nothing else in the plan."""
from collections import namedtuple

import pytest

from plan_tables import table_lines

Query = namedtuple('Query', 'N L cus z cache terms ovr wl mix heads prmsd')
Call = namedtuple('Call', 'entry ppl context_unused fuse_step fuse_heads fuse_tail step_rows fuse_node dbg')
Block = namedtuple('Block', 'node_kernel form tail carry_next carried frag_slot xt_read xt_write qk_terms masked')
Row = namedtuple('Row', 'q c step_fused ok blocks same')


@pytest.fixture(scope='module')
def table():
    rows = []
    for line in table_lines('forward_plan_rows_table'):
        body, same = line.split(' || ')
        q, c, net, blocks = body.split(' | ')
        net, f = list(map(int, net.split())), blocks.lstrip('| ').split()
        assert len(f) == 10 * net[2]
        bl = [Block(int(b[0]), b[1], b[2], *map(int, b[3:])) for b in (f[i:i + 10] for i in range(0, len(f), 10))]
        rows.append(Row(Query(*map(int, q.split())), Call(*map(int, c.split())), net[0], net[1], bl, int(same)))
    return rows


def test_grid_is_complete(table):
    assert len(table) > 10000
    assert {(r.q.N, r.q.L) for r in table} >= {(2, 80), (3, 64), (32, 256)} and {r.q.cus for r in table} == {8, 256}
    assert {r.c.entry for r in table} == {0, 1} and {r.c.context_unused for r in table} == {0, 1} and {r.c.ppl for r in table} == {0, 1}
    assert {r.q.prmsd for r in table} == {0, 1} and {r.q.cache for r in table} == {0, 1} and {r.c.step_rows for r in table} == {0, 1}
    assert {b.form for r in table for b in r.blocks} >= {'OneBlock', 'Persist', 'Core32'}
    assert {b.tail for r in table for b in r.blocks} == {'InCore', 'OutLnMlp', 'Gemm'}


def test_rule_on_every_line(table):
    seen = 0
    for r in table:
        assert r.same, r                                                    # nothing else in the plan moves; a query without the caller's word masks nothing;
        #                                                                     a lone block and a lone encoder never mask
        assert not any(b.masked for b in r.blocks[:-1]), r                  # never on a block somebody follows
        if not r.blocks:
            continue
        last = r.blocks[-1]
        fused_tail = r.c.entry == 1 and r.q.mix and r.q.heads and r.c.fuse_heads and r.c.fuse_step and not r.q.prmsd and not r.c.ppl
        assert bool(r.step_fused) == bool(fused_tail), r
        want = bool(r.ok and r.c.context_unused and fused_tail and last.form == 'Core32' and r.q.cache and last.tail == 'InCore' and not last.carry_next and
                    r.c.step_rows and not r.c.dbg)
        assert bool(last.masked) == want, r
        seen += last.masked
    assert seen > 100


def test_never_for(table):
    """the cases the kernel may not meet, one by one"""
    masked = [r for r in table if any(b.masked for b in r.blocks)]
    assert masked
    for r in masked:
        assert r.c.entry == 1 and r.c.context_unused                        # abopt_eps_net_forward never; only on the caller's word
        assert not r.q.prmsd and not r.c.ppl                                # a prmsd head, perplexity: per-sample reductions over every row
        assert r.blocks[-1].form == 'Core32' and r.q.cache                  # a 16-row core, no cache
        assert r.c.step_rows and r.c.fuse_step and r.c.fuse_heads and r.c.fuse_tail
        assert [b.masked for b in r.blocks] == [0] * (len(r.blocks) - 1) + [1] and not r.blocks[-1].carry_next
    # each of the refusals is in the grid next to a query that differs in that one thing and is masked
    key = lambda r, **kw: (r.q, r.c._replace(**kw))
    got = {(r.q, r.c) for r in masked}
    base = next(r for r in masked if r.q.N == 32 and r.q.L == 256 and r.q.cus == 256 and r.q.wl == 0 and r.q.terms and r.q.ovr == -1)
    for kw in (dict(entry=0), dict(ppl=1), dict(context_unused=0), dict(step_rows=0), dict(fuse_step=0), dict(fuse_heads=0), dict(fuse_tail=0)):
        assert key(base, **kw) in {(r.q, r.c) for r in table} and key(base, **kw) not in got, kw
    for kw in (dict(prmsd=1), dict(cache=0, terms=0), dict(ovr=0)):
        k = (base.q._replace(**kw), base.c)
        assert k in {(r.q, r.c) for r in table} and k not in got, kw


def test_pinned_bench_shape(table):
    """(32, 256) on 256 CUs, cache + terms, everything packed, no switch: blocks 0 and 1 carry their successor's fragments, block 2 -- the last -- masks its query rows"""
    (r,) = [r for r in table if r.q == Query(32, 256, 256, 0, 1, 1, -1, 0, 1, 1, 0) and r.c == Call(1, 0, 1, 1, 1, 1, 1, 1, 0)]
    assert [(b.form, b.tail, b.carry_next, b.masked) for b in r.blocks] == [('Core32', 'InCore', 1, 0), ('Core32', 'InCore', 1, 0), ('Core32', 'InCore', 0, 1)]


def test_shapes_of_the_gpu_test_are_masked(table):
    """tests/test_step_rows.py compares flag on with flag off bit for bit, which proves nothing where the plan refuses: its shapes under ABOPT_CORE32=1 on 256 CUs,
    with pair terms and without, distinct and shared pair features"""
    for N, L, z in ((2, 80, 0), (3, 64, 3)):
        for terms in (0, 1):
            (r,) = [r for r in table if r.q == Query(N, L, 256, z, 1, terms, 1, 0, 1, 1, 0) and r.c == Call(1, 0, 1, 1, 1, 1, 1, 1, 0)]
            assert [b.masked for b in r.blocks] == [0, 0, 1], (N, L, z, terms)
