"""Gathered query rows in the plan of a forward (ab_opt_amd/csrc/forward_plan.h: query_rows_compact) without a device.  tests/forward_plan_compact_table.cpp, a
host-only program, tabulates plan_network for abopt_eps_net_step over geometries, CU counts, block counts, tile counts of the caller's row list and the switches; here
the rule is restated from the columns of every line: the last block gathers only where it masks its query rows already, the caller gave a list, ABOPT_STEP_COMPACT is
not 0, N x tiles workgroups fit the CUs in one round, tiles <= ceil(L / 32) and the net has three blocks or more -- and it moves nothing else in the plan."""
from collections import namedtuple

import pytest

from plan_tables import build_table

Row = namedtuple('Row', 'N L cus z terms ovr nb tiles context_unused step_rows step_compact ppl prmsd ok masked compact compact_grid core_grid elsewhere same')


@pytest.fixture(scope='module')
def table():
    return build_table('forward_plan_compact_table', Row)


def test_grid_is_complete(table):
    assert len(table) > 10000
    assert {(r.N, r.L) for r in table} >= {(2, 80), (3, 48), (17, 256), (24, 256), (32, 256)} and {r.cus for r in table} == {8, 64, 256, 304}
    assert {r.tiles for r in table} == set(range(11)) and {r.nb for r in table} == {1, 2, 3, 6}
    assert {r.step_compact for r in table} == {0, 1} and {r.context_unused for r in table} == {0, 1} and {r.masked for r in table} == {0, 1}


def test_rule_on_every_line(table):
    seen = 0
    for r in table:
        assert r.ok and r.same and not r.elsewhere, r                       # nothing else in the plan moves; never on a block somebody follows
        want = bool(r.masked and r.tiles > 0 and r.step_compact and r.N * r.tiles <= r.cus and r.tiles <= (r.L + 31) // 32 and r.nb >= 3)
        assert r.compact == (r.tiles if want else 0), r
        assert r.compact_grid == (r.N * r.tiles if want else 0), r
        seen += want
    assert seen > 100


def test_never_for(table):
    """the refusals one by one, each next to a query that differs in that one thing and gathers"""
    got = {r[:13] for r in table if r.compact}
    base = next(r for r in table if (r.N, r.L, r.cus, r.z, r.terms, r.ovr, r.nb, r.tiles) == (32, 256, 256, 0, 1, -1, 6, 4) and r.compact)
    assert base.context_unused and base.step_rows and base.step_compact and not base.ppl and not base.prmsd
    every = {r[:13] for r in table}
    for kw in (dict(tiles=0), dict(tiles=9), dict(tiles=9, cus=304), dict(nb=1), dict(nb=2), dict(cus=64), dict(context_unused=0), dict(step_rows=0),
               dict(step_compact=0), dict(ppl=1), dict(prmsd=1), dict(ovr=0)):
        k = base._replace(**kw)[:13]
        assert k in every and k not in got, kw
    assert base._replace(tiles=8)[:13] in got and base._replace(tiles=1)[:13] in got            # up to half the rows, at 256 CUs
    for r in table:
        if r.compact:
            assert r.masked and r.context_unused and not r.ppl and not r.prmsd and r.nb >= 3 and r.compact_grid <= r.cus


def test_pinned_bench_shape(table):
    """(32, 256) on 256 CUs, six blocks, 53 generated rows per sample in four 16-row tiles: 128 workgroups where the masked form runs 256"""
    (r,) = [r for r in table if (r.N, r.L, r.cus, r.z, r.terms, r.ovr, r.nb, r.tiles) == (32, 256, 256, 0, 1, -1, 6, 4) and
            (r.context_unused, r.step_rows, r.step_compact, r.ppl, r.prmsd) == (1, 1, 1, 0, 0)]
    assert (r.masked, r.compact, r.compact_grid, r.core_grid) == (1, 4, 128, 256)


def test_shapes_of_the_gpu_test_gather(table):
    """tests/test_step_compact.py compares the entry with the row list against the masked form bit for bit, which proves nothing where the plan refuses: its shapes under
    ABOPT_CORE32=1 on 256 CUs with a three-block net gather for one to three (L = 80) and one or two (L = 48) tiles, and refuse beyond"""
    for N, L, most in ((2, 80, 3), (3, 48, 2)):
        for terms in (0, 1):
            for z in (0, N):
                rows = {r.tiles: r for r in table if (r.N, r.L, r.cus, r.z, r.terms, r.ovr, r.nb) == (N, L, 256, z, terms, 1, 3) and
                        (r.context_unused, r.step_rows, r.step_compact, r.ppl, r.prmsd) == (1, 1, 1, 0, 0)}
                assert [rows[t].compact for t in range(6)] == [t if 1 <= t <= most else 0 for t in range(6)], (N, L, z, terms)
                assert all(rows[t].masked for t in range(6))
