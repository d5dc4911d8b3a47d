"""When a denoising step's tail runs as one launch (ab_opt_amd/csrc/forward_plan.h: NetPlan::step_fused / mixer_launch / step_carry behind abopt_eps_net_step), without a
device: tests/step_plan_table.cpp, a host-only program, tabulates the fields over the switch, the packed mixer / heads operands, the prmsd head, a perplexity request
and the carry flags; the rule is checked on every line, and the bench shape (fused) and an AbDock call (not fused) are pinned."""
from collections import namedtuple

import pytest

from plan_tables import build_table

Query = namedtuple('Query', 'fuse_step fuse_heads x_terms mix heads prmsd ppl step carry_in carry_out')
Plan = namedtuple('Plan', 'step_fused mixer_launch step_carry mixer_kernel mixer_xt heads_kernel heads_epilogue')


@pytest.fixture(scope='module')
def table():
    return dict(build_table('step_plan_table', lambda *f: (Query(*f[:len(Query._fields)]), Plan(*f[len(Query._fields):]))))


def test_grid_is_complete(table):
    assert len(table) == 1 << 10
    assert {p.step_fused for p in table.values()} == {0, 1} and {p.mixer_launch for p in table.values()} == {0, 1} and {p.step_carry for p in table.values()} == {0, 1}


def test_the_rule_over_the_grid(table):
    for q, p in table.items():
        fused = bool(q.step and q.mix and q.heads and q.fuse_heads and q.fuse_step and not q.prmsd and not q.ppl)
        assert p.step_fused == fused, q
        assert p.mixer_launch == (not (fused and q.carry_in)), q            # only a fused call trusts a carried mixer output ...
        assert p.step_carry == (fused and bool(q.carry_out)), q             # ... and only a fused call leaves one
        if fused:                                                           # the fused tail is the heads kernel with its epilogue, and writes what the mixer kernel writes
            assert p.mixer_kernel and p.heads_kernel and p.heads_epilogue, q
            assert p.mixer_xt == (1 if q.x_terms else -1), q
        # the forward's own fields do not depend on the step
        base = table[q._replace(step=0, ppl=0, carry_in=0, carry_out=0)]
        assert p[3:] == base[3:], q
        if not q.step:
            assert (p.step_fused, p.mixer_launch, p.step_carry) == (0, 1, 0), q


def test_pinned_bench_shape(table):
    """AbDesign flavour, everything packed, no switch set: the first step of a loop launches the mixer and carries out, the middle ones do neither launch, the last
    one carries nothing out"""
    q = Query(1, 1, 1, 1, 1, 0, 0, 1, 0, 1)
    assert table[q] == Plan(1, 1, 1, 1, 1, 1, 1)
    assert table[q._replace(carry_in=1)] == Plan(1, 0, 1, 1, 1, 1, 1)
    assert table[q._replace(carry_in=1, carry_out=0)] == Plan(1, 0, 0, 1, 1, 1, 1)
    assert table[q._replace(fuse_step=0, carry_in=1)] == Plan(0, 1, 0, 1, 1, 1, 1)


def test_pinned_abdock_call(table):
    """AbDock flavour: a prmsd head and a perplexity request -- three launches, the mixer at the head of every call, whatever the carry flags say"""
    for cin in (0, 1):
        for cout in (0, 1):
            assert table[Query(1, 1, 1, 1, 1, 1, 1, 1, cin, cout)] == Plan(0, 1, 0, 1, 1, 1, 1)
