"""The launches of a denoiser forward (ab_opt_amd/csrc/forward_plan.h: plan_block / plan_encoder / plan_network) without a device: tests/forward_plan_table.cpp, a
host-only program, tabulates the plans of a three-block net over geometries, CU counts, operands given, switches and weight lists; what the kernels rely on -- who
writes term-form fragments and x terms, and who reads them -- is checked on every line, and three forwards are pinned."""
from collections import namedtuple

import pytest

from plan_tables import table_lines

GEOMETRIES = {(2, 33), (3, 70), (8, 256), (16, 256), (32, 256), (48, 256), (1000, 48), (1366, 256)}
Query = namedtuple('Query', 'N L cus z cache terms ask ws ovr no_split fuse_tail x_terms fuse_heads wl mix heads prmsd')
Net = namedtuple('Net', 'used ok num_blocks mixer_kernel mixer_xt heads_kernel heads_epilogue build_infeat prmsd')
Block = namedtuple('Block', 'node_kernel qk_terms form nsplit tail xt_read xt_write')
Row = namedtuple('Row', 'q net blocks enc_slots single')
TERM_TAILS = ('InCore', 'OutLnMlp')


def _block(text):
    f = text.split()
    return Block(int(f[0]), int(f[1]), f[2], int(f[3]), f[4], int(f[5]), int(f[6]))


@pytest.fixture(scope='module')
def table():
    rows = []
    for line in table_lines('forward_plan_table'):
        q, net, *blocks, enc, single = line.split(' | ')
        e = list(map(int, enc.split()))
        s = single.split()
        rows.append(Row(Query(*map(int, q.split())), Net(*map(int, net.split())), [_block(b) for b in blocks], list(zip(e[0::2], e[1::2])),
                        (s[0], int(s[1]), int(s[2]))))
    return rows


def packed(q, i):
    """block i of weight list q.wl carries the four packed operands (0: all do, 1: none does, 2 / 3 / 4: all but block 0 / 1 / 2)"""
    return q.wl == 0 or (q.wl >= 2 and q.wl - 2 != i)


def slab_fits_u32(q):
    return (q.N // q.z if q.z > 1 else q.N) * q.L * ((q.L + 15) // 16) * 768 < (1 << 32)


def test_grid_is_complete(table):
    assert {(r.q.N, r.q.L) for r in table} == GEOMETRIES
    assert {r.q.cus for r in table} == {8, 256} and {r.q.z for r in table} == {0, 16}
    assert {(r.q.cache, r.q.terms) for r in table} == {(0, 0), (1, 0), (1, 1)} and {r.q.ask for r in table} == {0, 1, 2, 3}
    assert {r.q.wl for r in table} == {0, 1, 2, 3, 4} and {r.q.ws for r in table} == {0, 1}
    # the switch settings the suite runs under (ABOPT_CORE32, _CORE_NO_SPLIT, _FUSE_TAIL, _X_TERMS, _FUSE_HEADS as values)
    assert {(r.q.ovr, r.q.no_split, r.q.fuse_tail, r.q.x_terms, r.q.fuse_heads) for r in table} >= {
        (-1, 0, 1, 1, 1), (1, 0, 1, 1, 1), (0, 0, 1, 1, 1), (-1, 1, 1, 1, 1), (1, 1, 1, 1, 1), (0, 1, 1, 1, 1), (-1, 0, 0, 1, 1), (-1, 0, 1, 0, 1), (-1, 0, 0, 0, 1),
        (-1, 1, 0, 1, 1), (0, 1, 0, 1, 1), (1, 1, 0, 1, 1), (-1, 0, 1, 1, 0), (1, 0, 1, 0, 1)}
    assert {b.form for r in table for b in r.blocks} == {'OneBlock', 'Persist', 'Split', 'Core32', 'Unsupported'}
    assert {b.tail for r in table for b in r.blocks} == {'InCore', 'OutLnMlp', 'Gemm'}
    assert any(b.qk_terms for r in table for b in r.blocks) and any(b.xt_write == 1 for r in table for b in r.blocks)


def test_fragment_and_tail_forms_over_the_grid(table):
    for r in table:
        q = r.q
        for i, b in enumerate(r.blocks):
            assert b.node_kernel == packed(q, i), r
            # term-form q / k fragments are written exactly for the one core that reads them: the 32-row kernel handed pair terms
            assert bool(b.qk_terms) == (b.form == 'Core32' and bool(q.cache and q.terms and b.node_kernel) and q.ask < 2), r
            if b.form in ('Persist', 'Split', 'OneBlock', 'Unsupported'):
                assert not b.qk_terms, r
            in_core = b.form == 'Core32' and bool(q.cache) and packed(q, i) and q.ask == 0 and bool(q.fuse_tail)
            assert (b.tail == 'InCore') == in_core, r
            if not in_core:
                assert b.tail == ('OutLnMlp' if packed(q, i) else 'Gemm'), r
            if q.cache and q.ask != 3:
                assert r.net.used == (b.form == 'Core32'), r        # abopt_pair_terms_used, asked without scratch, agrees with every cached block plan
            assert len({(b.form, b.nsplit) for b in r.blocks}) == 1, r


def test_x_terms_chain_over_the_grid(table):
    for r in table:
        q, n = r.q, r.net
        assert n.mixer_kernel == q.mix and n.mixer_xt == (1 if q.mix and q.x_terms and packed(q, 0) else -1), r
        for slots, produced in (([(b.xt_read, b.xt_write) for b in r.blocks], n.mixer_xt), (r.enc_slots, -1)):     # behind the mixer | an encoder on its own
            assert len(slots) == n.num_blocks, r
            for i, (rd, wr) in enumerate(slots):
                b = r.blocks[i]
                assert rd == (produced if b.node_kernel else -1), r         # reads only what its producer wrote, and only through node_frags
                assert wr == -1 or wr != rd, r                              # never writes the slot it reads
                if wr != -1:
                    assert wr in (0, 1) and i + 1 < 3 and packed(q, i + 1) and b.tail in TERM_TAILS and q.x_terms, r
                if not q.x_terms:
                    assert rd == -1 and wr == -1, r
                produced = wr
        assert r.single[1:] == (-1, -1) and r.single[0] == r.blocks[0].tail, r     # a block on its own: same forms, no slots
        if not q.x_terms:
            assert n.mixer_xt == -1, r


def test_network_forms_and_the_unsupported_case(table):
    for r in table:
        q, n = r.q, r.net
        refuses = q.ask == 3 and q.cache and not slab_fits_u32(q)
        assert n.ok == (not refuses), r
        if refuses:                                                         # the dumping core cannot reach the slab: planned up to there and no further
            assert n.num_blocks == 1 and r.blocks[0].form == 'Unsupported' and (n.heads_kernel, n.heads_epilogue, n.build_infeat, n.prmsd) == (0, 0, 0, 0), r
            continue
        assert n.num_blocks == 3 and all(b.form != 'Unsupported' for b in r.blocks), r
        assert n.heads_kernel == q.heads and n.heads_epilogue == (q.heads and q.fuse_heads), r
        assert n.build_infeat == (not q.heads or q.prmsd) and n.prmsd == q.prmsd, r


def _pinned(table, N, L, wl, cache):
    """256 CUs, the workspace's own scratch, no switches, mixer / heads packed with the blocks, a prmsd head"""
    (r,) = [r for r in table if r.q == Query(N, L, 256, 0, cache, cache, 0, 1, -1, 0, 1, 1, 1, wl, int(wl == 0), int(wl == 0), 1)]
    return r


def test_pinned_bench_shape(table):
    """(32, 256) with cache + terms: every block is one 32-row launch behind node_frags, reading term fragments; x terms alternate 1 -> 0 -> 1"""
    r = _pinned(table, 32, 256, 0, 1)
    assert r.blocks == [Block(1, 1, 'Core32', 1, 'InCore', 1, 0), Block(1, 1, 'Core32', 1, 'InCore', 0, 1), Block(1, 1, 'Core32', 1, 'InCore', 1, -1)]
    assert r.net == Net(1, 1, 3, 1, 1, 1, 1, 1, 1)


def test_pinned_small_batch(table):
    """(8, 256): keys split over two workgroups, out_ln_mlp behind it, fp32 q / k slots, x terms still chained"""
    r = _pinned(table, 8, 256, 0, 1)
    assert r.blocks == [Block(1, 0, 'Split', 2, 'OutLnMlp', 1, 0), Block(1, 0, 'Split', 2, 'OutLnMlp', 0, 1), Block(1, 0, 'Split', 2, 'OutLnMlp', 1, -1)]
    assert r.net.used == 0 and r.net.mixer_xt == 1


@pytest.mark.parametrize('N,L', [(32, 256), (8, 256)])
def test_pinned_plain_weights(table, N, L):
    """no packed operand anywhere: GEMM + ipa_frags, split-K GEMM + fused_ln_mlp, no slots, the heads as GEMMs"""
    r = _pinned(table, N, L, 1, 1)
    assert [(b.node_kernel, b.qk_terms, b.tail, b.xt_read, b.xt_write) for b in r.blocks] == [(0, 0, 'Gemm', -1, -1)] * 3
    assert (r.net.mixer_kernel, r.net.mixer_xt, r.net.heads_kernel, r.net.heads_epilogue, r.net.build_infeat) == (0, -1, 0, 0, 1)
