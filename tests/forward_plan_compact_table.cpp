// Tabulates the gathered-query-rows decision of plan_network / plan_encoder (ab_opt_amd/csrc/forward_plan.h: query_rows_compact) for tests/test_forward_plan_compact.py.
// Host C++17 only: no HIP, no device.  A fully packed net with a cache over geometries, CU counts, block counts and tile counts; one line per query:
//   N L cus z terms ovr nb tiles | context_unused step_rows step_compact ppl prmsd | ok masked_last compact_last compact_grid core_grid compact_elsewhere || same
// same: 1 if every other column of every block and of the net plan is what the same query plans with query_row_tiles = 0 (the decision moves nothing else).
#include <cstdio>
#include "../ab_opt_amd/csrc/forward_plan.h"

using namespace abopt;

static bool same_but_compact(const NetPlan& a, const NetPlan& b) {
    if (a.mixer_kernel != b.mixer_kernel || a.mixer_xt != b.mixer_xt || a.heads_kernel != b.heads_kernel || a.heads_epilogue != b.heads_epilogue ||
        a.build_infeat != b.build_infeat || a.prmsd != b.prmsd || a.step_fused != b.step_fused || a.mixer_launch != b.mixer_launch || a.step_carry != b.step_carry ||
        a.enc.ok != b.enc.ok || a.enc.num_blocks != b.enc.num_blocks) return false;
    for (int i = 0; i < a.enc.num_blocks; ++i) {
        const BlockPlan &x = a.enc.blocks[i], &y = b.enc.blocks[i];
        if (x.node != y.node || x.qk_terms != y.qk_terms || x.core.form != y.core.form || x.core.nsplit != y.core.nsplit || x.core.grid != y.core.grid ||
            x.core.remap != y.core.remap || x.tail != y.tail || x.xt_read != y.xt_read || x.xt_write != y.xt_write || x.carry_next != y.carry_next ||
            x.carried != y.carried || x.frag_slot != y.frag_slot || x.query_rows_masked != y.query_rows_masked) return false;
        if (y.query_rows_compact != 0 || y.compact_grid != 0u) return false;          // a query without a list gathers nothing
    }
    return true;
}

int main() {
    const int geo[][2] = {{2, 80}, {3, 48}, {8, 256}, {17, 256}, {24, 256}, {32, 256}, {48, 256}, {64, 256}, {32, 200}, {1000, 48}};
    const int cuss[] = {8, 64, 256, 304};
    const int nbs[] = {1, 2, 3, 6};
    for (const auto& g : geo) for (int cus : cuss) for (int z = 0; z < 2; ++z) for (int terms = 0; terms < 2; ++terms) for (int ovr = -1; ovr <= 1; ++ovr)
        for (int nb : nbs) for (int tiles = 0; tiles <= 10; ++tiles) for (int cu = 0; cu < 2; ++cu) for (int sw = 0; sw < 5; ++sw) {
            ForwardQuery q{};
            q.N = g[0]; q.L = g[1]; q.z_shared = z ? q.N : 0; q.cus = cus;
            q.cache = true; q.terms = terms != 0;
            q.split_ws_floats = ipa_split_ws_floats(q.N, q.L);
            q.split_ws = q.split_ws_floats != 0;
            q.num_blocks = nb;
            for (int i = 0; i < nb; ++i) q.blocks[i] = {true, true, true, true};
            q.mix_frag = q.heads_frag = true;
            q.prmsd = sw == 4;
            q.sw.core32_override = ovr;
            q.sw.step_rows = sw != 1; q.sw.step_compact = sw != 2;
            q.frag2 = true;
            q.step = q.carry_in = q.carry_out = true;
            q.ppl = sw == 3;
            q.context_unused = cu != 0;
            q.query_row_tiles = tiles;
            const NetPlan n = plan_network(q);
            ForwardQuery q0 = q;
            q0.query_row_tiles = 0;
            const NetPlan n0 = plan_network(q0);
            bool elsewhere = false;
            for (int i = 0; i + 1 < n.enc.num_blocks; ++i) elsewhere = elsewhere || n.enc.blocks[i].query_rows_compact || n.enc.blocks[i].compact_grid;
            const BlockPlan& last = n.enc.blocks[n.enc.num_blocks - 1];
            std::printf("%d %d %d %d %d %d %d %d | %d %d %d %d %d | %d %d %d %u %u %d || %d\n", q.N, q.L, q.cus, q.z_shared, q.terms, ovr, nb, tiles, cu, q.sw.step_rows,
                        q.sw.step_compact, q.ppl, q.prmsd, n.enc.ok, last.query_rows_masked, last.query_rows_compact, last.compact_grid, last.core.grid, elsewhere,
                        same_but_compact(n, n0));
        }
    return 0;
}
