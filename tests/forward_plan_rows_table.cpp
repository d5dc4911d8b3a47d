// Tabulates the masked-query-rows decision of plan_network / plan_encoder (ab_opt_amd/csrc/forward_plan.h: query_rows_masked) for tests/test_forward_plan_rows.py.
// Host C++17 only: no HIP, no device.  A three-block net with a cache over geometries, CU counts, core overrides and weight lists; one line per query:
//   N L cus z cache terms ovr wl mix heads prmsd | entry ppl context_unused fuse_step fuse_heads fuse_tail step_rows fuse_node dbg | step_fused ok num_blocks |
//   <node_kernel core tail carry_next carried frag_slot xt_read xt_write qk_terms query_rows_masked> once per planned block || same
// entry: 0 abopt_eps_net_forward (step = 0), 1 abopt_eps_net_step.  same: 1 if every other column of every block and of the net plan is what the same query plans
// with context_unused = 0 (the decision is additive: it moves nothing else).
#include <cstdio>
#include "../ab_opt_amd/csrc/forward_plan.h"

using namespace abopt;

static bool same_but_rows(const NetPlan& a, const NetPlan& b) {
    if (a.mixer_kernel != b.mixer_kernel || a.mixer_xt != b.mixer_xt || a.heads_kernel != b.heads_kernel || a.heads_epilogue != b.heads_epilogue ||
        a.build_infeat != b.build_infeat || a.prmsd != b.prmsd || a.step_fused != b.step_fused || a.mixer_launch != b.mixer_launch || a.step_carry != b.step_carry ||
        a.enc.ok != b.enc.ok || a.enc.num_blocks != b.enc.num_blocks) return false;
    for (int i = 0; i < a.enc.num_blocks; ++i) {
        const BlockPlan &x = a.enc.blocks[i], &y = b.enc.blocks[i];
        if (x.node != y.node || x.qk_terms != y.qk_terms || x.core.form != y.core.form || x.core.nsplit != y.core.nsplit || x.core.grid != y.core.grid ||
            x.core.remap != y.core.remap || x.tail != y.tail || x.xt_read != y.xt_read || x.xt_write != y.xt_write || x.carry_next != y.carry_next ||
            x.carried != y.carried || x.frag_slot != y.frag_slot) return false;
    }
    return true;
}

int main() {
    const char* forms[] = {"OneBlock", "Persist", "Split", "Core32", "Unsupported"};
    const char* tails[] = {"InCore", "OutLnMlp", "Gemm"};
    const int geo[][2] = {{2, 80}, {3, 64}, {8, 256}, {32, 256}, {48, 256}, {1000, 48}};
    const int cuss[] = {8, 256};
    const int zs[] = {0, 1};                                               // distinct pair features | one entry for the whole batch (z_shared = N)
    for (const auto& g : geo) for (int cus : cuss) for (int z : zs) for (int cache = 0; cache < 2; ++cache) for (int terms = 0; terms <= cache; ++terms)
        for (int ovr = -1; ovr <= 1; ++ovr) for (int wl = 0; wl < 5; ++wl) for (int net = 0; net < 4; ++net)
            for (int entry = 0; entry < 2; ++entry) for (int ppl = 0; ppl <= entry; ++ppl) for (int cu = 0; cu < 2; ++cu)
                for (int sws = 0; sws < 6; ++sws) for (int dbg = 0; dbg < 2; ++dbg) {
                    if (dbg && (entry || sws)) continue;                   // (a debugging forward is abopt_ga_block_forward's: once per query is enough)
                    ForwardQuery q{};
                    q.N = g[0]; q.L = g[1]; q.z_shared = z ? q.N : 0; q.cus = cus;
                    q.cache = cache; q.terms = terms;
                    q.split_ws_floats = ipa_split_ws_floats(q.N, q.L);
                    q.split_ws = q.split_ws_floats != 0;
                    q.num_blocks = 3;
                    for (int i = 0; i < 3; ++i) { const bool packed = wl == 0 || (wl >= 2 && wl - 2 != i); q.blocks[i] = {packed, packed, packed, packed}; }
                    q.mix_frag = net == 0 || net == 3; q.heads_frag = net <= 1 || net == 3; q.prmsd = net == 3;
                    q.sw.core32_override = ovr;
                    q.sw.fuse_step = sws != 1; q.sw.fuse_heads = sws != 2; q.sw.fuse_tail = sws != 3; q.sw.step_rows = sws != 4; q.sw.fuse_node = sws != 5;
                    q.frag2 = true;
                    q.dbg = dbg != 0;
                    q.step = entry != 0; q.ppl = ppl != 0; q.carry_in = q.carry_out = q.step;
                    q.context_unused = cu != 0;
                    const NetPlan n = plan_network(q);
                    ForwardQuery q0 = q;
                    q0.context_unused = false;
                    const NetPlan n0 = plan_network(q0);
                    bool none0 = true;
                    for (int i = 0; i < n0.enc.num_blocks; ++i) none0 = none0 && !n0.enc.blocks[i].query_rows_masked;
                    std::printf("%d %d %d %d %d %d %d %d %d %d %d | %d %d %d %d %d %d %d %d %d | %d %d %d |", q.N, q.L, q.cus, q.z_shared, q.cache, q.terms, ovr, wl, q.mix_frag,
                                q.heads_frag, q.prmsd, entry, ppl, cu, q.sw.fuse_step, q.sw.fuse_heads, q.sw.fuse_tail, q.sw.step_rows, q.sw.fuse_node, dbg, n.step_fused, n.enc.ok,
                                n.enc.num_blocks);
                    for (int i = 0; i < n.enc.num_blocks; ++i) {
                        const BlockPlan& b = n.enc.blocks[i];
                        std::printf(" %d %s %s %d %d %d %d %d %d %d", b.node == NodeForm::Kernel, forms[(int)b.core.form], tails[(int)b.tail], b.carry_next, b.carried,
                                    b.frag_slot, b.xt_read, b.xt_write, b.qk_terms, b.query_rows_masked);
                    }
                    // a block or an encoder on its own (abopt_ga_block_forward*, abopt_ga_encoder_forward) never masks: they are no steps
                    ForwardQuery qe = q;
                    qe.step = false;
                    const EncoderPlan e = plan_encoder(qe);
                    bool lone = plan_block(q, 2).query_rows_masked;
                    for (int i = 0; i < e.num_blocks; ++i) lone = lone || e.blocks[i].query_rows_masked;
                    std::printf(" || %d\n", same_but_rows(n, n0) && none0 && !lone);
                }
    return 0;
}
