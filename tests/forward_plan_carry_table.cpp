// Tabulates the carried-fragment decision of plan_network / plan_encoder (ab_opt_amd/csrc/forward_plan.h: carry_next, carried, frag_slot) over the grid of
// tests/forward_plan_table.cpp, for tests/test_forward_plan_carry.py.  Host C++17 only: no HIP, no device.  One line per query of that grid:
//   <the line forward_plan_table prints for the query, from a plan with fuse_node = 1 and frag2 = 1>
//   || fuse_node frag2 same | carry_next carried frag_slot (once per planned block)        three times: (1, 1), (0, 1), (1, 0)
// same: 1 if the columns of forward_plan_table come out the same under this (fuse_node, frag2) as under (1, 1).
// Behind the grid: `pin` lines, the shapes of the GPU test with frag2 from the workspace's fit rule (see main).
#include <cstdio>
#include <string>
#include "../ab_opt_amd/csrc/forward_plan.h"

using namespace abopt;

static std::string legacy_line(const ForwardQuery& q, int ask, int ws, int wl) {
    const char* forms[] = {"OneBlock", "Persist", "Split", "Core32", "Unsupported"};
    const char* tails[] = {"InCore", "OutLnMlp", "Gemm"};
    const Switches& sw = q.sw;
    char buf[512];
    const NetPlan n = plan_network(q);
    std::snprintf(buf, sizeof buf, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d | %d %d %d %d %d %d %d %d %d", q.N, q.L, q.cus, q.z_shared, q.cache, q.terms, ask, ws,
                  sw.core32_override, sw.no_split, sw.fuse_tail, sw.x_terms, sw.fuse_heads, wl, q.mix_frag, q.heads_frag, q.prmsd, plan_pair_terms_used(q.N, q.L, q.z_shared, q.cus, sw),
                  n.enc.ok, n.enc.num_blocks, n.mixer_kernel, n.mixer_xt, n.heads_kernel, n.heads_epilogue, n.build_infeat, n.prmsd);
    std::string s = buf;
    for (int i = 0; i < n.enc.num_blocks; ++i) {
        const BlockPlan& b = n.enc.blocks[i];
        std::snprintf(buf, sizeof buf, " | %d %d %s %d %s %d %d", b.node == NodeForm::Kernel, b.qk_terms, forms[(int)b.core.form], b.core.nsplit, tails[(int)b.tail], b.xt_read, b.xt_write);
        s += buf;
    }
    const EncoderPlan e = plan_encoder(q);
    s += " |";
    for (int i = 0; i < e.num_blocks; ++i) { std::snprintf(buf, sizeof buf, " %d %d", e.blocks[i].xt_read, e.blocks[i].xt_write); s += buf; }
    const BlockPlan b0 = plan_block(q, 0);
    std::snprintf(buf, sizeof buf, " | %s %d %d", tails[(int)b0.tail], b0.xt_read, b0.xt_write);
    // a block on its own never carries
    if (b0.carry_next || b0.carried || b0.frag_slot != 0) return "plan_block carries";
    return s + buf;
}

int main() {
    const int geo[][2] = {{2, 33}, {3, 70}, {8, 256}, {16, 256}, {32, 256}, {48, 256}, {1000, 48}, {1366, 256}};
    const int cuss[] = {8, 256};
    const int zs[] = {0, 16};
    const Switches sws[] = {{}, {1}, {0}, {-1, true}, {1, true}, {0, true}, {-1, false, false}, {-1, false, true, false}, {-1, false, false, false},
                            {-1, true, false}, {0, true, false}, {1, true, false}, {-1, false, true, true, false}, {1, false, true, false}, {1, false, false, false}};
    const bool variants[3][2] = {{true, true}, {false, true}, {true, false}};       // {fuse_node, frag2}
    for (const auto& g : geo) for (int cus : cuss) for (int z : zs) {
        const int N = g[0], L = g[1];
        if (z > 1 && N % z) continue;
        for (int cache = 0; cache < 2; ++cache) for (int terms = 0; terms <= cache; ++terms) for (int ask = 0; ask < 4; ++ask) for (int ws = 0; ws < 2; ++ws)
            for (const Switches& sw : sws) for (int wl = 0; wl < 5; ++wl) for (int net = 0; net < 5; ++net) {
                ForwardQuery q{};
                q.N = N; q.L = L; q.z_shared = z; q.cus = cus;
                q.cache = cache; q.terms = terms; q.feat_out = ask == 1; q.dbg = ask >= 2; q.dump = ask == 3;
                q.split_ws_floats = ws ? ipa_split_ws_floats(N, L) : 0;
                q.split_ws = q.split_ws_floats != 0;
                q.num_blocks = 3;
                for (int i = 0; i < 3; ++i) { const bool packed = wl == 0 || (wl >= 2 && wl - 2 != i); q.blocks[i] = {packed, packed, packed, packed}; }
                q.mix_frag = net == 1 || net == 2; q.heads_frag = net >= 1 && net <= 3; q.prmsd = net >= 2;
                q.sw = sw;
                std::string first;
                for (int v = 0; v < 3; ++v) {
                    q.sw.fuse_node = variants[v][0]; q.frag2 = variants[v][1];
                    const std::string line = legacy_line(q, ask, ws, wl);
                    if (v == 0) { first = line; std::fputs(line.c_str(), stdout); }
                    std::printf(" || %d %d %d |", q.sw.fuse_node, q.frag2, line == first);
                    const NetPlan n = plan_network(q);
                    for (int i = 0; i < n.enc.num_blocks; ++i) std::printf(" %d %d %d", n.enc.blocks[i].carry_next, n.enc.blocks[i].carried, n.enc.blocks[i].frag_slot);
                }
                std::printf("\n");
            }
    }
    // The shapes tests/test_node_carry.py runs (ABOPT_CORE32=1, ABOPT_CORE_NO_SPLIT, cache + pair terms, every operand packed, no prmsd head, 256 CUs), with frag2 from the
    // workspace's own fit rule (plan_frag2_fits over the sizes carve_ga carves: proj [M, 2048] | feat [M, 1824] against the two fragment buffers of ceil(L / 16) row tiles):
    //   pin N L z_shared fits | carry_next carried frag_slot (once per planned block)
    const int pins[][3] = {{2, 33, 0}, {2, 48, 0}, {3, 70, 0}, {8, 64, 0}, {4, 48, 2}, {2, 17, 0}, {2, 19, 0}, {2, 20, 0}, {32, 256, 0}};
    for (const auto& g : pins) {
        const int N = g[0], L = g[1];
        const size_t M = (size_t)N * L, tiles = (size_t)N * ((L + JC - 1) / JC);
        ForwardQuery q{};
        q.N = N; q.L = L; q.z_shared = g[2]; q.cus = 256;
        q.cache = q.terms = true;
        q.split_ws_floats = ipa_split_ws_floats(N, L);
        q.split_ws = q.split_ws_floats != 0;
        q.num_blocks = 3;
        for (int i = 0; i < 3; ++i) q.blocks[i] = {true, true, true, true};
        q.mix_frag = q.heads_frag = true;
        q.sw = Switches{1, true};
        q.frag2 = plan_frag2_fits(M * 2048, M * 1824, tiles * H * 8 * 64 * 4, tiles * H * 4 * 64 * 4);
        const NetPlan n = plan_network(q);
        std::printf("pin %d %d %d %d |", N, L, g[2], q.frag2);
        for (int i = 0; i < n.enc.num_blocks; ++i) std::printf(" %d %d %d", n.enc.blocks[i].carry_next, n.enc.blocks[i].carried, n.enc.blocks[i].frag_slot);
        std::printf("\n");
    }
    return 0;
}
