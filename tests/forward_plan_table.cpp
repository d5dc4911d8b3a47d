// Tabulates plan_network / plan_encoder / plan_block (ab_opt_amd/csrc/forward_plan.h) over a grid of forwards of a three-block net, one line per query, for
// tests/test_forward_plan.py.  Host C++17 only: no HIP, no device.  Columns:
//   N L cus z_shared cache terms ask ws ovr no_split fuse_tail x_terms fuse_heads wl mix heads prmsd
//   | used ok num_blocks mixer_kernel mixer_xt heads_kernel heads_epilogue build_infeat prmsd
//   | node_kernel qk_terms form nsplit tail xt_read xt_write      (once per planned block of plan_network)
//   | xt_read xt_write ... of plan_encoder's blocks (no mixer in front) | tail xt_read xt_write of plan_block(q, 0) (a block on its own)
// ask: 0 nothing, 1 feat_out, 2 abopt_ga_debug without logits / alpha, 3 with them (the dumping core).  ws: 0 no key-split scratch, 1 what the workspace carves.
// wl: 0 every block packed, 1 every block plain, 2 / 3 / 4 block 0 / 1 / 2 plain.  used: plan_pair_terms_used of the geometry and the switches.
#include <cstdio>
#include "../ab_opt_amd/csrc/forward_plan.h"

using namespace abopt;

int main() {
    const int geo[][2] = {{2, 33}, {3, 70}, {8, 256}, {16, 256}, {32, 256}, {48, 256}, {1000, 48}, {1366, 256}};
    const int cuss[] = {8, 256};
    const int zs[] = {0, 16};
    // {core32_override, no_split, fuse_tail, x_terms, fuse_heads}: the settings the suite runs under
    const Switches sws[] = {{}, {1}, {0}, {-1, true}, {1, true}, {0, true}, {-1, false, false}, {-1, false, true, false}, {-1, false, false, false},
                            {-1, true, false}, {0, true, false}, {1, true, false}, {-1, false, true, true, false}, {1, false, true, false}, {1, false, false, false}};
    const char* forms[] = {"OneBlock", "Persist", "Split", "Core32", "Unsupported"};
    const char* tails[] = {"InCore", "OutLnMlp", "Gemm"};
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
                const NetPlan n = plan_network(q);
                std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d | %d %d %d %d %d %d %d %d %d", N, L, cus, z, cache, terms, ask, ws, sw.core32_override, sw.no_split,
                            sw.fuse_tail, sw.x_terms, sw.fuse_heads, wl, q.mix_frag, q.heads_frag, q.prmsd, plan_pair_terms_used(N, L, z, cus, sw), n.enc.ok, n.enc.num_blocks,
                            n.mixer_kernel, n.mixer_xt, n.heads_kernel, n.heads_epilogue, n.build_infeat, n.prmsd);
                for (int i = 0; i < n.enc.num_blocks; ++i) {
                    const BlockPlan& b = n.enc.blocks[i];
                    std::printf(" | %d %d %s %d %s %d %d", b.node == NodeForm::Kernel, b.qk_terms, forms[(int)b.core.form], b.core.nsplit, tails[(int)b.tail], b.xt_read, b.xt_write);
                }
                const EncoderPlan e = plan_encoder(q);
                std::printf(" |");
                for (int i = 0; i < e.num_blocks; ++i) std::printf(" %d %d", e.blocks[i].xt_read, e.blocks[i].xt_write);
                const BlockPlan s = plan_block(q, 0);
                std::printf(" | %s %d %d\n", tails[(int)s.tail], s.xt_read, s.xt_write);
            }
    }
    return 0;
}
