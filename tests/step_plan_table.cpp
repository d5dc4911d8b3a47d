// Tabulates the step fields of plan_network (ab_opt_amd/csrc/forward_plan.h: step_fused, mixer_launch, step_carry) for tests/test_step_plan.py, one line per query of
// a three-block net at the bench geometry (N = 32, L = 256, 256 CUs, cache + terms).  Host C++17 only: no HIP, no device.  Columns:
//   fuse_step fuse_heads x_terms mix heads prmsd ppl step carry_in carry_out | step_fused mixer_launch step_carry mixer_kernel mixer_xt heads_kernel heads_epilogue
#include <cstdio>
#include "../ab_opt_amd/csrc/forward_plan.h"

using namespace abopt;

int main() {
    for (int bits = 0; bits < (1 << 10); ++bits) {
        const auto b = [&](int k) { return ((bits >> k) & 1) != 0; };
        ForwardQuery q{};
        q.N = 32; q.L = 256; q.z_shared = 0; q.cus = 256;
        q.cache = true; q.terms = true;
        q.split_ws_floats = ipa_split_ws_floats(q.N, q.L);
        q.split_ws = q.split_ws_floats != 0;
        q.num_blocks = 3;
        for (int i = 0; i < 3; ++i) q.blocks[i] = {true, true, true, true};
        q.sw.fuse_step = b(0); q.sw.fuse_heads = b(1); q.sw.x_terms = b(2);
        q.mix_frag = b(3); q.heads_frag = b(4); q.prmsd = b(5); q.ppl = b(6); q.step = b(7); q.carry_in = b(8); q.carry_out = b(9);
        const NetPlan n = plan_network(q);
        std::printf("%d %d %d %d %d %d %d %d %d %d | %d %d %d %d %d %d %d\n", q.sw.fuse_step, q.sw.fuse_heads, q.sw.x_terms, q.mix_frag, q.heads_frag, q.prmsd, q.ppl, q.step,
                    q.carry_in, q.carry_out, n.step_fused, n.mixer_launch, n.step_carry, n.mixer_kernel, n.mixer_xt, n.heads_kernel, n.heads_epilogue);
    }
    return 0;
}
