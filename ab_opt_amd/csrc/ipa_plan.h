// Which form of the IPA core runs for a launch geometry: the ONE place that decides (ipa_core.hip launches from the plan; api.hip asks through
// ipa_core32_applies).  Plain host C++17, no HIP: tests/ipa_plan_table.cpp tabulates plan_ipa_core without a device (tests/test_ipa_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/abopt.h"

namespace abopt {

constexpr int H = ABOPT_HEADS, D = ABOPT_QK_DIM, P = ABOPT_POINTS, C = 64;
constexpr int BI = 16;            // query rows per workgroup
constexpr int JC = 16;            // key rows per chunk
constexpr int BI2 = 32;           // query rows per workgroup of the 32-row kernels
constexpr int SPLIT_ROW = H * C + H * D + H * P * 3;   // 1440 unnormalised accumulators per row and key slice

struct CoreQuery {
    int N, L, z_shared, cus;        // cus: CUs of the device (read only with a cache and without a dump)
    bool cache, dump;               // a pair-bias cache is given; the logits dump is asked for
    bool split_ws;                  // the caller holds scratch for the key-split form, of
    size_t split_ws_floats;         // ... this many floats
    int core32_override;            // ABOPT_CORE32: -1 unset, 0, 1
    bool no_split;                  // ABOPT_CORE_NO_SPLIT
};
enum class CoreForm { OneBlock, Persist, Split, Core32, Unsupported };
struct CorePlan {
    CoreForm form;
    int nsplit;                     // key slices per query block (1 unless Split)
    int remap;                      // block -> (sample, query block) mapping: core32_remap for Core32, N % 8 == 0 for the 16-row kernels
    unsigned grid;                  // workgroups of the (first) launch
};

// scratch of the key-split form (small batches)
inline size_t ipa_split_ws_floats(int N, int L) {
    const int nib = (L + BI - 1) / BI;
    return ((int64_t)N * nib * 2 <= 256) ? (size_t)4 * N * L * (SPLIT_ROW + 2 * H) : 0;
}

// block -> (sample, query block) mapping of the 32-row kernels: 2 = by complex (groups of z_shared samples, a multiple of 8 complexes),
// 1 = all query blocks of a sample on one XCD (N % 8 == 0), 0 = plain
inline int core32_remap(int N, int z_shared) {
    if (z_shared > 1 && z_shared < N && N % z_shared == 0 && (N / z_shared) % 8 == 0) return 2;
    return (N % 8 == 0) ? 1 : 0;
}
// Whether 32-bit byte offsets reach every element of one layer's chunk-major slab of the bias cache (distinct samples x L rows x chunks x 768 bytes < 4 GB: up to 1365
// distinct samples at L = 256).  Beyond it only ipa_core_persist_kernel and ipa_core_kernel<false, true, false> run, whose offsets are 64 bits wide.
inline bool bias_slab_fits_u32(int N, int L, int z_shared = 0) {
    return (int64_t)(z_shared > 1 ? N / z_shared : N) * L * ((L + JC - 1) / JC) * (H * JC * 4) < (1ll << 32);
}

// The 32-row kernel runs one block per workgroup, so it pays where its N * ceil(L / 32) workgroups fill the CUs in whole rounds
// (tools/r03_c32_sweep.sh, r03_c32_sweep2.sh; microseconds per launch against the 16-row kernels on the same box):
//   one round, more than half full, where the 16-row blocks no longer fit one round themselves (N L / 16 > CUs: the persistent kernel
//   then walks two blocks per CU):  N = 23 / 24 / 28 / 32 at L = 256: 145 / 145 / 154 / 167 against 156 / 155 / 168 / 175; N = 32,
//   L = 200: 123 against 132.  Up to N L / 16 = CUs the one-block 16-row kernel is the faster one (N = 16: 90 against 124).
//   several rounds at least 95 % full:  N = 62 / 64: 334 / 335 against 344 / 345.  A half-empty last round loses (N = 48: 288 against
//   259; N = 20, L = 400: 385 against 258).
//   short lengths gain nothing (L = 128: equal; L = 64: 134 against 128).
// ABOPT_CORE32=0 / 1 overrides (1: whenever 16 < L <= 2048).
inline bool core32_pays(int N, int L, int cus, int core32_override) {
    if (core32_override == 0) return false;
    if (core32_override == 1) return L > BI;
    if (cus < 8) return false;
    const int64_t total = (int64_t)N * ((L + BI2 - 1) / BI2), rounds = (total + cus - 1) / cus;
    // short crops (pose sampling: N = 1000 x L = 48): since the epilogue runs on two fp16 terms (round 5) the fused 32-row kernel wins wherever it fills
    // the chip once -- 4.10 -> 3.80 ms per step at N = 1000 x L = 48, 3.60 -> 2.88 at 600 x 64, 0.95 -> 0.81 at 64 x 128; it loses below one workgroup
    // per CU (32 x 128: 0.64 -> 0.72).  Rounds 3-4 had excluded L < 192 (three key chunks did not amortise a 40 us epilogue).
    if (L < 192) return L > BI && total >= cus;
    if (rounds == 1) return total * 100 >= (int64_t)cus * 53 && (int64_t)N * ((L + BI - 1) / BI) > cus;
    return total * 100 >= rounds * cus * 95;
}

// The forms in their order of preference.  The two 32-bit reach limits are stated here and nowhere else:
//   slab_u32  the logits-dumping, the key-split and the 32-row kernels address a layer's slab of the bias cache with 32-bit offsets (the 32-row kernels through
//             ONE buffer descriptor per block); the persistent and the plain one-block kernel carry 64-bit offsets
//   L <= 2048 the 32-row kernels' buffer descriptors address a sample's z slab (L^2 * 256 bytes) with 32-bit offsets
inline CorePlan plan_ipa_core(const CoreQuery& q) {
    const int N = q.N, L = q.L;
    const int64_t nib = (L + BI - 1) / BI, nib2 = (L + BI2 - 1) / BI2, nchunk = (L + JC - 1) / JC, total = N * nib;
    const int remap16 = (N % 8 == 0) ? 1 : 0;
    const bool slab_u32 = bias_slab_fits_u32(N, L, q.z_shared);
    if (q.dump && q.cache && !slab_u32) return {CoreForm::Unsupported, 1, 0, 0u};
    if (q.cache && !q.dump) {
        if (L <= 2048 && slab_u32 && core32_pays(N, L, q.cus, q.core32_override))
            return {CoreForm::Core32, 1, core32_remap(N, q.z_shared), (unsigned)(N * nib2)};
        // more query blocks than CUs: one workgroup per CU walks its blocks
        const int pcus = q.cus & ~7;                                        // a multiple of 8 keeps blockIdx & 7 = XCD for every block of a workgroup
        if (nchunk >= 2 && pcus >= 8 && total > pcus) return {CoreForm::Persist, 1, remap16, (unsigned)pcus};
        // small batches: split the keys of every query block over 2 or 4 workgroups (see the SPLIT note at ipa_core_kernel)
        if (q.split_ws && !q.no_split && slab_u32) {
            const int nsplit = (total * 4 <= q.cus && nchunk >= 8) ? 4 : ((total * 2 <= q.cus && nchunk >= 4) ? 2 : 1);
            if (nsplit > 1 && (size_t)nsplit * ((int64_t)N * L) * (SPLIT_ROW + 2 * H) <= q.split_ws_floats)
                return {CoreForm::Split, nsplit, remap16, (unsigned)(total * nsplit)};
        }
    }
    return {CoreForm::OneBlock, 1, remap16, (unsigned)total};     // cached, uncached and dumping variants (launch_core_variant)
}

// What ipa_core32_applies answers: whether the cached, non-dumping launch of this geometry takes the 32-row kernels -- whatever scratch the caller holds
inline bool plan_is_core32(CoreQuery q) {
    q.cache = true; q.dump = false;
    return plan_ipa_core(q).form == CoreForm::Core32;
}

}  // namespace abopt
