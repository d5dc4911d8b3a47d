// Fused node projections of a GABlock for CDNA4: the six bias-free nn.Linear of ga.py:54-66 (q | k | v | q_pts | k_pts | v_pts,
// [M,128] x [2016,128]^T), the local -> global map of the three point sets (geometry.py:72-91, ga.py:96-105,129-132), the squared
// point norms, and the re-layout of everything into the MFMA fragment order the IPA core consumes (qfrag / kvfrag, see ipa.hip) --
// in ONE kernel.  The 67 MB projection buffer is never written or re-read.
//
// Weight-stationary: a workgroup owns HALF a head (since round 5; a whole head before).  A head's 168 weight rows, permuted and zero-padded at pack time to 12 tiles of 16 rows
//   tile 0,1: q channels 0..15, 16..31   2,3: k   4,5: q_pts points 0..3, 4..7 as (x, y, z, 0) quadruples  |  6,7: k_pts   8,9: v   10,11: v_pts
// sit in LDS in MFMA operand order (tiles 0..5 or 6..11: 48 KB, loaded once; three 4-wave workgroups per CU -- at the bench shape every wave of the chip
// runs exactly two tasks, where one 12-wave workgroup per CU and head left 24.4 tasks to 12 waves); residues stream through in pairs of 16-row tiles.
//
// Arithmetic (round 5): fp32 x fp32 products on the fp16 matrix pipe with TWO terms per operand (ipa_common.h: split_pair2): h = fp16(x),
// l = fp16(x - h), |x - h - l| <= 2^-22 |x|; the weights are multiplied by a power of two S (max |w| S in [2^14, 2^15), so their low terms
// stay normal), split once at pack time (hip.pack_node_weights) and the sums multiplied by 1 / S (exact) in the epilogue:
//     x w S = h_x l_w + l_x h_w + h_x h_w   [+ l_x l_w, <= 2^-22 relative, dropped]
// three v_mfma_f32_16x16x32_f16 (16 cycles each, K = 32) where the exact-fp32 path needs eight v_mfma_f32_16x16x4_f32 (32 cycles each).
// Rounds 2-4 used three bf16 terms and six products (exact up to 2^-25); the two schemes differ from fp64 by the same amount, the fp32
// accumulation error they share (ipa_common.h).  x is split in registers (6 VALU ops per pair of values).
//
// A task is (32 residues, half of the head's tiles): 6 tiles x 4 k-steps x 2 row tiles x 3 products = 144 MFMAs on 48 accumulator
// registers, with each weight fragment read from LDS once per TWO row tiles (at one row tile per read the kernel would sit exactly on
// the 128 B/clk LDS limit).  Register-only epilogue: with this row order an accumulator tile IS a fragment slot -- lane (residue, kq)
// holds 4 consecutive channels, or (x, y, z, pad) of one point, so the frame transform needs no cross-lane traffic.  The value tiles
// run with the operands swapped (accumulator = [residue 4 kq + r][channel fm]), which is the key-major layout of the aggregation
// operand.
// Traffic per launch at M = 8192: x re-read from L2 (24 x 4 MB), weights 12 x 96 KB, fragments written once (75 MB).
// The task itself (nf_task) lives in node_task.h: the fused block kernel runs it too, as its last phase, for the next block (ipa_core.hip).
#include "ipa_common.h"
#include "kernels.h"
#include "node_task.h"


namespace abopt {

// XT: x arrives as fp16 terms (xt) -- its own instantiation, so that neither path carries the other's registers (one kernel with a run-time switch: 172 instead of
// 144 registers, two waves per SIMD instead of three, 24.4 -> 30.7 us at the bench shape)
template <bool XT>
__global__ __launch_bounds__(NF_WAVES * 64) void node_frags_kernel(const float* __restrict__ x, const unsigned* __restrict__ xt, const float* __restrict__ wfrag, const float* __restrict__ R,
                                                                   const float* __restrict__ t, const float* __restrict__ spatial_coef,
                                                                   float* __restrict__ qfrag, float* __restrict__ kvfrag, int L, int nchunk,
                                                                   int total_tiles, int qk_terms) {
    extern __shared__ __attribute__((aligned(16))) char nf_smem[];
    u32x4* wl = reinterpret_cast<u32x4*>(nf_smem);                             // [12 tiles][4 k-steps][2 terms][64]
    const int h = blockIdx.y >> 1, tid = threadIdx.x, lane = tid & 63, fm = lane & 15, kq = lane >> 4;
    const int half = blockIdx.y & 1;                                           // which six tiles this workgroup owns
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        const u32x4* wg = reinterpret_cast<const u32x4*>(wfrag) + (int64_t)h * NF_HEAD_VEC + half * NF_LDS_VEC;
        static_assert(NF_LDS_VEC % (NF_WAVES * 64) == 0, "weight load loop");
#pragma unroll
        for (int e = 0; e < NF_LDS_VEC / (NF_WAVES * 64); ++e) wl[e * (NF_WAVES * 64) + tid] = wg[e * (NF_WAVES * 64) + tid];
    }
    const float sc = spatial_coef[h];
    const float winv = wfrag[(int64_t)H * NF_HEAD_VEC * 4 + 1];                  // 1 / S behind the packed weights
    const float gamma = (sc > 20.f) ? sc : log1pf(expf(sc));                     // softplus, ga.py:108
    const float ch_ = (-1.f * gamma * 0.16666666666666666f) / 2.f;               // -gamma sqrt(2/(9*8)) / 2, ga.py:109-110
    const float m2c = -2.f * ch_;
    __syncthreads();
    // every workgroup owns a contiguous, equal (+-1) share of the head's tasks (pair of row tiles, half of the tiles); its waves take
    // them round-robin, so both halves of a row-tile pair run on neighbouring waves and share the x rows in L1
    // (a task index is a pair of row tiles, all of this workgroup's tasks are of its own half)
    constexpr NfX XS = XT ? NfX::GlobalTerms : NfX::GlobalF32;
    const int ntask = (total_tiles + 1) / 2;
    const int t_lo = (int)((int64_t)ntask * blockIdx.x / gridDim.x), t_hi = (int)((int64_t)ntask * (blockIdx.x + 1) / gridDim.x);
    for (int task = t_lo + wave; task < t_hi; task += NF_WAVES) {
        const int tile0 = task * 2;
        if (half) nf_task<1, XS, 2>(x, xt, wl, R, t, qfrag, kvfrag, L, nchunk, total_tiles, tile0, h, ch_, m2c, winv, lane, fm, kq, qk_terms);
        else          nf_task<0, XS, 2>(x, xt, wl, R, t, qfrag, kvfrag, L, nchunk, total_tiles, tile0, h, ch_, m2c, winv, lane, fm, kq, qk_terms);
    }
}

size_t node_wfrag_floats() { return (size_t)H * NF_HEAD_VEC * 4 + 4; }      // + {S, 1 / S, 0, 0}

int launch_node_frags(const float* x, const float* wfrag, const float* R, const float* t, const float* spatial_coef, float* qfrag, float* kvfrag,
                      int N, int L, hipStream_t st, int cus, int qk_terms, const float* x_terms) {
    if ((int64_t)N * L == 0) return ABOPT_OK;
    const int nchunk = (L + JC - 1) / JC, total = N * nchunk;
    int rc;
    static LdsConfig lds_cfg[2];
    const bool xt = x_terms != nullptr;
    if ((rc = ensure_dynamic_lds(xt ? reinterpret_cast<const void*>(node_frags_kernel<true>) : reinterpret_cast<const void*>(node_frags_kernel<false>), NF_LDS_VEC * 16,
                                 lds_cfg[xt])))
        return rc;
    // 24 (head, half) columns of workgroups x `groups` shares of the row-tile pairs; 48 KB of LDS each: 3 per CU.  At the bench shape
    // (256 pairs, 256 CUs): 32 groups of 8 pairs, two tasks for each of the four waves -- every wave of the chip does the same amount of work.
    const int ntask = (total + 1) / 2;
    const int groups = max(1, min(cus * 3 / (2 * H), (ntask + NF_WAVES - 1) / NF_WAVES));
    const dim3 grid(groups, 2 * H);
    if (xt)
        hipLaunchKernelGGL(node_frags_kernel<true>, grid, dim3(NF_WAVES * 64), NF_LDS_VEC * 16, st, x, reinterpret_cast<const unsigned*>(x_terms), wfrag, R, t,
                           spatial_coef, qfrag, kvfrag, L, nchunk, total, qk_terms);
    else
        hipLaunchKernelGGL(node_frags_kernel<false>, grid, dim3(NF_WAVES * 64), NF_LDS_VEC * 16, st, x, nullptr, wfrag, R, t, spatial_coef, qfrag, kvfrag, L, nchunk,
                           total, qk_terms);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}

}  // namespace abopt
