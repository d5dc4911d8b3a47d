// One task of the node projections (node_frags.hip has the layout and the arithmetic): 32 residues x half of a head's tiles -> their q / k / v fragment slots.
// Shared by the stand-alone kernel (node_frags.hip: node_frags_kernel -- weights in LDS, x or its fp16 terms from global memory) and by the last phase of the
// fused block kernel (ipa_core.hip: ipa_core32_kernel<true, *, true> -- the NEXT block's weights streamed from L2, x terms in LDS), the way tail_common.h serves the
// two tails.  Both run the SAME arithmetic in the SAME order per output element: the MFMA order l wH, h wL, h wH per (k-step, tile), the 1 / S scaling, and an
// epilogue whose every product and sum is spelled out (fmaf / nf_mul_rn under fp contract(off)) -- left to the compiler, the contraction of a * b + c * d + ...
// follows the operand order of the optimised IR and has differed between two kernels compiled from one function (DESIGN_LOG.md, "After round 6").  The spelling
// is what hipcc made of the plain expressions in node_frags_kernel before the task was shared, read from its disassembly (the kernel's floating-point
// instructions are the same, count for count).
#pragma once
#include "ipa_common.h"

namespace abopt {

constexpr int NF_F = 128;                                       // node feature width (ga.py:54-66 with node_feat_dim = 128)
// A workgroup owns HALF a head (six tiles, 48 KB of LDS), three 4-wave workgroups per CU (round 5; a whole head in 96 KB, one 12-wave workgroup
// per CU before -- see the header of node_frags.hip).
constexpr int NF_TILES = 12, NF_HT = NF_TILES / 2, NF_WAVES = 4;       // 12 waves per CU = 3 per SIMD (152 VGPRs): the task epilogues of one wave hide behind the MFMAs of two others (8 -> 12 waves: 35.8 -> 34.9 us at M = 8192, 205 -> 188 us at M = 48000, same box)
constexpr int NF_KS = NF_F / 32, NF_SPL = 2;                // k-steps of 32, fp16 terms per fp32 value
constexpr int NF_HEAD_VEC = NF_TILES * NF_KS * NF_SPL * 64;    // 16-byte vectors (8 fp16) per head: [tile][k-step][term][lane]
constexpr int NF_LDS_VEC = NF_HEAD_VEC / 2;                    // what a workgroup keeps in LDS: half a head

__device__ __forceinline__ float quad_bcast0(float v) { return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x00, 0xf, 0xf, false)); }
__device__ __forceinline__ float quad_bcast1(float v) { return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x55, 0xf, 0xf, false)); }
__device__ __forceinline__ float quad_bcast2(float v) { return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0xAA, 0xf, 0xf, false)); }

// One task: tiles [HALF * 6, HALF * 6 + 6) of head h for the row tiles tile0, tile0 + 1.
// Where x comes from: fp32 rows in global memory (split here) | their fp16 terms in global memory ([row][64 words high | 64 words low]) | the terms of the
// workgroup's own 32 rows in an LDS tile of the same row layout with a padded stride (NF_XLDS_STRIDE words; row = residue - xrow0)
enum class NfX { GlobalF32, GlobalTerms, LdsTerms };
constexpr int NF_XLDS_STRIDE = NF_F + 4;                         // 528 bytes: the 16 rows of a 16-byte request 4 banks apart (512 would put them on one bank)
typedef const __attribute__((address_space(3))) unsigned* NfLdsTerms;
typedef const __attribute__((address_space(3))) u32x4* NfLdsVec;
// a product the compiler may not contract with a neighbouring sum
__device__ __forceinline__ float nf_mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
// WD: weight fragments of step g + WD - 1 are requested before the 12 MFMAs of step g are issued (a ring of WD slots of 8 registers).  2 for weights in LDS;
// streamed from L2 (~750 clk) the fused phase keeps 8 steps ahead.
template <int HALF, NfX XS, int WD, class XP, class WP>
__device__ __forceinline__ void nf_task(const float* __restrict__ x, XP xt, WP wl, const float* __restrict__ R, const float* __restrict__ t,
                                        float* __restrict__ qfrag, float* __restrict__ kvfrag, int L, int nchunk, int total_tiles, int tile0, int h,
                                        float ch_, float m2c, float winv, int lane, int fm, int kq, int qk_terms, int xrow0 = 0) {
    constexpr bool XT = XS != NfX::GlobalF32;
    constexpr int XLD_ = XS == NfX::LdsTerms ? NF_XLDS_STRIDE : NF_F;
    int64_t rowbase[2], row[2];
    int cbs[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int tile = min(tile0 + rt, total_tiles - 1);                       // odd tile count: the last task computes its last tile twice, stores once
        const int n = tile / nchunk;
        cbs[rt] = tile % nchunk;
        rowbase[rt] = (int64_t)n * L;
        row[rt] = rowbase[rt] + min(cbs[rt] * JC + fm, L - 1);                   // rows past the end: clamped copies (finite; the core never stores them)
    }
    auto xvec = [&](int rt, int word) {
        if constexpr (XS == NfX::LdsTerms) return *reinterpret_cast<NfLdsVec>(xt + (min(cbs[rt] * JC + fm, L - 1) - xrow0) * XLD_ + word);
        else return *reinterpret_cast<const u32x4*>(xt + row[rt] * XLD_ + word);
    };
    // lane (row fm, kq) holds k = 32 s + 8 kq + i of its row for k-step s -- as fp32 (split here) or, when the kernel that produced x also wrote its terms
    // (xt: [row][64 words of high terms | 64 words of low terms]), as the two 16-byte term vectors themselves
    f32x4 xa[2][2];
    Split2 xn[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        if constexpr (XT) {
            xn[rt].h = xvec(rt, kq * 4);
            xn[rt].l = xvec(rt, 64 + kq * 4);
        } else {
            xa[rt][0] = *reinterpret_cast<const f32x4*>(x + row[rt] * NF_F + kq * 8);
            xa[rt][1] = *reinterpret_cast<const f32x4*>(x + row[rt] * NF_F + kq * 8 + 4);
        }
    }
    f32x4 acc[2][NF_HT];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int T = 0; T < NF_HT; ++T) acc[rt][T] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const auto wh = wl + lane;
    // weight fragments of step g + WD - 1 are requested before the 12 MFMAs of step g are issued (hipcc left to itself hoists every read)
    static_assert(WD >= 2 && WD <= NF_KS * NF_HT, "weight ring");
    u32x4 wa[WD][NF_SPL];
    auto wfrag_at = [&](int g_, int sp) { return wh[(((g_ % NF_HT) * NF_KS + g_ / NF_HT) * NF_SPL + sp) * 64]; };
#pragma unroll
    for (int g = 0; g < WD - 1; ++g)
#pragma unroll
        for (int sp = 0; sp < NF_SPL; ++sp) wa[g][sp] = wfrag_at(g, sp);
    Split2 xs[2];
#pragma unroll
    for (int g = 0; g < NF_KS * NF_HT; ++g) {
        const int s = g / NF_HT, T = g % NF_HT;
        if (T == 0) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                if constexpr (XT) xs[rt] = xn[rt];
                else xs[rt] = split2(xa[rt][0], xa[rt][1]);
            }
            if (s + 1 < NF_KS) {
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    if constexpr (XT) {
                        xn[rt].h = xvec(rt, (s + 1) * 16 + kq * 4);
                        xn[rt].l = xvec(rt, 64 + (s + 1) * 16 + kq * 4);
                    } else {
                        xa[rt][0] = *reinterpret_cast<const f32x4*>(x + row[rt] * NF_F + (s + 1) * 32 + kq * 8);
                        xa[rt][1] = *reinterpret_cast<const f32x4*>(x + row[rt] * NF_F + (s + 1) * 32 + kq * 8 + 4);
                    }
                }
            }
        }
        if (g + WD - 1 < NF_KS * NF_HT) {
#pragma unroll
            for (int sp = 0; sp < NF_SPL; ++sp) wa[(g + WD - 1) % WD][sp] = wfrag_at(g + WD - 1, sp);
        }
        const u32x4 wH = wa[g % WD][0], wL = wa[g % WD][1];
        const bool swap = (HALF == 1) && (T >= 2);                               // value tiles: x is the A operand -> accumulator [residue 4 kq + r][channel fm]
        // smallest terms first; the two row tiles alternate so consecutive MFMAs never depend on each other
#define NF_PROD(XT, WT)                                                                                                         \
        if (swap) { acc[0][T] = mfma_h(xs[0].XT, WT, acc[0][T]); acc[1][T] = mfma_h(xs[1].XT, WT, acc[1][T]); }               \
        else      { acc[0][T] = mfma_h(WT, xs[0].XT, acc[0][T]); acc[1][T] = mfma_h(WT, xs[1].XT, acc[1][T]); }
        NF_PROD(l, wH) NF_PROD(h, wL) NF_PROD(h, wH)
#undef NF_PROD
        __builtin_amdgcn_sched_barrier(0);
    }
    auto sq = [](const f32x4& g) { return fmaf(g[2], g[2], fmaf(g[1], g[1], g[0] * g[0])); };
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        if (tile0 + rt >= total_tiles) break;
        const int tile = tile0 + rt;
#pragma unroll
        for (int T = 0; T < NF_HT; ++T) acc[rt][T] *= winv;                      // sums of S w x -> w x (exact)
        // frames are fetched only now: x fragments and weight registers are dead
        float Rm[9], tv[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rm[k] = R[row[rt] * 9 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tv[k] = t[row[rt] * 3 + k];
        // p <- R p + t (geometry.py:72-91) on (x, y, z, pad) of one point of residue fm
        // (a b + c d + e f) + t as hipcc contracts it: fma(e, f, fma(a, b, c d)) + t
        auto dot3 = [](float a, float b, float c, float d, float e, float f, float t_) { return fmaf(e, f, fmaf(a, b, nf_mul_rn(c, d))) + t_; };
        auto to_global = [&](const f32x4& p) {
            return (f32x4){dot3(Rm[0], p[0], Rm[1], p[1], Rm[2], p[2], tv[0]), dot3(Rm[3], p[0], Rm[4], p[1], Rm[5], p[2], tv[1]),
                           dot3(Rm[6], p[0], Rm[7], p[1], Rm[8], p[2], tv[2]), 0.f};
        };
        f32x4* outq = reinterpret_cast<f32x4*>(qfrag) + ((int64_t)tile * H + h) * (4 * 64) + lane;
        f32x4* outk = reinterpret_cast<f32x4*>(kvfrag) + ((int64_t)tile * H + h) * (8 * 64) + lane;
        if (HALF == 0) {
            // ---- q, k: accumulator row 4 kq + r = channel, column fm = residue
            const float s = 0.17677669529663687f;                                // 1 / sqrt(D), ga.py:84
            if (qk_terms) {
                // round 6: the consumer (ipa_core32_kernel<*, true>) multiplies the 32 channels of q / sqrt(D) and k as two fp16 terms each -- slot 0 holds the high
                // terms, slot 1 the low terms; K slot e of lane (residue fm, kq) is channel 4 kq + e (e < 4) or 16 + 4 kq + e - 4: the same map on both sides
                // (channels 0..15: the low term is the rounded product minus its high term; channels 16..31: hipcc contracted product and difference into
                // one fma, fp16 high term as the addend -- v_fma_mix_f32; both are kept)
                const f32x4 q0 = (f32x4){nf_mul_rn(acc[rt][0][0], s), nf_mul_rn(acc[rt][0][1], s), nf_mul_rn(acc[rt][0][2], s), nf_mul_rn(acc[rt][0][3], s)};
                const f32x4 q1 = (f32x4){nf_mul_rn(acc[rt][1][0], s), nf_mul_rn(acc[rt][1][1], s), nf_mul_rn(acc[rt][1][2], s), nf_mul_rn(acc[rt][1][3], s)};
                Split2 tq;
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    unsigned hw, lw;
                    split_pair2(q0[2 * p], q0[2 * p + 1], hw, lw);
                    tq.h[p] = hw; tq.l[p] = lw;
                    hw = pk_f16(q1[2 * p], q1[2 * p + 1]);
                    tq.h[2 + p] = hw;
                    tq.l[2 + p] = pk_f16(fmaf(acc[rt][1][2 * p], s, -f16lo_f32(hw)), fmaf(acc[rt][1][2 * p + 1], s, -f16hi_f32(hw)));
                }
                const Split2 tk = split2(acc[rt][2], acc[rt][3]);
                outq[0] = __builtin_bit_cast(f32x4, tq.h); outq[64] = __builtin_bit_cast(f32x4, tq.l);
                outk[0] = __builtin_bit_cast(f32x4, tk.h); outk[64] = __builtin_bit_cast(f32x4, tk.l);
            } else {
            outq[0] = acc[rt][0] * s; outq[64] = acc[rt][1] * s;
            outk[0] = acc[rt][2]; outk[64] = acc[rt][3];
            }
            // ---- q_pts: point kq (tile A) and 4 + kq (tile B) of residue fm
            f32x4 ga = to_global(acc[rt][4]), gb = to_global(acc[rt][5]);
            const float nq = rows_sum(sq(ga) + sq(gb));                          // |q_pts|^2 over the head's 8 points
            ga *= m2c; gb *= m2c;
            ga[3] = kq == 0 ? ch_ * nq : (kq == 1 ? ch_ : 0.f);                  // norm step, q side
            gb[3] = 0.f;
            outq[128] = ga; outq[192] = gb;
        } else {
            // ---- k_pts
            f32x4 ga = to_global(acc[rt][0]), gb = to_global(acc[rt][1]);
            const float nk = rows_sum(sq(ga) + sq(gb));
            ga[3] = kq == 0 ? 1.f : (kq == 1 ? nk : 0.f);                        // norm step, k side
            outk[128] = ga; outk[192] = gb;
            // ---- v, v_pts: accumulator row 4 kq + r = residue, column fm = channel / (point fm >> 2, coordinate fm & 3)
            const int c = fm & 3, cr = min(c, 2);                                // row cr of R and t[cr] of residue 4 kq + r
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t rr = rowbase[rt] + min(cbs[rt] * JC + kq * 4 + r, L - 1);
                const float r0 = R[rr * 9 + cr * 3], r1 = R[rr * 9 + cr * 3 + 1], r2 = R[rr * 9 + cr * 3 + 2], r3 = t[rr * 3 + cr];
                const float xa_ = quad_bcast0(acc[rt][4][r]), ya = quad_bcast1(acc[rt][4][r]), za = quad_bcast2(acc[rt][4][r]);
                const float xb = quad_bcast0(acc[rt][5][r]), yb = quad_bcast1(acc[rt][5][r]), zb = quad_bcast2(acc[rt][5][r]);
                float g0 = dot3(r0, xa_, r1, ya, r2, za, r3);
                float g1 = dot3(r0, xb, r1, yb, r2, zb, r3);
                if (c == 3) { g0 = 0.f; g1 = 0.f; }
                outk[(4 + r) * 64] = (f32x4){acc[rt][2][r], acc[rt][3][r], g0, g1};
            }
        }
    }
}

}  // namespace abopt
