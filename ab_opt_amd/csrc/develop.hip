// Developability of designed candidates on the device: what the designed SEQUENCE is, chemically, and where it lies on the surface.
// Two entry points, one launch each, nothing allocated, nothing synchronised, no memset node, every output written whole by plain stores:
//   abopt_sequence_liabilities_grouped  motif windows of a sequence (N-glycosylation sequons, deamidation, isomerisation, cleavage, Cys, Met, hydrophobic runs),
//                                       the charged residues and the hydropathy of the scored rows -- integers only;
//   abopt_surface_patches_grouped       per residue, the sum of hydrophobicity x exposed area over the residues within a radius -- the "spatial aggregation
//                                       propensity" family of scores, fp32 with every step rounded once and the additions in ascending residue order.
// Nothing in the reference is matched; the definitions are this library's own (include/abopt.h) and numpy restates them bit for bit
// (tests/developability_statement.py).
#include <math.h>
#include <algorithm>
#include "abopt_common.h"
#include "candidate_common.h"

// The multiply and the add of a patch are rounded once each and must not be fused (section 6.6, "Every step rounded once": __fmul_rn / __fadd_rn carry the
// permission to contract with them).  So they are spelled dv_mul / dv_add below, compiled under contract(off); d2_fma of candidate_common.h, included BEFORE the
// pragma, is an explicit fmaf chain and means the same on either side of it.
#pragma clang fp contract(off)

namespace abopt {

// ---------------------------------------------------------------- sequence liabilities
constexpr int LB_T = 256;                  // positions of a tile = threads of a workgroup
constexpr int LB_HALO = 15;                // the widest window reaches 15 positions past its anchor (run_min <= 16)
constexpr int LB_COUNTS = 13;              // columns of `counts`
constexpr int LB_RUN_MAX = 16;
// residue types, model.AA_LETTERS = 'ACDEFGHIKLMNPQRSTVWY'
enum : int { AA_C = 1, AA_D = 2, AA_E = 3, AA_G = 5, AA_H = 6, AA_K = 8, AA_M = 10, AA_N = 11, AA_P = 12, AA_R = 14, AA_S = 15, AA_T = 16 };
constexpr unsigned LB_HYDROPHOBIC = (1u << 4) | (1u << 7) | (1u << 9) | (1u << 10) | (1u << 17) | (1u << 18) | (1u << 19);      // F, I, L, M, V, W, Y
// the info byte of a position: bit 0 the byte is a type (< 20), bit 1 the type is hydrophobic, bit 2 the position is a scored row, bit 3 it is linked to the next
enum : int { LB_TYPE = 1, LB_HYD = 2, LB_ROW = 4, LB_LINK = 8 };

// ten times the Kyte-Doolittle hydropathy of type t < 20; 0 for every other byte
__device__ __forceinline__ int lb_hyd10(int t) {
    constexpr int8_t kd[20] = {18, 25, -35, -35, 28, -4, -32, 45, -39, 38, 19, -35, -16, -35, -45, -8, -7, 42, -9, -13};
    return t < 20 ? kd[t] : 0;
}

// rows == NULL: every position is scored; link == NULL: every step is bonded
__device__ __forceinline__ int lb_rowlink(const uint8_t* __restrict__ rows, const uint8_t* __restrict__ link, int64_t p) {
    return ((rows == nullptr || rows[p]) ? LB_ROW : 0) | ((link == nullptr || link[p]) ? LB_LINK : 0);
}

// position p of a sequence of n bytes into slot i of the tile: a position past the end is "no type, no row, no link", so no window reaches over it
__device__ __forceinline__ void lb_put(uint8_t* typ, uint8_t* info, int i, const uint8_t* __restrict__ seq, int64_t p, int n, int rowlink) {
    int t = 255, f = 0;
    if (p < n) {
        t = seq[p];
        f = rowlink | (t < 20 ? LB_TYPE | (((LB_HYDROPHOBIC >> t) & 1u) ? LB_HYD : 0) : 0);
    }
    typ[i] = (uint8_t)t;
    info[i] = (uint8_t)f;
}

// The flag byte of the anchor in slot i (< LB_T) of a staged tile.  A window of width w exists iff all of its bytes are types and all of its w - 1 steps are linked
// (a position past the end is no type); it counts iff one of its positions is a scored row.
__device__ __forceinline__ int lb_flag(const uint8_t* typ, const uint8_t* info, int i, int run_min) {
    const int t0 = typ[i], t1 = typ[i + 1], t2 = typ[i + 2];
    const int i0 = info[i], i1 = info[i + 1], i2 = info[i + 2];
    const int a2 = i0 & i1, o2 = i0 | i1, a3 = a2 & i2, o3 = o2 | i2;
    const bool c1 = (i0 & LB_TYPE) && (i0 & LB_ROW);
    const bool c2 = (a2 & LB_TYPE) && (i0 & LB_LINK) && (o2 & LB_ROW);
    const bool c3 = (a3 & LB_TYPE) && (a2 & LB_LINK) && (o3 & LB_ROW);
    int f = 0;
    if (c3 && t0 == AA_N && t1 != AA_P && (t2 == AA_S || t2 == AA_T)) f |= 1;
    if (c2 && t0 == AA_N && (t1 == AA_G || t1 == AA_S)) f |= 2;
    if (c2 && t0 == AA_D && (t1 == AA_G || t1 == AA_S)) f |= 4;
    if (c2 && t0 == AA_D && t1 == AA_P) f |= 8;
    if (c1 && t0 == AA_C) f |= 16;
    if (c1 && t0 == AA_M) f |= 32;
    if (run_min) {
        int all = LB_TYPE | LB_HYD, steps = LB_LINK, any = 0;
        for (int w = 0; w < run_min; ++w) {
            const int v = info[i + w];
            all &= v;
            any |= v;
            if (w < run_min - 1) steps &= v;
        }
        if (all == (LB_TYPE | LB_HYD) && steps && (any & LB_ROW)) f |= 64;
    }
    return f;
}

// Grid folded over x and y, 4 waves.  Workgroup b < N owns design b: it walks the sequence in tiles of 256 positions (+ 15 of halo) staged in LDS as a type byte
// and an info byte, a thread per anchor; flags leave by plain stores, the 13 counters are kept per thread, reduced by one butterfly per counter and summed over
// the four waves by thread t < 13, which stores counts[b][t].  Workgroup N + (group, tile) -- launched only when freq is wanted -- owns 256 positions of a
// group: it stages the same tile of each of the group's S designs in turn and counts, per anchor, the designs whose flag byte is not zero; freq leaves by plain
// stores.  So the flags are computed twice when freq is asked for and nothing is accumulated across workgroups: no atomic, nothing to clear, one launch.
__global__ __launch_bounds__(LB_T) void sequence_liabilities_kernel(const uint8_t* __restrict__ seq_all, const uint8_t* __restrict__ rows_all,
                                                                     const uint8_t* __restrict__ link_all, int run_min, int64_t N, int S, int n, int tiles,
                                                                     int64_t blocks, uint8_t* __restrict__ flags_all, int32_t* __restrict__ counts_all,
                                                                     int32_t* __restrict__ freq_all) {
    __shared__ uint8_t typ[LB_T + LB_HALO + 1], info[LB_T + LB_HALO + 1];
    __shared__ int red[LB_T / 64][LB_COUNTS];
    const int64_t b = folded_block();
    if (b >= blocks) return;                                                    // the last row of a folded grid; block-uniform
    const int tid = threadIdx.x;
    if (b < N) {
        const int64_t g = b / S;
        const uint8_t* seq = seq_all + b * n;
        const uint8_t* rows = rows_all ? rows_all + g * n : nullptr;
        const uint8_t* link = link_all ? link_all + g * n : nullptr;
        uint8_t* flags = flags_all + b * n;
        int cnt[LB_COUNTS];
#pragma unroll
        for (int k = 0; k < LB_COUNTS; ++k) cnt[k] = 0;
        for (int64_t k0 = 0; k0 < n; k0 += LB_T) {                             // 64-bit: k0 + 270 may pass 2^31
            __syncthreads();                                                    // the previous tile's reads are done
            for (int i = tid; i < LB_T + LB_HALO; i += LB_T) {
                const int64_t p = k0 + i;
                lb_put(typ, info, i, seq, p, n, p < n ? lb_rowlink(rows, link, p) : 0);
            }
            __syncthreads();
            const int64_t k = k0 + tid;
            if (k < n) {
                const int f = lb_flag(typ, info, tid, run_min);
                flags[k] = (uint8_t)f;
#pragma unroll
                for (int c = 0; c < 7; ++c) cnt[c] += (f >> c) & 1;
                cnt[7] += f != 0;
                const int t = typ[tid];
                if (info[tid] & LB_ROW) {
                    cnt[8] += t == AA_K || t == AA_R;
                    cnt[9] += t == AA_D || t == AA_E;
                    cnt[10] += t == AA_H;
                    cnt[11] += t < 20;
                    cnt[12] += lb_hyd10(t);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < LB_COUNTS; ++k) cnt[k] = wave_sum_butterfly(cnt[k]);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int k = 0; k < LB_COUNTS; ++k) red[tid >> 6][k] = cnt[k];
        }
        __syncthreads();
        if (tid < LB_COUNTS) counts_all[b * LB_COUNTS + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
        return;
    }
    const int64_t u = b - N;
    const int64_t g = u / tiles;
    const int64_t k0 = (u - g * tiles) * LB_T;
    const uint8_t* rows = rows_all ? rows_all + g * n : nullptr;
    const uint8_t* link = link_all ? link_all + g * n : nullptr;
    // the two slots a thread stages: tid and, for the halo, LB_T + tid; the rows and links are the group's, the same for every design
    const int64_t p0 = k0 + tid, p1 = k0 + LB_T + tid;
    const int rl0 = p0 < n ? lb_rowlink(rows, link, p0) : 0;
    const int rl1 = (tid < LB_HALO && p1 < n) ? lb_rowlink(rows, link, p1) : 0;
    int fr = 0;
    for (int s = 0; s < S; ++s) {
        const uint8_t* seq = seq_all + (g * S + s) * n;
        __syncthreads();
        lb_put(typ, info, tid, seq, p0, n, rl0);
        if (tid < LB_HALO) lb_put(typ, info, LB_T + tid, seq, p1, n, rl1);
        __syncthreads();
        if (p0 < n) fr += lb_flag(typ, info, tid, run_min) != 0;
    }
    if (p0 < n) freq_all[g * n + p0] = fr;
}

// ---------------------------------------------------------------- surface patches
constexpr int SP_TJ = 256;                 // residues staged at a time: 4 KB of LDS whatever L is

__device__ __forceinline__ float dv_add(float a, float b) { return a + b; }
__device__ __forceinline__ float dv_mul(float a, float b) { return a * b; }

// Residue r of a candidate as (centre, h = weight x area), or NaN in x for a residue that takes no part -- a NaN drops out of `d2 <= T` by definition.  The ONE
// rule of who takes part (include/abopt.h): side 1, the centre slot (CB if A >= 5 and CB is masked in, else CA) masked in with finite coordinates, a finite
// area >= 0 and a finite weight.
__device__ __forceinline__ float4 sp_residue(const float* __restrict__ pos, const uint8_t* __restrict__ mask, const int32_t* __restrict__ grp,
                                             const float* __restrict__ area, const uint8_t* __restrict__ seq, const float* __restrict__ weight, int r, int A) {
    const float qnan = __uint_as_float(0x7fc00000u);
    float4 v = make_float4(qnan, qnan, qnan, qnan);
    if (grp[r] != 1) return v;
    const uint8_t* m = mask + (int64_t)r * A;
    const int slot = (A >= 5 && m[4]) ? 4 : 1;
    if (!m[slot]) return v;
    const float* x = pos + ((int64_t)r * A + slot) * 3;
    const float a = area[r], w = weight[min((int)seq[r], 20)];
    if (finite_f32(x[0]) && finite_f32(x[1]) && finite_f32(x[2]) && finite_f32(a) && a >= 0.f && finite_f32(w)) v = make_float4(x[0], x[1], x[2], dv_mul(w, a));
    return v;
}

// Grid (candidate folded over x and y, slice in z), ONE wave per workgroup, a lane per target residue: the row is cut into units of 64 residues and slice s owns
// the units [nu s / slices, nu (s + 1) / slices).  For each of its units the wave walks ALL residues of the candidate in index order, staged through LDS as
// float4 (x, y, z, h) in tiles of 256: per occluder one broadcast read, the fused distance of candidate_common.h, a compare, a conditional add and a count.
// Every lane adds its neighbours' h in ascending j, from 0.0f; nothing is reduced across lanes, so no order but the definition's exists.  No prune.
__global__ __launch_bounds__(64) void surface_patches_kernel(const float* __restrict__ pos_all, const uint8_t* __restrict__ mask_all, int mask_shared,
                                                             const int32_t* __restrict__ group_all, const float* __restrict__ area_all,
                                                             const uint8_t* __restrict__ seq_all, int seq_shared, const float* __restrict__ weight, float thr,
                                                             int64_t N, int S, int L, int A, float* __restrict__ patch_all, int32_t* __restrict__ nbr_all) {
    __shared__ __attribute__((aligned(16))) float4 occ[SP_TJ];
    const int64_t c = folded_block();
    if (c >= N) return;                                                         // the last row of a folded grid; block-uniform
    const int64_t g = c / S;
    const int lane = threadIdx.x;
    const float* pos = pos_all + c * L * A * 3;
    const uint8_t* mask = mask_all + (mask_shared ? g : c) * L * A;
    const int32_t* grp = group_all + g * L;
    const float* area = area_all + c * L;
    const uint8_t* seq = seq_all + (seq_shared ? g : c) * L;
    const int nu = (L + 63) >> 6, slices = gridDim.z, slice = blockIdx.z;
    const int u_lo = (int)((int64_t)nu * slice / slices), u_hi = (int)((int64_t)nu * (slice + 1) / slices);
    for (int u = u_lo; u < u_hi; ++u) {
        const int i = u * 64 + lane;
        const float4 t = i < L ? sp_residue(pos, mask, grp, area, seq, weight, i, A) : make_float4(0.f, 0.f, 0.f, 0.f);
        float acc = 0.f;
        int cnt = 0;
        for (int j0 = 0; j0 < L; j0 += SP_TJ) {
            const int nj = min(SP_TJ, L - j0);
            __syncthreads();                                                    // the previous tile's reads are done
            for (int j = lane; j < nj; j += 64) occ[j] = sp_residue(pos, mask, grp, area, seq, weight, j0 + j, A);
            __syncthreads();
            for (int j = 0; j < nj; ++j) {
                const float4 o = occ[j];                                        // one broadcast read
                const bool near = d2_fma(__fsub_rn(t.x, o.x), __fsub_rn(t.y, o.y), __fsub_rn(t.z, o.z)) <= thr;       // false for a NaN on either side
                acc = near ? dv_add(acc, o.w) : acc;
                cnt += near;
            }
        }
        if (i < L) {
            patch_all[c * L + i] = acc;                                         // a target that takes no part is NaN: no comparison held, 0 and 0
            nbr_all[c * L + i] = cnt;
        }
    }
}

}  // namespace abopt

using namespace abopt;

extern "C" int abopt_sequence_liabilities_grouped(const uint8_t* seqs, const uint8_t* rows, const uint8_t* link, int run_min, int G, int S, int n, void* flags,
                                                  void* counts, void* freq, abopt_stream stream) {
    ABOPT_CHECK_ARG(G >= 0 && S >= 1 && n >= 1 && (int64_t)G * S * n <= 0x7fffffff, "sequence_liabilities_grouped: bad dims G=%d S=%d n=%d", G, S, n);
    ABOPT_CHECK_ARG(run_min == 0 || (run_min >= 2 && run_min <= LB_RUN_MAX), "sequence_liabilities_grouped: run_min=%d, expected 0 (off) or 2 .. %d", run_min,
                    LB_RUN_MAX);
    if (G == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(G <= kMaxGroups, "sequence_liabilities_grouped: G=%d groups exceed one launch (max %d)", G, kMaxGroups);
    ABOPT_CHECK_ARG(seqs && flags && counts, "sequence_liabilities_grouped: NULL argument");
    const int64_t N = (int64_t)G * S;
    const int tiles = (int)(((int64_t)n + LB_T - 1) / LB_T);
    const int64_t blocks = N + (freq ? (int64_t)G * tiles : 0);                 // <= 2 (2^31 - 1): far inside a folded grid
    hipLaunchKernelGGL(sequence_liabilities_kernel, fold_grid(blocks, 1u), dim3(LB_T), 0, (hipStream_t)stream, seqs, rows, link, run_min, N, S, n, tiles, blocks,
                       (uint8_t*)flags, (int32_t*)counts, (int32_t*)freq);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}

extern "C" int abopt_surface_patches_grouped(const float* pos, const uint8_t* mask, int mask_shared, const int32_t* group, const float* area, const uint8_t* seqs,
                                             int seq_shared, const float* weight, float radius, int G, int S, int L, int A, void* patch, void* nbr,
                                             abopt_stream stream) {
    int rc = check_candidate_dims("surface_patches_grouped", G, S, L, A);
    if (rc != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(A >= 2, "surface_patches_grouped: A=%d atoms per residue, the slot 1 is CA (expected 2 .. %d)", A, kMaxAtoms);
    static const char* const names[] = {"radius"};
    if ((rc = check_nonnegative("surface_patches_grouped", names, &radius, 1)) != ABOPT_OK) return rc;
    if (G == 0 || S == 0) return ABOPT_OK;
    if ((rc = check_group_count("surface_patches_grouped", G)) != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(pos && mask && group && area && seqs && weight && patch && nbr, "surface_patches_grouped: NULL argument");
    const int64_t N = (int64_t)G * S;
    const float thr = radius * radius;                                          // rounded once; +inf for a huge radius: every participating pair is a neighbour
    int cus = 0;
    if ((rc = device_cu_count(&cus)) != ABOPT_OK) return rc;
    // one wave per workgroup: enough of them for eight per CU, no slice thinner than one unit of 64 target residues
    const int slices = slice_count(cus, 8, N, ((int64_t)L + 63) / 64);
    hipLaunchKernelGGL(surface_patches_kernel, fold_grid(N, (unsigned)slices), dim3(64), 0, (hipStream_t)stream, pos, mask, mask_shared ? 1 : 0, group, area, seqs,
                       seq_shared ? 1 : 0, weight, thr, N, S, L, A, (float*)patch, (int32_t*)nbr);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}
