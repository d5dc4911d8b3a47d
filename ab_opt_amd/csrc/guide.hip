// Guided sampling: after a reverse step, a geometric potential nudges the generated residues of every sample -- a rigid pull of the
// generated set towards the centroid of the hotspot residues, and a push of each generated residue away from the repeller residues that are closer than a
// radius.  Nothing in the reference is matched; the definition is this library's own (include/abopt.h: abopt_guide_positions).  One launch, in place on p.
// One workgroup owns a sample, so nobody else reads the sample's centroid or its rows while they are written; every sum is taken in a fixed order (lanes stride
// the rows, a butterfly over the wave, the four waves in ascending order): no float atomic, no workspace, and a repeated call gives the same bits.
#include <math.h>
#include "abopt_common.h"
#include "candidate_common.h"
#include "kernels.h"

// The squared distances are d2_fma of candidate_common.h (an fmaf chain; included before the pragma), as in interface.hip, and everything else -- the differences, the
// force sums, p + shift, (p - mean) / scale -- as plain operators under contract(off), as in sasa.hip: hipcc would otherwise contract a * b + c across statements
// (DESIGN.md section 6.6), and p_norm has to be the rounded difference divided by the scale, bit for bit what denoise_store_position writes.
#pragma clang fp contract(off)

namespace abopt {

constexpr int GD_WAVES = 4;                // waves per workgroup
constexpr int GD_SEG = 256;                // rows of a repeller tile that one wave compacts
constexpr int GD_TILE = GD_WAVES * GD_SEG; // rows per repeller tile: 16 KB of LDS whatever L is
constexpr int GD_K = 4;                    // moved rows a wave carries through the tiles at a time
constexpr int GD_PASS = GD_WAVES * GD_K;   // consecutive rows dealt to the waves per pass

// Grid: the sample folded over x and y; 4 waves.
//   phase A   thread t strides the rows t, t + 256, ...: coordinate sums (relative to position_mean, so that the magnitudes stay small) and counts of the moved
//             rows M = gen & res and of the hotspots H = res & ~gen & bit 0; butterfly per wave, one LDS exchange, the waves added in ascending order by every
//             thread.  From them the attraction a, the same for every moved row.
//   phase B   the rows are dealt to the waves 16 at a time (row r of a pass to wave (r / 4) % 4); a pass without a moved row costs one ballot.  The repellers
//             R = res & ~gen & bit 1 of a tile of 1024 rows are staged in LDS as float4, compacted by ballot ranks, each wave its own 256 rows of the tile.  The
//             lanes of a wave stride the tile's repellers for each of the wave's moved rows and keep the three partial sums of a row in registers across the tiles;
//             after the last tile one butterfly per row, and lane 0 adds a, caps the shift and stores.  With L <= 1024 the one tile is staged once for all passes.
// The update is in place and race-free: the forces read context rows (never written) and the centroid of M, which is complete before the first store; a moved
// row is read by the wave that writes it alone.
__global__ __launch_bounds__(256) void guide_positions_kernel(float* __restrict__ p_all, float* __restrict__ pn_all, const uint8_t* __restrict__ gen_all,
                                                              const uint8_t* __restrict__ res_all, const int32_t* __restrict__ role_all, int S, int N, int L,
                                                              float w_att, float r_att, float w_rep, float r_rep, float max_shift, float scale, float m0,
                                                              float m1, float m2) {
    __shared__ __attribute__((aligned(16))) float4 rep[GD_WAVES][GD_SEG];
    __shared__ float red[GD_WAVES][6];
    __shared__ int redn[GD_WAVES][2];
    __shared__ int cnt[GD_WAVES];
    const int64_t c = folded_block();
    if (c >= N) return;                                                         // the last row of a folded grid; block-uniform
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* p = p_all + c * L * 3;
    float* pn = pn_all ? pn_all + c * L * 3 : nullptr;
    const uint8_t* gen = gen_all + c * L;
    const uint8_t* res = res_all + c * L;
    const int32_t* role = role_all + (S > 0 ? c / S : c) * L;

    // ---- phase A: centroids and counts of M and H
    float sm0 = 0.f, sm1 = 0.f, sm2 = 0.f, sh0 = 0.f, sh1 = 0.f, sh2 = 0.f;
    int nm = 0, nh = 0;
    for (int r = tid; r < L; r += 256) {
        if (!res[r]) continue;
        const bool g = gen[r] != 0;
        if (!g && !(role[r] & 1)) continue;
        const float x = p[r * 3] - m0, y = p[r * 3 + 1] - m1, z = p[r * 3 + 2] - m2;
        if (g) { sm0 = sm0 + x; sm1 = sm1 + y; sm2 = sm2 + z; ++nm; }
        else   { sh0 = sh0 + x; sh1 = sh1 + y; sh2 = sh2 + z; ++nh; }
    }
    sm0 = wave_sum_butterfly(sm0); sm1 = wave_sum_butterfly(sm1); sm2 = wave_sum_butterfly(sm2);
    sh0 = wave_sum_butterfly(sh0); sh1 = wave_sum_butterfly(sh1); sh2 = wave_sum_butterfly(sh2);
    nm = wave_sum_butterfly(nm); nh = wave_sum_butterfly(nh);
    if (lane == 0) {
        red[wave][0] = sm0; red[wave][1] = sm1; red[wave][2] = sm2; red[wave][3] = sh0; red[wave][4] = sh1; red[wave][5] = sh2;
        redn[wave][0] = nm; redn[wave][1] = nh;
    }
    __syncthreads();
    sm0 = red[0][0]; sm1 = red[0][1]; sm2 = red[0][2]; sh0 = red[0][3]; sh1 = red[0][4]; sh2 = red[0][5];
    nm = redn[0][0]; nh = redn[0][1];
#pragma unroll
    for (int w = 1; w < GD_WAVES; ++w) {
        sm0 = sm0 + red[w][0]; sm1 = sm1 + red[w][1]; sm2 = sm2 + red[w][2]; sh0 = sh0 + red[w][3]; sh1 = sh1 + red[w][4]; sh2 = sh2 + red[w][5];
        nm += redn[w][0]; nh += redn[w][1];
    }
    if (nm == 0) return;                                                        // nothing to move; block-uniform
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (nh > 0) {
        const float fm = (float)nm, fh = (float)nh;
        const float dx = sh0 / fh - sm0 / fm, dy = sh1 / fh - sm1 / fm, dz = sh2 / fh - sm2 / fm;
        const float D = sqrtf(d2_fma(dx, dy, dz));
        if (D > 0.f) {
            const float g = w_att * fmaxf(D - r_att, 0.f) / D;
            ax = g * dx; ay = g * dy; az = g * dz;
        }
    }
    const bool repel = w_rep > 0.f && r_rep > 0.f;                              // otherwise every term of the sum is 0: no tile is staged
    const int tiles = repel ? (L + GD_TILE - 1) / GD_TILE : 0;
    const double cap2 = (double)max_shift * (double)max_shift;
    bool staged = false;

    // ---- phase B
    for (int r0 = 0; r0 < L; r0 += GD_PASS) {
        const int rl = r0 + lane;
        const unsigned long long mb = __ballot(lane < GD_PASS && rl < L && gen[rl] != 0 && res[rl] != 0);      // the same word in every wave
        if (mb == 0ull) continue;                                               // block-uniform
        const unsigned mine = (unsigned)(mb >> (wave * GD_K)) & ((1u << GD_K) - 1u);
        float px[GD_K], py[GD_K], pz[GD_K], fx[GD_K], fy[GD_K], fz[GD_K];
#pragma unroll
        for (int k = 0; k < GD_K; ++k) {
            const int i = r0 + wave * GD_K + k;
            const bool on = (mine >> k) & 1u;                                   // wave-uniform
            px[k] = on ? p[i * 3] : 0.f; py[k] = on ? p[i * 3 + 1] : 0.f; pz[k] = on ? p[i * 3 + 2] : 0.f;
            fx[k] = 0.f; fy[k] = 0.f; fz[k] = 0.f;
        }
        for (int tile = 0; tile < tiles; ++tile) {
            if (tiles > 1 || !staged) {                                         // block-uniform
                __syncthreads();                                                // the readers of the tile that is replaced are done
                const int base = tile * GD_TILE + wave * GD_SEG;
                int n = 0;
#pragma unroll
                for (int q = 0; q < GD_SEG / 64; ++q) {
                    const int r = base + q * 64 + lane;
                    const bool f = r < L && res[r] != 0 && gen[r] == 0 && (role[r] & 2) != 0;
                    const unsigned long long b = __ballot(f);
                    if (f) rep[wave][n + __popcll(b & ((1ull << lane) - 1ull))] = make_float4(p[r * 3], p[r * 3 + 1], p[r * 3 + 2], 0.f);
                    n += __popcll(b);                                           // <= 256: a segment has 256 rows
                }
                if (lane == 0) cnt[wave] = n;
                __syncthreads();
                staged = true;
            }
            if (mine == 0u) continue;                                           // wave-uniform; the barriers above are passed by every wave
#pragma unroll
            for (int w = 0; w < GD_WAVES; ++w) {
                const int n = cnt[w];
                for (int j = lane; j < n; j += 64) {
                    const float4 q = rep[w][j];
#pragma unroll
                    for (int k = 0; k < GD_K; ++k) {
                        if (!((mine >> k) & 1u)) continue;
                        const float dx = px[k] - q.x, dy = py[k] - q.y, dz = pz[k] - q.z;
                        const float d2 = d2_fma(dx, dy, dz);
                        if (d2 < 1e-12f) continue;                              // a coincident pair has no direction: it contributes 0
                        const float d = sqrtf(d2);
                        const float s = fmaxf(r_rep - d, 0.f) / d;
                        fx[k] = fx[k] + s * dx; fy[k] = fy[k] + s * dy; fz[k] = fz[k] + s * dz;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < GD_K; ++k) {
            if (!((mine >> k) & 1u)) continue;                                  // wave-uniform
            const float sx = wave_sum_butterfly(fx[k]), sy = wave_sum_butterfly(fy[k]), sz = wave_sum_butterfly(fz[k]);
            if (lane != 0) continue;
            float dx = ax + w_rep * sx, dy = ay + w_rep * sy, dz = az + w_rep * sz;
            // the cap in double: the capped shift is max_shift / |shift| times the shift with ONE fp32 rounding per component, so its length stays
            // within max_shift (1 + 2^-23) whatever the roundings of an fp32 norm would have been
            const double n2 = (double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz;
            if (n2 > cap2) {
                const double q = (double)max_shift / sqrt(n2);
                dx = (float)((double)dx * q); dy = (float)((double)dy * q); dz = (float)((double)dz * q);
            }
            if (dx == 0.f && dy == 0.f && dz == 0.f) continue;                  // the row keeps its bits
            const int i = r0 + wave * GD_K + k;
            const float x = px[k] + dx, y = py[k] + dy, z = pz[k] + dz;
            p[i * 3] = x; p[i * 3 + 1] = y; p[i * 3 + 2] = z;
            if (pn) { pn[i * 3] = (x - m0) / scale; pn[i * 3 + 1] = (y - m1) / scale; pn[i * 3 + 2] = (z - m2) / scale; }
        }
    }
}

}  // namespace abopt

using namespace abopt;

extern "C" int abopt_guide_positions(float* p, float* p_norm, const uint8_t* mask_generate, const uint8_t* mask_res, const int32_t* role, int role_shared,
                                     int N, int L, float w_att, float r_att, float w_rep, float r_rep, float max_shift, float position_scale,
                                     const float* position_mean, abopt_stream stream) {
    ABOPT_CHECK_ARG(N >= 0 && L >= 0 && (int64_t)L * 3 <= 0x7fffffff, "guide_positions: bad dims N=%d L=%d", N, L);
    ABOPT_CHECK_ARG(role_shared >= 0 && (role_shared == 0 || N % role_shared == 0),
                    "guide_positions: N=%d samples are not whole groups of role_shared=%d", N, role_shared);
    const float sc[6] = {w_att, r_att, w_rep, r_rep, max_shift, position_scale};
    static const char* const names[6] = {"w_att", "r_att", "w_rep", "r_rep", "max_shift", "position_scale"};
    if (const int rc = check_nonnegative("guide_positions", names, sc, 6)) return rc;
    ABOPT_CHECK_ARG(w_att <= 1.f, "guide_positions: w_att must be <= 1, the pull may not overshoot (got %g)", (double)w_att);
    ABOPT_CHECK_ARG(max_shift > 0.f, "guide_positions: max_shift must be > 0 (got %g)", (double)max_shift);
    ABOPT_CHECK_ARG(position_scale > 0.f, "guide_positions: position_scale must be > 0 (got %g)", (double)position_scale);
    ABOPT_CHECK_ARG(p && mask_generate && mask_res && role && position_mean, "guide_positions: NULL argument");
    ABOPT_CHECK_ARG(isfinite(position_mean[0]) && isfinite(position_mean[1]) && isfinite(position_mean[2]), "guide_positions: position_mean must be finite");
    if (N == 0 || L == 0) return ABOPT_OK;
    if (w_att == 0.f && w_rep == 0.f) return ABOPT_OK;                          // every shift is 0: nothing is written
    ABOPT_CHECK_ARG((int64_t)N <= (int64_t)kGridX * 65535, "guide_positions: N=%d samples exceed one launch", N);
    hipLaunchKernelGGL(guide_positions_kernel, fold_grid(N, 1u), dim3(256), 0, (hipStream_t)stream, p, p_norm, mask_generate,
                       mask_res, role, role_shared, N, L, w_att, r_att, w_rep, r_rep, max_shift, position_scale, position_mean[0], position_mean[1],
                       position_mean[2]);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}
