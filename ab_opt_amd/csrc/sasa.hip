// Solvent-accessible surface of docked candidates on the device, Shrake-Rupley: how many test points of every atom's probe-inflated
// sphere are hidden by the atom's own side (the free surface) and by either side (the surface in the complex); per residue the two areas, whose difference is
// the buried surface.  Nothing in the reference is matched; the definition is this library's own (include/abopt.h: abopt_sasa_grouped).  Counts are integers
// and the per-residue areas are summed in a fixed order by one wave, so no reduction order can change a result.
// Two launches: sasa_prepare_kernel writes one bounding sphere per residue into the workspace and zeroes `area` and `pts`; sasa_points_kernel walks, for every
// atom of a slice of a candidate's residues, the residues whose sphere can reach the atom's test points, and writes the residue's two areas and the point totals.
#include <math.h>
#include <algorithm>
#include "abopt_common.h"
#include "candidate_common.h"
#include "kernels.h"

// Every fp32 step of this file is rounded once; nothing may be contracted into an fma.  (So d2_fma of candidate_common.h is not for this file.)  hipcc contracts a * b + c across statements and across inlined
// functions by default, and __fadd_rn / __fsub_rn / __fmul_rn are plain operators to it that carry the permission with them from their header: written with
// them, q = c + R u and d2 were compiled to v_fma_f32 / v_fmac_f32.  So the round-to-nearest steps are spelled sa_add / sa_sub / sa_mul below -- the same
// operators, compiled under contract(off), which no later pass may fuse.  The two fmaf of the prune are explicit.
#pragma clang fp contract(off)

namespace abopt {

constexpr int SA_MAX_POINTS = 1024;        // test points per atom
constexpr int SA_TO = 64;                  // occluder residues staged at a time: one per lane for the prune
constexpr float SA_MAX_RADIUS = 16.f;      // a larger van der Waals radius takes no part

__device__ __forceinline__ float sa_add(float a, float b) { return a + b; }
__device__ __forceinline__ float sa_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float sa_mul(float a, float b) { return a * b; }

// the ONE rule of which atoms take part (include/abopt.h): mask byte set, finite coordinates, 0 < r <= 16 (a NaN radius fails both comparisons)
__device__ __forceinline__ bool sa_takes_part(uint8_t m, float x, float y, float z, float r) {
    return m && finite_f32(x) && finite_f32(y) && finite_f32(z) && r > 0.f && r <= SA_MAX_RADIUS;
}

// d2 = (dx dx + dy dy) + dz dz, every step rounded once, in this association
__device__ __forceinline__ float sa_d2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = sa_sub(ax, bx), dy = sa_sub(ay, by), dz = sa_sub(az, bz);
    return sa_add(sa_add(sa_mul(dx, dx), sa_mul(dy, dy)), sa_mul(dz, dz));
}

// One thread per (candidate, residue): the residue's bounding sphere into the workspace -- centre = the mean of its participating atoms, radius = the largest
// (distance from the centre + R) over them, so that every point an atom of the residue can hide lies inside; (0, 0, 0, -inf) for a residue that takes no part or
// has no participating atom (the prune always skips it; it hides nothing anyway) -- and zeroes for the residue's two areas and, from residue 0, the candidate's
// four point counters: plain stores, so that the chain a caller captures into a graph has no memset node.
__global__ __launch_bounds__(256) void sasa_prepare_kernel(const float* __restrict__ pos_all, const uint8_t* __restrict__ mask_all, int mask_shared,
                                                           const int32_t* __restrict__ group_all, const float* __restrict__ radius_all, float4* __restrict__ sph_all,
                                                           int32_t* __restrict__ pts, float* __restrict__ area, int64_t rows, int S, int L, int A, float probe) {
    const int64_t row = folded_block() * 256 + threadIdx.x;
    if (row >= rows) return;
    const int64_t c = row / L;
    const int r = (int)(row - c * L);
    const int64_t g = c / S;
    area[row * 2] = 0.f;
    area[row * 2 + 1] = 0.f;
    if (r == 0) { pts[c * 4] = 0; pts[c * 4 + 1] = 0; pts[c * 4 + 2] = 0; pts[c * 4 + 3] = 0; }
    float4 sph = make_float4(0.f, 0.f, 0.f, -INFINITY);
    const int side = group_all[g * L + r];
    if (side == 1 || side == 2) {
        const float* x = pos_all + row * A * 3;
        const uint8_t* m = mask_all + ((mask_shared ? g : c) * L + r) * A;
        const float* rad = radius_all + (g * L + r) * A;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        int cnt = 0;
        for (int p = 0; p < A; ++p)
            if (sa_takes_part(m[p], x[p * 3], x[p * 3 + 1], x[p * 3 + 2], rad[p])) { sx += x[p * 3]; sy += x[p * 3 + 1]; sz += x[p * 3 + 2]; ++cnt; }
        if (cnt) {
            const float inv = 1.f / (float)cnt;
            const float cx = sx * inv, cy = sy * inv, cz = sz * inv;
            float rb = 0.f;
            for (int p = 0; p < A; ++p)
                if (sa_takes_part(m[p], x[p * 3], x[p * 3 + 1], x[p * 3 + 2], rad[p])) {
                    const float v = sa_add(sqrtf(sa_d2(cx, cy, cz, x[p * 3], x[p * 3 + 1], x[p * 3 + 2])), sa_add(rad[p], probe));
                    rb = (v > rb || v != v) ? v : rb;                              // a NaN (an overflowed mean) sticks: the prune never skips it
                }
            sph = make_float4(cx, cy, cz, rb);
        }
    }
    sph_all[row] = sph;
}

// Grid (candidate folded over x and y, slice in z), 4 waves.  The participating residues of the candidate (group 1 or 2) are numbered in index order and slice s
// takes the ranks [np s / slices, np (s + 1) / slices): the re-dock shape has fewer candidates than the chip has CUs.  Per workgroup:
//   target tile   up to TT residues of the slice (TT / 4 per wave): indices compacted by ballots (take, candidate_common.h), atoms staged in LDS as float4 (x, y, z, R); an atom
//                 that takes no part is staged as NaN and skipped.  Two verdict words per (residue, atom, pass of 64 points) in LDS, bit = lane = point: hidden by
//                 the own side / by the other side.  They persist while the occluder tiles go by.
//   occluder tile up to 64 participating residues of the candidate, atoms staged as float4 (x, y, z, T) -- an atom that takes no part as NaN, which drops out of
//                 `d2 < T` by definition --, their sides, and their bounding spheres from the workspace, one per lane.
//   an atom       a wave owns one target atom at a time.  __ballot over the lanes' spheres gives the occluder residues of the tile that can reach the atom's
//                 points (below); for every pass of 64 points a lane computes ITS point q once and walks those residues: each occluder atom is one broadcast LDS
//                 read, own and other are two bits per lane.  The walk of a pass ends once every live lane is hidden by its own side -- such a point counts
//                 nowhere, whatever else hides it -- and a pass whose stored word says so is not entered again.
//   areas         after the last occluder tile the words of a residue are counted, atom by atom in ascending order, into the two areas of the residue:
//                 acc = acc + float(count) (k T), by every lane of the wave alike; lane 0 stores.  No float atomic anywhere.  The point totals of the wave go to
//                 `pts` by one integer atomicAdd per counter.
// LDS (TT = 16 for n <= 128, else 4): A <= 5, n <= 128: 5.0 KB of occluder atoms + 1.3 KB of target atoms + 2.5 KB of verdict words + 1.7 KB of indices, sides and spheres;
// A = 15, n = 1024: 15 + 0.9 + 15 + 1.6 KB -- whatever L is.
//
// The prune is conservative in fp32.  A point q of target atom i is hidden by occluder atom j iff the computed d2(q, c_j) < T_j.  q = fl(c_i + fl(R_i u)) lies
// within R_i |u| (1 + u0) + e of c_i (u0 = 2^-24), where e <= 2^-23 (|c_ix| + |c_iy| + |c_iz| + 3 R_i |u|) bounds the roundings of the three products and the three
// sums (each half an ulp of its result).  A computed d2 of two fp32 points is the true one x (1 +- 5 u0) (one rounded subtraction relative to the difference, a
// square, two sums of non-negative terms), and T_j = fl(R_j R_j), so d2 < T_j gives |q - c_j| <= R_j (1 + 4 u0).  The sphere of j's residue has the fp32 centre m
// (whatever the mean rounds to: the radius is measured from THAT point) and the computed radius rb >= (|c_j - m| (1 - 4 u0) + R_j) (1 - u0).  So a hidden point has
//   |c_i - m| <= R_i umax (1 + u0) + e + (rb)(1 + 6 u0),   umax = the largest |u| of the caller's directions (computed here, so a direction that is not quite
// of unit length costs tightness, not correctness), and the computed distance D^ >= |c_i - m| (1 - 4 u0).  The residue is skipped iff
//   D^ > (R_i umax^ + rb) (1 + 2^-16) + 0.01 + 2^-21 (|c_ix| + |c_iy| + |c_iz| + 3 R_i umax^):
// 2^-16 = 256 u0 covers every relative term above with room to spare (umax^ itself is good to 4 u0 and is widened by 2^-20), the last term is 4 e, and the 0.01 A
// would cover a centre whose arithmetic were off by ten ulps of a coordinate of 10^4 A.  A NaN sphere is never skipped (the comparison is false), an infinite
// umax skips nothing.  The same bound, read the other way, is the test's: float32 and float64 statements of the definition can differ only on a point whose
// float64 margin |d - R_j| is below 64 ulps of the largest magnitude entering q, 2^-18 (max |coordinate| + max R) -- q carries <= 2 roundings of that magnitude
// per coordinate, d2 and T the relative 5 u0 above, far inside 64.
template <int AQ, int PQ>
__global__ __launch_bounds__(256) void sasa_points_kernel(const float* __restrict__ pos_all, const uint8_t* __restrict__ mask_all, int mask_shared,
                                                          const int32_t* __restrict__ group_all, const float* __restrict__ radius_all,
                                                          const float* __restrict__ dirs, int n, const float4* __restrict__ sph_all, int32_t* __restrict__ pts_all,
                                                          float* __restrict__ area_all, int N, int S, int L, int A, float probe, float kf) {
    constexpr int TT = PQ <= 2 ? 16 : 4;
    __shared__ __attribute__((aligned(16))) float4 occ[SA_TO][AQ];
    __shared__ __attribute__((aligned(16))) float4 tgt[TT][AQ];
    __shared__ __attribute__((aligned(16))) float4 sph_o[SA_TO];
    __shared__ __attribute__((aligned(16))) ulonglong2 vb[TT][AQ][PQ];
    __shared__ int idx_o[SA_TO], side_o[SA_TO], idx_t[TT], side_t[TT];
    const int64_t c64 = folded_block();
    if (c64 >= N) return;                                                       // the last row of a folded grid; block-uniform
    const int slice = blockIdx.z, slices = gridDim.z;
    const int64_t g = c64 / S;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* pos = pos_all + c64 * L * A * 3;
    const uint8_t* mask = mask_all + (mask_shared ? g : c64) * L * A;
    const int32_t* grp = group_all + g * L;
    const float* radius = radius_all + g * L * A;
    const float4* sph = sph_all + c64 * L;
    float* area = area_all + c64 * L * 2;
    const float qnan = __uint_as_float(0x7fc00000u);
    const int passes = (n + 63) >> 6;                                           // <= PQ, checked by the host

    // ---- this slice's ranks of participating residues (every wave counts the row itself: wave-uniform, no exchange)
    const OnEitherSide part{grp};
    int cur_t;
    int left = slice_ranks(L, part, slice, slices, cur_t);
    if (left == 0) return;                                                      // block-uniform

    // ---- the largest length of a direction, widened: wave-uniform
    float umax = 0.f;
    for (int b = 0; b < n; b += 64) {
        const int i = b + lane;
        if (i < n) umax = fmaxf(umax, sa_d2(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2], 0.f, 0.f, 0.f));      // a NaN direction hides nowhere: ignored
    }
    for (int off = 32; off > 0; off >>= 1) umax = fmaxf(umax, __shfl_xor(umax, off, 64));
    umax = sqrtf(umax) * (1.f + 9.5367431640625e-7f);

    int free1 = 0, free2 = 0, cplx1 = 0, cplx2 = 0;                             // wave-uniform: exposed points by side, free and in the complex
    while (left > 0) {
        __syncthreads();                                                        // the previous tile's reads are done
        const int ntt = take(L, part, cur_t, min(TT, left), idx_t, wave == 0);
        left -= ntt;
        if (ntt == 0) break;                                                    // cannot happen (the ranks were counted on the same row); block-uniform
        __syncthreads();
        for (int t = tid; t < ntt * AQ; t += 256) {
            const int i = t / AQ, p = t % AQ, r = idx_t[i];
            float4 v = make_float4(qnan, qnan, qnan, qnan);
            if (p < A) {
                const float* x = pos + ((int64_t)r * A + p) * 3;
                const float rr = radius[(int64_t)r * A + p];
                if (sa_takes_part(mask[(int64_t)r * A + p], x[0], x[1], x[2], rr)) v = make_float4(x[0], x[1], x[2], sa_add(rr, probe));
            }
            tgt[i][p] = v;
        }
        if (tid < ntt) side_t[tid] = grp[idx_t[tid]];
        for (int t = tid; t < ntt * AQ * PQ; t += 256) (&vb[0][0][0])[t] = make_ulonglong2(0ull, 0ull);

        int cur_o = 0;
        while (true) {
            __syncthreads();                                                    // the previous occluder tile's reads are done (and the target tile is written)
            const int nto = take(L, part, cur_o, SA_TO, idx_o, wave == 0);
            if (nto == 0) break;                                                // block-uniform
            __syncthreads();
            for (int t = tid; t < nto * AQ; t += 256) {
                const int j = t / AQ, q = t % AQ, r = idx_o[j];
                float4 v = make_float4(qnan, qnan, qnan, qnan);
                if (q < A) {
                    const float* x = pos + ((int64_t)r * A + q) * 3;
                    const float rr = radius[(int64_t)r * A + q];
                    if (sa_takes_part(mask[(int64_t)r * A + q], x[0], x[1], x[2], rr)) {
                        const float R = sa_add(rr, probe);
                        v = make_float4(x[0], x[1], x[2], sa_mul(R, R));
                    }
                }
                occ[j][q] = v;
            }
            if (tid < nto) { side_o[tid] = grp[idx_o[tid]]; sph_o[tid] = sph[idx_o[tid]]; }
            __syncthreads();
            const bool have = lane < nto;
            const float4 sb = have ? sph_o[lane] : make_float4(0.f, 0.f, 0.f, -INFINITY);
            for (int i = wave; i < ntt; i += 4) {
                const int ri = idx_t[i], si = side_t[i];
                for (int p = 0; p < A; ++p) {
                    const float4 t = tgt[i][p];
                    if (!(t.w == t.w)) continue;                                // takes no part; wave-uniform
                    const float ru = t.w * umax;
                    const float reach = fmaf(sa_add(ru, sb.w), 1.f + 1.52587890625e-5f,
                                             fmaf(4.76837158203125e-7f, fabsf(t.x) + fabsf(t.y) + fabsf(t.z) + 3.f * ru, 0.01f));
                    const unsigned long long near = __ballot(have && !(sqrtf(sa_d2(t.x, t.y, t.z, sb.x, sb.y, sb.z)) > reach));
                    if (near == 0ull) continue;
                    for (int s = 0; s < passes; ++s) {
                        const int pt = s * 64 + lane;
                        const bool live = pt < n;
                        const unsigned long long livemask = __ballot(live);
                        const ulonglong2 w = vb[i][p][s];
                        if ((w.x & livemask) == livemask) continue;             // every point of the pass is hidden by the own side already
                        bool own = (w.x >> lane) & 1ull, oth = (w.y >> lane) & 1ull;
                        const float ux = live ? dirs[pt * 3] : 0.f, uy = live ? dirs[pt * 3 + 1] : 0.f, uz = live ? dirs[pt * 3 + 2] : 0.f;
                        const float qx = sa_add(t.x, sa_mul(t.w, ux)), qy = sa_add(t.y, sa_mul(t.w, uy)), qz = sa_add(t.z, sa_mul(t.w, uz));
                        for (unsigned long long m = near; m; m &= m - 1ull) {
                            const int j = __builtin_ctzll(m);                   // wave-uniform
                            const int self = idx_o[j] == ri ? p : -1;
                            bool h = false;
                            for (int q = 0; q < A; ++q) {
                                const float4 o = occ[j][q];                     // one broadcast read
                                const float T = q == self ? -INFINITY : o.w;    // j != i; wave-uniform
                                h = h | (sa_d2(qx, qy, qz, o.x, o.y, o.z) < T);
                            }
                            if (side_o[j] == si) {
                                own = own | h;
                                if (__ballot(live && !own) == 0ull) break;
                            } else {
                                oth = oth | h;
                            }
                        }
                        const unsigned long long bo = __ballot(own) & livemask, bt = __ballot(oth) & livemask;
                        if (lane == 0) vb[i][p][s] = make_ulonglong2(bo, bt);
                    }
                }
            }
            if (nto < SA_TO) break;                                             // the row ended inside this tile; block-uniform
        }

        // ---- the tile's residues: counts -> areas, in ascending atom order (a wave reads only the words it wrote itself)
        for (int i = wave; i < ntt; i += 4) {
            const int si = side_t[i];
            float acc_free = 0.f, acc_cplx = 0.f;
            for (int p = 0; p < A; ++p) {
                const float4 t = tgt[i][p];
                if (!(t.w == t.w)) continue;
                int nf = 0, nc = 0;
                for (int s = 0; s < passes; ++s) {
                    const unsigned long long livemask = n - s * 64 >= 64 ? ~0ull : (1ull << (n - s * 64)) - 1ull;
                    const ulonglong2 w = vb[i][p][s];
                    nf += __popcll(livemask & ~w.x);
                    nc += __popcll(livemask & ~w.x & ~w.y);
                }
                const float kt = sa_mul(kf, sa_mul(t.w, t.w));
                acc_free = sa_add(acc_free, sa_mul((float)nf, kt));
                acc_cplx = sa_add(acc_cplx, sa_mul((float)nc, kt));
                if (si == 1) { free1 += nf; cplx1 += nc; } else { free2 += nf; cplx2 += nc; }
            }
            if (lane == 0) { area[(int64_t)idx_t[i] * 2] = acc_free; area[(int64_t)idx_t[i] * 2 + 1] = acc_cplx; }
        }
    }
    if (lane == 0) {
        int32_t* pts = pts_all + c64 * 4;
        if (free1) atomicAdd(&pts[0], free1);
        if (free2) atomicAdd(&pts[1], free2);
        if (cplx1) atomicAdd(&pts[2], cplx1);
        if (cplx2) atomicAdd(&pts[3], cplx2);
    }
}

}  // namespace abopt

using namespace abopt;

namespace abopt {
// one float4 (bounding sphere) per residue of every candidate
size_t sasa_ws_bytes(int G, int S, int L, int A) {
    if (G <= 0 || S <= 0 || L <= 0 || A <= 0) return 0;
    return (size_t)G * S * L * sizeof(float4);
}
}  // namespace abopt

extern "C" size_t abopt_sasa_ws_bytes(int G, int S, int L, int A) { return sasa_ws_bytes(G, S, L, A); }

extern "C" int abopt_sasa_grouped(const float* pos, const uint8_t* mask, int mask_shared, const int32_t* group, const float* radius, const float* dirs,
                                  int n_points, int G, int S, int L, int A, float probe, float k, void* pts, void* area, void* ws, size_t ws_bytes,
                                  abopt_stream stream) {
    int rc = check_candidate_dims("sasa_grouped", G, S, L, A);
    if (rc != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(n_points >= 1 && n_points <= SA_MAX_POINTS, "sasa_grouped: n_points=%d test points per atom, expected 1 .. %d", n_points, SA_MAX_POINTS);
    ABOPT_CHECK_ARG(isfinite(probe) && probe >= 0.f, "sasa_grouped: the probe radius must be finite and >= 0 (got %g)", (double)probe);
    ABOPT_CHECK_ARG(isfinite(k), "sasa_grouped: k (the area of one test point on the unit sphere, 4 pi / n) must be finite (got %g)", (double)k);
    if (G == 0 || S == 0) return ABOPT_OK;
    if ((rc = check_group_count("sasa_grouped", G)) != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(pos && mask && group && radius && dirs && pts && area && ws, "sasa_grouped: NULL argument");
    const int64_t N = (int64_t)G * S, rows = N * L, prep_blocks = (rows + 255) / 256;
    ABOPT_CHECK_ARG(prep_blocks <= (int64_t)kGridX * 65535, "sasa_grouped: G S L = %lld residues exceed one launch", (long long)rows);
    if ((rc = check_workspace("sasa_grouped", ws, 16, ws_bytes, sasa_ws_bytes(G, S, L, A))) != ABOPT_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    int cus = 0;
    if ((rc = device_cu_count(&cus)) != ABOPT_OK) return rc;
    // enough workgroups for four per CU, no slice thinner than four residues of the row
    const int slices = slice_count(cus, 4, N, ((int64_t)L + 3) / 4);
    hipLaunchKernelGGL(sasa_prepare_kernel, fold_grid(prep_blocks, 1u), dim3(256), 0, st, pos, mask, mask_shared ? 1 : 0, group, radius, (float4*)ws, (int32_t*)pts,
                       (float*)area, rows, S, L, A, probe);
    ABOPT_LAUNCH_CHECK();
    const bool few = n_points <= 128;
    auto kernel = A <= 5 ? (few ? sasa_points_kernel<5, 2> : sasa_points_kernel<5, 16>) : (few ? sasa_points_kernel<kMaxAtoms, 2> : sasa_points_kernel<kMaxAtoms, 16>);
    hipLaunchKernelGGL(kernel, fold_grid(N, (unsigned)slices), dim3(256), 0, st, pos, mask, mask_shared ? 1 : 0, group, radius, dirs, n_points, (const float4*)ws,
                       (int32_t*)pts, (float*)area, (int)N, S, L, A, probe, k);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}
