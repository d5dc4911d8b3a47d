// lDDT-CA of candidate structures on the device: every candidate of a group against the group's reference structure, per residue
// (abopt_lddt_ca_grouped), and every candidate of a group against every other one, pooled over the residues (abopt_lddt_ca_ensemble).  The definition is the
// text of include/abopt.h; all results are integer counts, so no order of the additions can change them.
// Two launches: lddt_prep_kernel zeroes the outputs, packs the CA of every structure into the workspace as float4 and compacts the scored rows of every group;
// lddt_pairs_kernel walks the pairs (row i, residue j) with one row per lane and leaves num / den by integer atomics.
#include <math.h>
#include <algorithm>
#include "abopt_common.h"
#include "kernels.h"

namespace abopt {

constexpr int LD_B = 4;                    // models scored against one reference tile in the ensemble form: dt of a pair is computed once for the four
constexpr int LD_GRID_X = 1 << 22;         // workgroups along x: units beyond fold into y
constexpr int LD_MAX_SLICES = 64;          // workgroups the tiles of one unit are split over at most

// The ONE distance of this file, the spelling of interface.hip: fmaf(dz, dz, fmaf(dy, dy, dx dx)), every step rounded once, then the root.
__device__ __forceinline__ float ld_dist(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return __fsqrt_rn(fmaf(dz, dz, fmaf(dy, dy, __fmul_rn(dx, dx))));
}

__device__ __forceinline__ float ld_lane(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// Grid-stride, 256 threads.  (1) num / den <- 0 (plain vector stores: the chain a caller captures has no memset node).  (2) The CA (atom slot 1) of every
// candidate, and of every reference in the grouped form, as float4 {x, y, z, valid}: valid = the CA's mask byte is set; an invalid residue holds NaN
// coordinates, so that as the REFERENCE side of a pair it fails dt < cutoff by itself, and valid = 0 takes it out as the MODEL side.  A NaN coordinate of a
// valid residue stays what it is.  (3) One wave per group: the indices of the rows that are scored (rows[g][r] != 0, or all), compacted in index order.
__global__ __launch_bounds__(256) void lddt_prep_kernel(const float* __restrict__ pos, const uint8_t* __restrict__ mask, int mask_shared,
                                                        const float* __restrict__ ref_pos, const uint8_t* __restrict__ ref_mask,
                                                        const uint8_t* __restrict__ rows, float4* __restrict__ model, float4* __restrict__ ref,
                                                        int32_t* __restrict__ rowidx, int32_t* __restrict__ nrows, int32_t* __restrict__ num,
                                                        int32_t* __restrict__ den, size_t nout, int64_t N, int G, int S, int L, int A) {
    const size_t step = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t i = t0; i < nout; i += step) { num[i] = 0; den[i] = 0; }
    const float qnan = __uint_as_float(0x7fc00000u);
    const size_t nm = (size_t)N * L, nall = nm + (ref_pos ? (size_t)G * L : 0);
    for (size_t i = t0; i < nall; i += step) {
        const bool is_ref = i >= nm;
        const size_t idx = is_ref ? i - nm : i, s = idx / L, r = idx % L;
        const float* p = (is_ref ? ref_pos : pos) + (idx * A + 1) * 3;
        const uint8_t* m = is_ref ? ref_mask + idx * A + 1 : mask + ((mask_shared ? s / S : s) * L + r) * A + 1;
        const bool ok = *m != 0;
        (is_ref ? ref : model)[idx] = ok ? make_float4(p[0], p[1], p[2], 1.f) : make_float4(qnan, qnan, qnan, 0.f);
    }
    const int lane = threadIdx.x & 63;
    for (size_t g = t0 >> 6; g < (size_t)G; g += step >> 6) {                   // wave-uniform
        int n = 0;
        for (int r0 = 0; r0 < L; r0 += 64) {
            const int r = r0 + lane;
            const bool f = r < L && (!rows || rows[g * L + r]);
            const unsigned long long b = __ballot(f);
            if (f) rowidx[g * L + n + __popcll(b & ((1ull << lane) - 1ull))] = r;
            n += __popcll(b);
        }
        if (lane == 0) nrows[g] = n;
    }
}

// 4 waves per workgroup, every wave a unit of its own (no LDS, no barrier), slice in z.
//   grouped  (ENS = false, B = 1): unit = (candidate c, chunk rc of 64 compacted rows); reference = ref[g], model = model[c]; the wave walks the j-tiles
//            slice, slice + slices, ... and adds its lanes' counters to num / den [c][i].
//   ensemble (ENS = true): unit = (group g, reference a, block of B models b0 .. b0 + B - 1); reference = model[g S + a]; the wave walks the pairs
//            (row chunk, j-tile) slice, slice + slices, ..., sums its lanes' counters and adds them to num / den [g][a][b].
// A lane owns row i = rowidx[rc 64 + lane]: its reference and model CA stay in registers.  A j-tile is 64 residues, one per lane, and is broadcast lane by
// lane with v_readlane (the index is wave-uniform): reference CA, the B model CAs, and one word of flags (bit k: model k is valid at j; bits 8..: the side of j
// if `group` is given, else 0).  The pair is scored iff dt < cutoff (false for a NaN: an invalid or NaN reference residue on either end), j != i and the side
// of j is the one row i wants (the other of {1, 2}; 0 without `group`; -2 for a lane without a row, which nothing matches); model k then counts it iff it is
// valid at both ends.  dt is computed once per pair, for all B models.
template <int B, bool ENS>
__global__ __launch_bounds__(256) void lddt_pairs_kernel(const float4* __restrict__ model, const float4* __restrict__ refs, const int32_t* __restrict__ group,
                                                         const int32_t* __restrict__ rowidx, const int32_t* __restrict__ nrows, int32_t* __restrict__ num,
                                                         int32_t* __restrict__ den, int64_t units, int S, int L, int nb, int nrc, float cutoff) {
    const int64_t u = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (u >= units) return;                                                     // wave-uniform
    const int lane = threadIdx.x & 63, slice = blockIdx.z, slices = gridDim.z, njt = (L + 63) / 64;
    int64_t c, g;                                                               // grouped: the candidate; ensemble: the reference structure g S + a
    int b0 = 0, rc_only = 0;
    if (ENS) { c = u / nb; b0 = (int)(u % nb) * B; g = c / S; } else { c = u / nrc; rc_only = (int)(u % nrc); g = c / S; }
    const float4* ref = ENS ? model + c * L : refs + g * L;
    const float4* mod[B];
    bool have[B];
#pragma unroll
    for (int k = 0; k < B; ++k) {
        have[k] = !ENS || b0 + k < S;
        mod[k] = ENS ? model + (g * S + (have[k] ? b0 + k : S - 1)) * L : model + c * L;
    }
    const int32_t* grp = group ? group + g * L : nullptr;
    const int32_t* ridx = rowidx + g * L;
    const int nr = nrows[g];
    const float qnan = __uint_as_float(0x7fc00000u);
    int n[B], d[B];
#pragma unroll
    for (int k = 0; k < B; ++k) n[k] = d[k] = 0;
    int row_i = -1;                                                             // grouped: the lane's row, for the store

    const int first = ENS ? slice : rc_only * njt + slice, last = ENS ? nrc * njt : (rc_only + 1) * njt;
    for (int w = first; w < last; w += slices) {
        const int rc = w / njt, jt = w % njt;
        if (rc * 64 >= nr) break;                                               // wave-uniform: the chunks beyond the scored rows
        const int r = rc * 64 + lane;
        const bool live = r < nr;
        const int i = live ? ridx[r] : 0;
        if (live) row_i = i;
        const float4 ri = ref[i];
        int want = -2;
        if (live) {
            const int gi = grp ? grp[i] : 0;
            want = grp ? (gi == 1 ? 2 : gi == 2 ? 1 : -2) : 0;
        }
        float4 mi[B];
        unsigned ibits = 0u;
#pragma unroll
        for (int k = 0; k < B; ++k) {
            mi[k] = mod[k][i];
            ibits |= (have[k] && mi[k].w != 0.f ? 1u : 0u) << k;
        }
        const int j = jt * 64 + lane;
        const bool jl = j < L;
        const float4 rj = jl ? ref[j] : make_float4(qnan, qnan, qnan, 0.f);
        float4 mj[B];
        unsigned fj = 0u;
#pragma unroll
        for (int k = 0; k < B; ++k) {
            mj[k] = jl ? mod[k][j] : make_float4(qnan, qnan, qnan, 0.f);
            fj |= (mj[k].w != 0.f ? 1u : 0u) << k;
        }
        if (grp && jl) {
            const int gj = grp[j];
            fj |= (gj == 1 || gj == 2 ? (unsigned)gj : 0u) << 8;
        }
        const int jn = min(64, L - jt * 64);
        for (int jj = 0; jj < jn; ++jj) {
            const unsigned f = (unsigned)__builtin_amdgcn_readlane((int)fj, jj);
            const float dt = ld_dist(ri.x, ri.y, ri.z, ld_lane(rj.x, jj), ld_lane(rj.y, jj), ld_lane(rj.z, jj));
            const bool scored = dt < cutoff && (int)(f >> 8) == want && jt * 64 + jj != i;
            const unsigned ok = scored ? (ibits & f) : 0u;
            if (__ballot(ok != 0u) == 0ull) continue;                           // wave-uniform: residue j is beyond the cutoff of all 64 rows (a chain is local)
#pragma unroll
            for (int k = 0; k < B; ++k) {
                const float dp = ld_dist(mi[k].x, mi[k].y, mi[k].z, ld_lane(mj[k].x, jj), ld_lane(mj[k].y, jj), ld_lane(mj[k].z, jj));
                const float e = fabsf(__fsub_rn(dt, dp));                       // a NaN dp: e is NaN, no hit, and the pair still counts
                const int hits = (e < 0.5f ? 1 : 0) + (e < 1.f ? 1 : 0) + (e < 2.f ? 1 : 0) + (e < 4.f ? 1 : 0);
                const bool o = (ok >> k) & 1u;
                d[k] += o ? 1 : 0;
                n[k] += o ? hits : 0;
            }
        }
    }
    if (ENS) {
#pragma unroll
        for (int k = 0; k < B; ++k) {
            int ns = n[k], ds = d[k];
            for (int off = 32; off > 0; off >>= 1) { ns += __shfl_xor(ns, off, 64); ds += __shfl_xor(ds, off, 64); }
            if (lane == 0 && have[k] && ds) {
                const int64_t o = c * S + b0 + k;
                atomicAdd(&den[o], ds);
                if (ns) atomicAdd(&num[o], ns);
            }
        }
    } else if (row_i >= 0 && d[0]) {
        atomicAdd(&den[c * L + row_i], d[0]);
        if (n[0]) atomicAdd(&num[c * L + row_i], n[0]);
    }
}

// packed CA of the G S candidates | of the G references | compacted rows [G][L] | their number [G]
size_t lddt_ws_bytes(int G, int S, int L) {
    if (G <= 0 || S <= 0 || L <= 0) return 0;
    return ((size_t)G * S + G) * L * 16 + (size_t)G * L * 4 + (size_t)G * 4;
}

// ref_pos == nullptr: the ensemble form (num / den [G][S][S]); else the grouped form (num / den [G S][L]).  Arguments are checked by the callers (api.hip).
int launch_lddt(const float* pos, const uint8_t* mask, int mask_shared, const float* ref_pos, const uint8_t* ref_mask, const uint8_t* rows,
                const int32_t* group, int G, int S, int L, int A, float cutoff, int32_t* num, int32_t* den, void* ws, hipStream_t st) {
    const bool ens = ref_pos == nullptr;
    const int64_t N = (int64_t)G * S;
    float4* model = (float4*)ws;
    float4* ref = model + (size_t)N * L;
    int32_t* rowidx = (int32_t*)(ref + (size_t)G * L);
    int32_t* nrows = rowidx + (size_t)G * L;
    int cus = 0;
    int rc = device_cu_count(&cus);
    if (rc != ABOPT_OK) return rc;
    const size_t nout = ens ? (size_t)N * S : (size_t)N * L;
    const size_t work = std::max(nout, ((size_t)N + G) * L);
    const size_t prep_blocks = std::max<size_t>(std::min<size_t>((work + 255) / 256, 4096), 1);
    hipLaunchKernelGGL(lddt_prep_kernel, dim3((unsigned)prep_blocks), dim3(256), 0, st, pos, mask, mask_shared ? 1 : 0, ref_pos, ref_mask, rows, model, ref,
                       rowidx, nrows, num, den, nout, N, G, S, L, A);
    ABOPT_LAUNCH_CHECK();
    const int nrc = (L + 63) / 64, njt = nrc, nb = (S + LD_B - 1) / LD_B;
    const int64_t units = ens ? N * nb : N * nrc;
    const int64_t split = ens ? (int64_t)nrc * njt : njt;
    // sixteen waves per CU, if the shape has them: a unit's tiles are split over up to 64 workgroups
    const int slices = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(LD_MAX_SLICES, split), ((int64_t)cus * 16 + units - 1) / units));
    const int64_t blocks = (units + 3) / 4, x = std::min<int64_t>(blocks, LD_GRID_X);
    const dim3 grid((unsigned)x, (unsigned)((blocks + x - 1) / x), (unsigned)slices);
    if (ens)
        hipLaunchKernelGGL((lddt_pairs_kernel<LD_B, true>), grid, dim3(256), 0, st, model, ref, group, rowidx, nrows, num, den, units, S, L, nb, nrc, cutoff);
    else
        hipLaunchKernelGGL((lddt_pairs_kernel<1, false>), grid, dim3(256), 0, st, model, ref, group, rowidx, nrows, num, den, units, S, L, nb, nrc, cutoff);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}

}  // namespace abopt
