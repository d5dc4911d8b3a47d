// Interface geometry of docked candidates on the device: steric clashes across the interface, the size of the interface in
// residue contacts, the residues of either side in a contact (per candidate, and per group as the consensus epitope) and broken peptide bonds.
// Nothing in the reference is matched: its only physical check is the relax stage this project does not have.  The definition is this library's own
// (include/abopt.h: abopt_interface_geometry_grouped); all results are integer counts, so no reduction order can change them.
// Three launches: interface_clear_kernel zeroes the workspace and freq, interface_pairs_kernel walks the pairs (side-1 residue, side-2 residue) of a candidate and leaves three counters and one bit per residue
// ("in at least one contact") in the workspace; interface_count_kernel counts the bits into iface1 / iface2 / freq and writes the five outputs.
#include <math.h>
#include <algorithm>
#include "abopt_common.h"
#include "candidate_common.h"
#include "kernels.h"

namespace abopt {

constexpr int IG_T1 = 16;                  // side-1 residues staged at a time: 4 per wave
constexpr int IG_T2 = 64;                  // side-2 residues staged at a time: one per lane
constexpr int IG_WS_COUNTERS = 4;          // int32 per candidate behind its bit row: clash, contacts, breaks, (pad)

// Bounding sphere of one residue from its staged atoms (masked-out atoms are NaN there and are told apart by the mask word `m`): centre = mean of the masked
// atoms, radius = the largest d2_fma distance from that centre.  No atoms: radius -inf, which the prune below always skips.  A NaN coordinate makes centre
// and radius NaN, which the prune never skips (every comparison with NaN is false).
__device__ __forceinline__ float4 ig_sphere(const float* __restrict__ atoms, int stride, int A, unsigned m) {
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int p = 0; p < A; ++p)
        if ((m >> p) & 1u) { sx += atoms[p * stride]; sy += atoms[p * stride + 1]; sz += atoms[p * stride + 2]; }
    if (m == 0u) return make_float4(0.f, 0.f, 0.f, -INFINITY);
    const float inv = 1.f / (float)__popc(m);
    const float cx = sx * inv, cy = sy * inv, cz = sz * inv;
    float r2 = 0.f;
    for (int p = 0; p < A; ++p)
        if ((m >> p) & 1u) {
            const float d2 = d2_fma(cx, cy, cz, atoms[p * stride], atoms[p * stride + 1], atoms[p * stride + 2]);
            r2 = d2 > r2 ? d2 : (d2 == d2 ? r2 : d2);                          // a NaN distance sticks
        }
    return make_float4(cx, cy, cz, sqrtf(r2));
}

// Grid (candidate folded over x and y, slice in z), 4 waves.  The side-1 residues of the candidate are numbered in index order and slice s takes the ranks
// [n1 s / slices, n1 (s + 1) / slices): the re-dock shape has fewer candidates than the chip has CUs.  Per workgroup:
//   side-1 tile   up to 16 residues of the slice: indices compacted by ballots (take, candidate_common.h), atoms staged in LDS as float4 (masked-out atoms as NaN: they
//                 drop out of every comparison below, like a NaN coordinate does by definition), mask words and bounding spheres next to them
//   side-2 tile   up to 64 residues, compacted likewise, atoms staged with an odd stride, spheres; then every lane holds ITS residue's atoms in registers
//   pairs         a wave owns one side-1 residue at a time (4 per tile) against the 64 lanes.  Prune: the pair is entered unless the spheres prove that no atom
//                 pair can reach the larger cutoff (below); a link-bonded neighbour pair is skipped by definition.  The A x A loop reads the side-1 atom as one
//                 broadcast LDS read and keeps the running minimum and the clash count in registers.  __ballot of (minimum <= contact^2) is the row of
//                 contacts of the side-1 residue in this tile: its population goes to `contacts`, its bits mark the side-2 residues, any bit marks the side-1 one.
//   marks         one atomicOr per marked residue into the candidate's bit row in the workspace; counters by one atomicAdd per wave.
// LDS: 3.8 KB + 11.5 KB of atoms + 1.7 KB of indices, masks and spheres, whatever L is.
//
// The prune is conservative in fp32.  Every distance here is d2_fma (candidate_common.h) between two fp32 POINTS followed (for the spheres) by sqrtf: the subtraction of two fp32
// numbers is rounded once, relative to the difference (u = 2^-24) whatever the magnitude of the coordinates, the square and the two fmas add three more
// roundings of non-negative terms, so a computed d2 is the true one x (1 +- 5 u) and a computed distance the true one x (1 +- 4 u).  The centre is whatever
// fp32 point the mean rounds to -- the radius is measured from THAT point, so the mean's own rounding costs tightness, not correctness.  For atoms p of a, q of b
// the triangle inequality gives |p - q| >= D - ra - rb (true values).  The pair is skipped iff  D^ > (ra^ + rb^ + cut) (1 + 2^-16) + 0.01  with the computed
// D^, ra^, rb^ and cut = max(clash_d, contact_d): D >= D^ (1 - 4 u), ra + rb + cut <= (ra^ + rb^ + cut) (1 + 6 u) (two more additions), and 2^-16 = 256 u, so
// a skipped pair has D - ra - rb > cut (1 + 240 u) while an atom pair that passes d2^ <= fl(cut^2) has |p - q| <= cut (1 + 4 u).  The 0.01 A on top is ten ulps of
// a coordinate of 10^4 A (2^-10 A each): it would cover a centre whose arithmetic were off by that much in absolute terms; it costs no measurable pruning.
template <int AQ>
__global__ __launch_bounds__(256) void interface_pairs_kernel(const float* __restrict__ pos_all, const uint8_t* __restrict__ mask_all, int mask_shared,
                                                              const int32_t* __restrict__ group_all, const uint8_t* __restrict__ link_all,
                                                              unsigned* __restrict__ ws_all, int N, int S, int L, int A, int ws_stride, float thr_clash,
                                                              float thr_contact, float cut_max, float thr_bond, int count_breaks) {
    constexpr int S2 = AQ * 3 + ((AQ * 3) % 2 == 0 ? 1 : 0);                    // odd: lane j reads word j S2 + e, conflict-free
    __shared__ __attribute__((aligned(16))) float4 at1[IG_T1][AQ];
    __shared__ float at2[IG_T2][S2];
    __shared__ __attribute__((aligned(16))) float4 sph1[IG_T1];
    __shared__ __attribute__((aligned(16))) float4 sph2[IG_T2];
    __shared__ int idx1[IG_T1], idx2[IG_T2];
    __shared__ unsigned msk1[IG_T1];
    const int64_t c64 = folded_block();
    if (c64 >= N) return;                                                       // the last row of a folded grid; block-uniform
    const int c = (int)c64, slice = blockIdx.z, slices = gridDim.z, g = c / S;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* pos = pos_all + (int64_t)c * L * A * 3;
    const uint8_t* mask = mask_all + (int64_t)(mask_shared ? g : c) * L * A;
    const int32_t* grp = group_all + (int64_t)g * L;
    const uint8_t* link = link_all ? link_all + (int64_t)g * L : nullptr;
    unsigned* bits = ws_all + (int64_t)c * ws_stride;
    int* counters = (int*)(bits + (ws_stride - IG_WS_COUNTERS));
    const float qnan = __uint_as_float(0x7fc00000u);

    // ---- broken peptide bonds: slice 0, straight from global memory (L - 1 candidates for a test, two atoms each)
    if (slice == 0 && link && count_breaks) {
        int nb = 0;
        for (int r0 = 0; r0 < L - 1; r0 += 256) {
            const int r = r0 + tid;
            bool brk = false;
            if (r < L - 1 && link[r] && mask[(int64_t)r * A + 2] && mask[(int64_t)(r + 1) * A]) {
                const float* cp = pos + ((int64_t)r * A + 2) * 3;
                const float* np_ = pos + (int64_t)(r + 1) * A * 3;
                brk = !(d2_fma(cp[0], cp[1], cp[2], np_[0], np_[1], np_[2]) <= thr_bond);      // a NaN coordinate is a break
            }
            nb += __popcll(__ballot(brk));
        }
        if (lane == 0 && nb) atomicAdd(&counters[2], nb);
    }

    // ---- this slice's ranks of side-1 residues (every wave counts the row itself: wave-uniform, no exchange)
    const OnSide side1{grp, 1}, side2{grp, 2};
    int cur1;
    int left = slice_ranks(L, side1, slice, slices, cur1);
    if (left == 0) return;                                                      // block-uniform

    int clash = 0, contacts = 0;                                                // clash: per lane; contacts: wave-uniform
    while (left > 0) {
        __syncthreads();                                                        // the previous tile's reads are done
        const int n1t = take(L, side1, cur1, min(IG_T1, left), idx1, wave == 0);
        left -= n1t;
        if (n1t == 0) break;                                                    // cannot happen (the ranks were counted on the same row); block-uniform
        __syncthreads();
        for (int t = tid; t < n1t * AQ; t += 256) {
            const int i = t / AQ, p = t % AQ, r = idx1[i];
            const bool ok = p < A && mask[(int64_t)r * A + p];
            const float* x = pos + ((int64_t)r * A + p) * 3;
            at1[i][p] = ok ? make_float4(x[0], x[1], x[2], 0.f) : make_float4(qnan, qnan, qnan, 0.f);
        }
        if (tid < n1t) {
            unsigned m = 0u;
            for (int p = 0; p < A; ++p) m |= (mask[(int64_t)idx1[tid] * A + p] ? 1u : 0u) << p;
            msk1[tid] = m;
        }
        __syncthreads();
        if (tid < n1t) sph1[tid] = ig_sphere((const float*)&at1[tid][0], 4, A, msk1[tid]);

        int cur2 = 0;
        while (true) {
            __syncthreads();                                                    // the previous side-2 tile's reads are done (and sph1 is written)
            const int n2t = take(L, side2, cur2, IG_T2, idx2, wave == 0);
            if (n2t == 0) break;                                                // block-uniform
            __syncthreads();
            for (int t = tid; t < n2t * (AQ * 3); t += 256) {
                const int j = t / (AQ * 3), e = t % (AQ * 3), r = idx2[j];
                const bool ok = e < A * 3 && mask[(int64_t)r * A + e / 3];
                at2[j][e] = ok ? pos[(int64_t)r * A * 3 + e] : qnan;
            }
            __syncthreads();
            if (tid < n2t) {
                unsigned m = 0u;
                for (int p = 0; p < A; ++p) m |= (mask[(int64_t)idx2[tid] * A + p] ? 1u : 0u) << p;
                sph2[tid] = ig_sphere(&at2[tid][0], 3, A, m);
            }
            __syncthreads();
            const bool live = lane < n2t;
            const int b = live ? idx2[lane] : -1;
            const float4 sb = live ? sph2[lane] : make_float4(0.f, 0.f, 0.f, -INFINITY);
            float bx[AQ], by[AQ], bz[AQ];
#pragma unroll
            for (int q = 0; q < AQ; ++q) {
                bx[q] = live ? at2[lane][q * 3] : qnan;
                by[q] = live ? at2[lane][q * 3 + 1] : qnan;
                bz[q] = live ? at2[lane][q * 3 + 2] : qnan;
            }
            unsigned long long hit2 = 0ull;                                     // wave-uniform: lanes (side-2 residues of the tile) in a contact
            for (int i = wave; i < n1t; i += 4) {
                const unsigned m1 = msk1[i];
                if (m1 == 0u) continue;                                         // a residue without atoms contacts nobody
                const int a = idx1[i];
                const float4 sa = sph1[i];
                const float reach = fmaf(__fadd_rn(__fadd_rn(sa.w, sb.w), cut_max), 1.f + 1.52587890625e-5f, 0.01f);
                bool skip = !live || sqrtf(d2_fma(sa.x, sa.y, sa.z, sb.x, sb.y, sb.z)) > reach;
                if (link && live) skip = skip || (b == a + 1 && link[a]) || (a == b + 1 && link[b]);
                if (__ballot(!skip) == 0ull) continue;
                float best = INFINITY;
                if (!skip) {
                    for (int p = 0; p < A; ++p) {
                        if (!((m1 >> p) & 1u)) continue;                        // wave-uniform
                        const float4 pa = at1[i][p];                            // one broadcast read
#pragma unroll
                        for (int q = 0; q < AQ; ++q) {
                            const float d2 = d2_fma(pa.x, pa.y, pa.z, bx[q], by[q], bz[q]);
                            best = fminf(best, d2);                             // a NaN (masked-out or not a number) never lowers it
                            clash += d2 < thr_clash ? 1 : 0;
                        }
                    }
                }
                const unsigned long long row = __ballot(!skip && best <= thr_contact);
                if (row) {
                    contacts += __popcll(row);
                    hit2 |= row;
                    if (lane == 0) atomicOr(&bits[a >> 5], 1u << (a & 31));
                }
            }
            if ((hit2 >> lane) & 1ull) atomicOr(&bits[b >> 5], 1u << (b & 31));
            if (n2t < IG_T2) break;                                             // the row ended inside this tile; block-uniform
        }
    }
    clash = wave_sum_butterfly(clash);
    if (lane == 0) {
        if (clash) atomicAdd(&counters[0], clash);
        if (contacts) atomicAdd(&counters[1], contacts);
    }
}

// One wave per candidate, 4 per workgroup: the marks of the bit row counted by side (each residue once, however many slices marked it), added into the
// group's freq row, and the five outputs stored.
__global__ __launch_bounds__(256) void interface_count_kernel(const unsigned* __restrict__ ws_all, const int32_t* __restrict__ group_all, int32_t* __restrict__ out,
                                                              int32_t* __restrict__ freq, int N, int S, int L, int ws_stride) {
    const int64_t c64 = folded_block() * 4 + (threadIdx.x >> 6);
    const int c = (int)c64, lane = threadIdx.x & 63;
    if (c64 >= N) return;                                                         // wave-uniform
    const int g = c / S;
    const unsigned* bits = ws_all + (int64_t)c * ws_stride;
    const int* counters = (const int*)(bits + (ws_stride - IG_WS_COUNTERS));
    const int32_t* grp = group_all + (int64_t)g * L;
    int i1 = 0, i2 = 0;
    for (int r0 = 0; r0 < L; r0 += 64) {
        const int r = r0 + lane;
        const bool hit = r < L && ((bits[r >> 5] >> (r & 31)) & 1u);
        const int side = hit ? grp[r] : 0;
        i1 += __popcll(__ballot(side == 1));
        i2 += __popcll(__ballot(side == 2));
        if (freq && hit) atomicAdd(&freq[(int64_t)g * L + r], 1);
    }
    if (lane == 0) {
        int32_t* o = out + (int64_t)c * 5;
        o[0] = counters[0]; o[1] = counters[1]; o[2] = i1; o[3] = i2; o[4] = counters[2];
    }
}

// zeroes the workspace (marks and counters) and the optional freq rows: plain vector stores, grid-stride
__global__ __launch_bounds__(256) void interface_clear_kernel(unsigned* __restrict__ ws, size_t nws, unsigned* __restrict__ freq, size_t nfreq) {
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nws; i += step) ws[i] = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nfreq; i += step) freq[i] = 0u;
}

}  // namespace abopt

using namespace abopt;

// per candidate: a bit row of ceil(L / 32) words ("residue in at least one contact") | clash, contacts, breaks, pad (int32)
extern "C" size_t abopt_interface_geometry_ws_bytes(int G, int S, int L) {
    if (G <= 0 || S <= 0 || L <= 0) return 0;
    return (size_t)G * S * (((size_t)L + 31) / 32 + IG_WS_COUNTERS) * 4;
}

extern "C" int abopt_interface_geometry_grouped(const float* pos, const uint8_t* mask, int mask_shared, const int32_t* group, const uint8_t* link,
                                                int G, int S, int L, int A, float clash_d, float contact_d, float bond_max, void* out, void* freq,
                                                void* ws, size_t ws_bytes, abopt_stream stream) {
    int rc = check_candidate_dims("interface_geometry_grouped", G, S, L, A);
    if (rc != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(isfinite(clash_d) && clash_d >= 0.f && isfinite(contact_d) && contact_d >= 0.f,
                    "interface_geometry_grouped: the cutoffs must be finite and >= 0 (got clash %g, contact %g)", (double)clash_d, (double)contact_d);
    ABOPT_CHECK_ARG(isfinite(bond_max), "interface_geometry_grouped: bond_max must be finite (negative: breaks are not counted), got %g", (double)bond_max);
    ABOPT_CHECK_ARG(!link || A >= 3, "interface_geometry_grouped: link needs the backbone atoms N, CA, C (A >= 3, got %d)", A);
    if (G == 0 || S == 0) return ABOPT_OK;
    if ((rc = check_group_count("interface_geometry_grouped", G)) != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(pos && mask && group && out && ws, "interface_geometry_grouped: NULL argument");
    const size_t need = abopt_interface_geometry_ws_bytes(G, S, L);
    if ((rc = check_workspace("interface_geometry_grouped", ws, 4, ws_bytes, need)) != ABOPT_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int N = G * S, ws_stride = (L + 31) / 32 + IG_WS_COUNTERS;
    int cus = 0;
    if ((rc = device_cu_count(&cus)) != ABOPT_OK) return rc;
    // enough workgroups for four per CU, no slice thinner than four residues of the row
    const int slices = slice_count(cus, 4, N, ((int64_t)L + 3) / 4);
    const float thr_clash = clash_d * clash_d, thr_contact = contact_d * contact_d, thr_bond = bond_max * bond_max;   // each rounded once
    const float cut_max = clash_d > contact_d ? clash_d : contact_d;
    const int count_breaks = bond_max >= 0.f ? 1 : 0;
    // cleared by a kernel, so that the chain a caller captures into a graph has no memset node
    const size_t nws = need / 4, nfreq = freq ? (size_t)G * L : 0;
    const size_t clear_blocks = std::min<size_t>((std::max(nws, nfreq) + 255) / 256, 4096);
    hipLaunchKernelGGL(interface_clear_kernel, dim3((unsigned)clear_blocks), dim3(256), 0, st, (unsigned*)ws, nws, (unsigned*)freq, nfreq);
    ABOPT_LAUNCH_CHECK();
    auto kernel = A <= 4 ? interface_pairs_kernel<4> : A <= 8 ? interface_pairs_kernel<8> : interface_pairs_kernel<kMaxAtoms>;
    hipLaunchKernelGGL(kernel, fold_grid(N, (unsigned)slices), dim3(256), 0, st, pos, mask, mask_shared ? 1 : 0, group, link, (unsigned*)ws, N, S, L, A,
                       ws_stride, thr_clash, thr_contact, cut_max, thr_bond, count_breaks);
    ABOPT_LAUNCH_CHECK();
    hipLaunchKernelGGL(interface_count_kernel, fold_grid(((int64_t)N + 3) / 4, 1u), dim3(256), 0, st, (const unsigned*)ws, group, (int32_t*)out, (int32_t*)freq,
                       N, S, L, ws_stride);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}
