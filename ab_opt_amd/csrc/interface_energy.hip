// Interface energetics of docked candidates on the device: what the contacts across an interface ARE, chemically.  Per residue of either
// side, summed over its partners on the other side: backbone hydrogen bonds by the DSSP rule (Kabsch & Sander 1983), a Coulomb term between charged residue
// centres with the distance-dependent dielectric eps r, and a caller's residue-pair table inside a contact radius -- three fp32 energies and five integer counts.
// One entry point, one launch, nothing allocated, nothing synchronised, no atomic, no memset node, every output written whole by plain stores.
// Nothing in the reference is matched (it ranks by Rosetta's dG_separated); the definition is this library's own (include/abopt.h:
// abopt_interface_energy_grouped) and numpy restates it bit for bit (tests/interface_energy_statement.py).
#include <math.h>
#include <algorithm>
#include "abopt_common.h"
#include "candidate_common.h"

// Every fp32 step of this file is rounded once and nothing may be contracted into an fma (section 6.6, "Every step rounded once": __fadd_rn and its kin carry the
// permission to contract with them).  So the steps are spelled ie_add / ie_sub / ie_mul / ie_div below, compiled under contract(off).  The division and sqrtf are
// the compiler's correctly rounded ones (hipcc's default; the Makefile does not change it).  d2_fma of candidate_common.h is not for this file.
#pragma clang fp contract(off)

namespace abopt {

constexpr int IE_T = 64;                   // residues staged at a time = owners of a tile = lanes of the workgroup's one wave
constexpr int IE_TYPES = 21;               // the twenty types and "no type"
constexpr int IE_PRO = 12;                 // model.AA_LETTERS = 'ACDEFGHIKLMNPQRSTVWY'
constexpr float IE_Q = 27.888f;            // 0.42 e x 0.20 e x 332 kcal A / (mol e^2)
constexpr float IE_CLAMP = -9.9f;
constexpr float IE_COULOMB = 332.0637f;
// the bits of a staged residue: which of its atoms take part, whether it has an amide hydrogen / a centre, whether the step to r + 1 is bonded; its side in bits
// 8-9 (0 for a lane that owns nothing)
enum : int { IE_N = 1, IE_CA = 2, IE_C = 4, IE_O = 8, IE_H = 16, IE_X = 32, IE_LINK = 64, IE_SIDE = 8, IE_TYPE = 16 };

__device__ __forceinline__ float ie_add(float a, float b) { return a + b; }
__device__ __forceinline__ float ie_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float ie_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float ie_div(float a, float b) { return a / b; }

struct ie_vec { float x, y, z; };

// d2 = (dx dx + dy dy) + dz dz, every step rounded once, in this association; (x - y)^2 == (y - x)^2, so d2(p, q) == d2(q, p) bit for bit
__device__ __forceinline__ float ie_d2(ie_vec a, ie_vec b) {
    const float dx = ie_sub(a.x, b.x), dy = ie_sub(a.y, b.y), dz = ie_sub(a.z, b.z);
    return ie_add(ie_add(ie_mul(dx, dx), ie_mul(dy, dy)), ie_mul(dz, dz));
}

// the ONE rule of which atoms take part (include/abopt.h): mask byte set, three finite coordinates
__device__ __forceinline__ bool ie_atom(const float* __restrict__ pos, const uint8_t* __restrict__ mask, int r, int A, int slot, ie_vec& v) {
    const float* x = pos + ((int64_t)r * A + slot) * 3;
    v.x = x[0]; v.y = x[1]; v.z = x[2];
    return mask[(int64_t)r * A + slot] && finite_f32(v.x) && finite_f32(v.y) && finite_f32(v.z);
}

struct ie_res {
    ie_vec n, ca, c, o, h, x;              // N, CA, C, O, the constructed amide hydrogen, the centre (CB, else CA)
    float q;                               // charge[type]; 0 for a NaN entry
    int bits, idx;
};

// Residue r of a candidate (side 1 or 2), everything a pair term reads.  H = N_r + (C_{r-1} - O_{r-1}) / |C_{r-1} - O_{r-1}| is built here, once, from the
// previous residue in global memory -- which need not be on a side.
__device__ __forceinline__ ie_res ie_residue(const float* __restrict__ pos, const uint8_t* __restrict__ mask, const int32_t* __restrict__ grp,
                                             const uint8_t* __restrict__ seq, const uint8_t* __restrict__ link, const float* __restrict__ charge, int r, int A) {
    ie_res v;
    const int t = min((int)seq[r], IE_TYPES - 1);
    int bits = (grp[r] << IE_SIDE) | (t << IE_TYPE);
    if (ie_atom(pos, mask, r, A, 0, v.n)) bits |= IE_N;
    if (ie_atom(pos, mask, r, A, 1, v.ca)) bits |= IE_CA;
    if (ie_atom(pos, mask, r, A, 2, v.c)) bits |= IE_C;
    if (ie_atom(pos, mask, r, A, 3, v.o)) bits |= IE_O;
    v.x = v.ca;
    if (bits & IE_CA) bits |= IE_X;
    if (A >= 5) {
        ie_vec cb;
        if (ie_atom(pos, mask, r, A, 4, cb)) { v.x = cb; bits |= IE_X; }
    }
    if (link == nullptr || link[r]) bits |= IE_LINK;
    v.h = v.n;
    if (r >= 1 && (link == nullptr || link[r - 1]) && t != IE_PRO && (bits & IE_N)) {
        ie_vec pc, po;
        if (ie_atom(pos, mask, r - 1, A, 2, pc) && ie_atom(pos, mask, r - 1, A, 3, po)) {
            const float ux = ie_sub(pc.x, po.x), uy = ie_sub(pc.y, po.y), uz = ie_sub(pc.z, po.z);
            const float len = sqrtf(ie_add(ie_add(ie_mul(ux, ux), ie_mul(uy, uy)), ie_mul(uz, uz)));
            if (len > 0.f) {
                v.h.x = ie_add(v.n.x, ie_div(ux, len));
                v.h.y = ie_add(v.n.y, ie_div(uy, len));
                v.h.z = ie_add(v.n.z, ie_div(uz, len));
                bits |= IE_H;
            }
        }
    }
    const float q = charge[t];
    v.q = q == q ? q : 0.f;                                                    // a NaN entry takes the type out
    v.bits = bits;
    v.idx = r;
    return v;
}

// The DSSP energy of donor (N, H) and acceptor (C, O): 27.888 (((1 / r_ON + 1 / r_CH) - 1 / r_OH) - 1 / r_CN), -9.9 if a distance is below 0.5 A, never below -9.9
__device__ __forceinline__ float ie_hbond(ie_vec n, ie_vec h, ie_vec c, ie_vec o) {
    const float r_on = sqrtf(ie_d2(o, n)), r_ch = sqrtf(ie_d2(c, h)), r_oh = sqrtf(ie_d2(o, h)), r_cn = sqrtf(ie_d2(c, n));
    if (r_on < 0.5f || r_ch < 0.5f || r_oh < 0.5f || r_cn < 0.5f) return IE_CLAMP;
    const float e = ie_mul(IE_Q, ie_sub(ie_sub(ie_add(ie_div(1.f, r_on), ie_div(1.f, r_ch)), ie_div(1.f, r_oh)), ie_div(1.f, r_cn)));
    return e < IE_CLAMP ? IE_CLAMP : e;
}

struct ie_knobs { float hb_cutoff, elec2, salt2, pair2, eps, dmin2; };

// Grid (candidate folded over x and y, slice in z), ONE wave per workgroup, a lane per owner residue.  The participating residues of the candidate (side 1 or
// 2) are numbered in index order and slice s owns the ranks [np s / slices, np (s + 1) / slices): the re-dock shape has fewer candidates than the chip has CUs.
// Per tile of up to 64 owners -- each lane keeps ITS residue in registers -- the wave walks ALL participating residues of the candidate in index order, staged
// through LDS 64 at a time as six float4 (N + charge, CA + bits, C + index, O, H, centre): per partner a few broadcast reads (every lane reads the same
// address: no bank conflict), the side and bonded-neighbour tests, the 9 A CA rule, up to two DSSP energies, the centre distance and its three cutoffs.  Every
// lane adds by itself, in ascending j, donor before acceptor; nothing is reduced across lanes, so no order but the definition's exists.  No prune beyond the
// definition's own exact tests.  The pair table, if given, is staged in LDS once (row stride 21, odd).  Slice 0 also writes the zeros of the residues on no side.
__global__ __launch_bounds__(IE_T) void interface_energy_kernel(const float* __restrict__ pos_all, const uint8_t* __restrict__ mask_all, int mask_shared,
                                                                const int32_t* __restrict__ group_all, const uint8_t* __restrict__ seq_all, int seq_shared,
                                                                const uint8_t* __restrict__ link_all, const float* __restrict__ charge,
                                                                const float* __restrict__ table, ie_knobs kn, int64_t N, int S, int L, int A,
                                                                float* __restrict__ energy_all, int32_t* __restrict__ count_all) {
    __shared__ __attribute__((aligned(16))) float4 p_n[IE_T], p_ca[IE_T], p_c[IE_T], p_o[IE_T], p_h[IE_T], p_x[IE_T];
    __shared__ float tab[IE_TYPES * IE_TYPES];
    __shared__ int idx_t[IE_T], idx_o[IE_T];
    const int64_t c = folded_block();
    if (c >= N) return;                                                         // the last row of a folded grid; block-uniform
    const int64_t g = c / S;
    const int lane = threadIdx.x, slice = blockIdx.z, slices = gridDim.z;
    const float* pos = pos_all + c * L * A * 3;
    const uint8_t* mask = mask_all + (mask_shared ? g : c) * L * A;
    const int32_t* grp = group_all + g * L;
    const uint8_t* seq = seq_all + (seq_shared ? g : c) * L;
    const uint8_t* link = link_all ? link_all + g * L : nullptr;
    float* energy = energy_all + c * L * 3;
    int32_t* count = count_all + c * L * 5;
    const OnEitherSide part{grp};

    if (slice == 0) {
        for (int r = lane; r < L; r += IE_T)
            if (!part(r)) {
                for (int k = 0; k < 3; ++k) energy[(int64_t)r * 3 + k] = 0.f;
                for (int k = 0; k < 5; ++k) count[(int64_t)r * 5 + k] = 0;
            }
    }
    int cur_t;
    int left = slice_ranks(L, part, slice, slices, cur_t);
    if (left == 0) return;                                                      // block-uniform
    if (table) for (int k = lane; k < IE_TYPES * IE_TYPES; k += IE_T) tab[k] = table[k];

    while (left > 0) {
        __syncthreads();                                                        // the previous tile's reads of idx_t are done
        const int ntt = take(L, part, cur_t, min(IE_T, left), idx_t, true);
        left -= ntt;
        if (ntt == 0) break;                                                    // cannot happen (the ranks were counted on the same row); block-uniform
        __syncthreads();
        ie_res me;
        me.bits = 0;                                                            // side 0: a lane that owns nothing meets no partner
        me.idx = -2;
        me.q = 0.f;
        if (lane < ntt) me = ie_residue(pos, mask, grp, seq, link, charge, idx_t[lane], A);
        const int my_side = (me.bits >> IE_SIDE) & 3, my_type = (me.bits >> IE_TYPE) & 31;
        float e_hb = 0.f, e_el = 0.f, e_pr = 0.f;
        int n_don = 0, n_acc = 0, n_salt = 0, n_like = 0, n_near = 0;

        int cur_o = 0;
        while (true) {
            __syncthreads();                                                    // the previous partner tile's reads are done
            const int nto = take(L, part, cur_o, IE_T, idx_o, true);
            if (nto == 0) break;                                                // block-uniform
            __syncthreads();
            if (lane < nto) {
                const ie_res v = ie_residue(pos, mask, grp, seq, link, charge, idx_o[lane], A);
                p_n[lane] = make_float4(v.n.x, v.n.y, v.n.z, v.q);
                p_ca[lane] = make_float4(v.ca.x, v.ca.y, v.ca.z, __int_as_float(v.bits));
                p_c[lane] = make_float4(v.c.x, v.c.y, v.c.z, __int_as_float(v.idx));
                p_o[lane] = make_float4(v.o.x, v.o.y, v.o.z, 0.f);
                p_h[lane] = make_float4(v.h.x, v.h.y, v.h.z, 0.f);
                p_x[lane] = make_float4(v.x.x, v.x.y, v.x.z, 0.f);
            }
            __syncthreads();
            for (int j = 0; j < nto; ++j) {
                const float4 a = p_ca[j], cc = p_c[j];                          // broadcast reads
                const int bj = __float_as_int(a.w), rj = __float_as_int(cc.w);
                if (my_side + ((bj >> IE_SIDE) & 3) != 3) continue;             // the same side, or this lane owns nothing
                if ((rj == me.idx + 1 && (me.bits & IE_LINK)) || (rj + 1 == me.idx && (bj & IE_LINK))) continue;      // bonded neighbours
                const ie_vec ca_j{a.x, a.y, a.z}, c_j{cc.x, cc.y, cc.z};
                if ((me.bits & bj & IE_CA) && ie_d2(me.ca, ca_j) < 81.f) {
                    const float4 nn = p_n[j], oo = p_o[j];
                    if ((me.bits & IE_H) && (bj & (IE_C | IE_O)) == (IE_C | IE_O)) {                // the owner donates to j
                        const float e = ie_hbond(me.n, me.h, c_j, ie_vec{oo.x, oo.y, oo.z});
                        if (e < kn.hb_cutoff) { e_hb = ie_add(e_hb, e); ++n_don; }
                    }
                    if ((bj & IE_H) && (me.bits & (IE_C | IE_O)) == (IE_C | IE_O)) {                // the owner accepts from j
                        const float4 hh = p_h[j];
                        const float e = ie_hbond(ie_vec{nn.x, nn.y, nn.z}, ie_vec{hh.x, hh.y, hh.z}, me.c, me.o);
                        if (e < kn.hb_cutoff) { e_hb = ie_add(e_hb, e); ++n_acc; }
                    }
                }
                if (me.bits & bj & IE_X) {
                    const float4 xx = p_x[j];
                    const float d2 = ie_d2(me.x, ie_vec{xx.x, xx.y, xx.z});
                    const float qj = p_n[j].w;
                    if (me.q != 0.f && qj != 0.f && d2 <= kn.elec2) {
                        const float qq = ie_mul(me.q, qj);
                        e_el = ie_add(e_el, ie_div(ie_mul(IE_COULOMB, qq), ie_mul(kn.eps, fmaxf(d2, kn.dmin2))));
                        if (d2 <= kn.salt2) { n_salt += qq < 0.f; n_like += qq > 0.f; }
                    }
                    if (d2 <= kn.pair2) {
                        ++n_near;
                        if (table) {
                            const float w = tab[my_type * IE_TYPES + ((bj >> IE_TYPE) & 31)];
                            if (w == w) e_pr = ie_add(e_pr, w);                 // a NaN entry adds nothing
                        }
                    }
                }
            }
            if (nto < IE_T) break;                                              // the row ended inside this tile; block-uniform
        }
        if (lane < ntt) {
            float* e = energy + (int64_t)me.idx * 3;
            int32_t* n = count + (int64_t)me.idx * 5;
            e[0] = e_hb; e[1] = e_el; e[2] = e_pr;
            n[0] = n_don; n[1] = n_acc; n[2] = n_salt; n[3] = n_like; n[4] = n_near;
        }
    }
}

}  // namespace abopt

using namespace abopt;

extern "C" int abopt_interface_energy_grouped(const float* pos, const uint8_t* mask, int mask_shared, const int32_t* group, const uint8_t* seqs, int seq_shared,
                                              const uint8_t* link, const float* charge, const float* pair_table, int G, int S, int L, int A, float hb_cutoff,
                                              float elec_cutoff, float salt_cutoff, float pair_cutoff, float eps, float d_min, void* energy, void* count,
                                              abopt_stream stream) {
    const char* name = "interface_energy_grouped";
    int rc = check_candidate_dims(name, G, S, L, A);
    if (rc != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(A >= 4, "interface_energy_grouped: A=%d atoms per residue, the slots 0 .. 3 are N, CA, C, O (expected 4 .. %d)", A, kMaxAtoms);
    ABOPT_CHECK_ARG(isfinite(hb_cutoff) && hb_cutoff <= 0.f, "interface_energy_grouped: hb_cutoff must be finite and <= 0 (got %g)", (double)hb_cutoff);
    static const char* const names[] = {"elec_cutoff", "salt_cutoff", "pair_cutoff", "eps", "d_min"};
    const float v[] = {elec_cutoff, salt_cutoff, pair_cutoff, eps, d_min};
    if ((rc = check_nonnegative(name, names, v, 5)) != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(eps > 0.f && d_min > 0.f, "interface_energy_grouped: eps and d_min must be > 0 (got eps=%g, d_min=%g)", (double)eps, (double)d_min);
    if (G == 0 || S == 0) return ABOPT_OK;
    if ((rc = check_group_count(name, G)) != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(pos && mask && group && seqs && charge && energy && count, "interface_energy_grouped: NULL argument");
    const int64_t N = (int64_t)G * S;
    // each squared once, in fp32; +inf for a huge cutoff: every pair with both centres is inside
    const ie_knobs kn{hb_cutoff, elec_cutoff * elec_cutoff, salt_cutoff * salt_cutoff, pair_cutoff * pair_cutoff, eps, d_min * d_min};
    int cus = 0;
    if ((rc = device_cu_count(&cus)) != ABOPT_OK) return rc;
    // one wave per workgroup: enough of them for eight per CU, no slice thinner than one tile of 64 owners
    const int slices = slice_count(cus, 8, N, ((int64_t)L + IE_T - 1) / IE_T);
    hipLaunchKernelGGL(interface_energy_kernel, fold_grid(N, (unsigned)slices), dim3(IE_T), 0, (hipStream_t)stream, pos, mask, mask_shared ? 1 : 0, group, seqs,
                       seq_shared ? 1 : 0, link, charge, pair_table, kn, N, S, L, A, (float*)energy, (int32_t*)count);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}
