// Backbone conformation of candidates on the device: whether a generated backbone is a plausible polypeptide BETWEEN its residues.
// Per scored residue: phi, psi, omega as (cos, sin), the peptide bond's length and its two angles as cosines, a Ramachandran class against a caller's table of
// boxes, cis / twisted peptide flags, and DSSP-LIKE states (Kabsch & Sander's n-turn, helix and bridge patterns on the hydrogen-bond energy of section 6.10,
// here within the candidate) with the lowest bridge partners; per candidate 24 integer counts.  This is NOT DSSP: no ladders or sheets, no B / E distinction,
// no bends, no helix trimming.  One entry point, one launch, nothing allocated, no global atomic, no memset node, every output written whole by plain stores.
// Nothing in the reference is matched; the definition is this library's own (include/abopt.h: abopt_backbone_conformation_grouped) and numpy restates it bit
// for bit (tests/backbone_statement.py).
#include <math.h>
#include <algorithm>
#include "abopt_common.h"
#include "candidate_common.h"

// Every fp32 step of this file is rounded once and nothing may be contracted into an fma (section 6.6, "Every step rounded once").  So the steps are spelled
// bb_add / bb_sub / bb_mul / bb_div below, compiled under contract(off), as interface_energy.hip's and sasa.hip's are.  The division and sqrtf are the
// compiler's correctly rounded ones (hipcc's default; the Makefile does not change it).  d2_fma of candidate_common.h is not for this file.
#pragma clang fp contract(off)

namespace abopt {

constexpr int BB_MAX_ROWS = 512;           // residues of a candidate at most: the hydrogen-bond relation lives in LDS as L x ceil(L / 64) 64-bit words
constexpr int BB_THREADS = 256;
constexpr int BB_MAX_REGIONS = 8;
constexpr int BB_COUNTS = 24;
constexpr int BB_PRO_T = 12, BB_GLY_T = 5; // model.AA_LETTERS = 'ACDEFGHIKLMNPQRSTVWY'
constexpr float BB_Q = 27.888f;            // 0.42 e x 0.20 e x 332 kcal A / (mol e^2)
constexpr float BB_CLAMP = -9.9f;
// the bits of a staged residue: which of its atoms take part, whether it has an amide hydrogen, whether the step to r + 1 is bonded, whether it is a scored row,
// whether it is Pro / Gly
enum : int { BB_N = 1, BB_CA = 2, BB_C = 4, BB_O = 8, BB_H = 16, BB_LINK = 32, BB_ROW = 64, BB_PRO = 128, BB_GLY = 256 };
// the bits of `have`, of `ss`, the codes of `state` (model.SS_LETTERS = 'HEGITC') and the columns of `count`
enum : int { HV_PHI = 1, HV_PSI = 2, HV_OMEGA = 4, HV_LEN = 8, HV_ANG_C = 16, HV_ANG_N = 32 };
enum : int { SS_H4 = 1, SS_H3 = 2, SS_H5 = 4, SS_PAR = 8, SS_ANTI = 16, SS_TURN = 32 };
enum : int { CN_PART = 0, CN_PHIPSI = 1, CN_REGION = 2, CN_OUTLIER = 10, CN_OUTLIER_GLY = 11, CN_OMEGA = 12, CN_CIS = 13, CN_CIS_NONPRO = 14, CN_TWISTED = 15,
             CN_STATE = 16, CN_DONOR = 22, CN_ACCEPTOR = 23 };

__device__ __forceinline__ float bb_add(float a, float b) { return a + b; }
__device__ __forceinline__ float bb_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float bb_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float bb_div(float a, float b) { return a / b; }

struct bb_vec { float x, y, z; };

__device__ __forceinline__ bb_vec bb_vsub(bb_vec a, bb_vec b) { return bb_vec{bb_sub(a.x, b.x), bb_sub(a.y, b.y), bb_sub(a.z, b.z)}; }
// a . b = (ax bx + ay by) + az bz, in this association
__device__ __forceinline__ float bb_dot(bb_vec a, bb_vec b) { return bb_add(bb_add(bb_mul(a.x, b.x), bb_mul(a.y, b.y)), bb_mul(a.z, b.z)); }
// a x b = (ay bz - az by, az bx - ax bz, ax by - ay bx): two products and one difference per component
__device__ __forceinline__ bb_vec bb_cross(bb_vec a, bb_vec b) {
    return bb_vec{bb_sub(bb_mul(a.y, b.z), bb_mul(a.z, b.y)), bb_sub(bb_mul(a.z, b.x), bb_mul(a.x, b.z)), bb_sub(bb_mul(a.x, b.y), bb_mul(a.y, b.x))};
}
// d2 = (dx dx + dy dy) + dz dz on the differences a - b: section 6.10's, bit for bit
__device__ __forceinline__ float bb_d2(bb_vec a, bb_vec b) { const bb_vec d = bb_vsub(a, b); return bb_dot(d, d); }

// the ONE rule of which atoms take part (include/abopt.h): mask byte set, three finite coordinates
__device__ __forceinline__ bool bb_atom(const float* __restrict__ pos, const uint8_t* __restrict__ mask, int r, int A, int slot, bb_vec& v) {
    const float* x = pos + ((int64_t)r * A + slot) * 3;
    v.x = x[0]; v.y = x[1]; v.z = x[2];
    return mask[(int64_t)r * A + slot] && finite_f32(v.x) && finite_f32(v.y) && finite_f32(v.z);
}

// The torsion of four points as (cos, sin), IUPAC sign: b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, n1 = b1 x b2, n2 = b2 x b3, x = n1 . n2,
// y = |b2| (b1 . n2), rho = sqrt(x x + y y), cos = x / rho, sin = y / rho.  -> false (undefined) unless 0 < rho < inf.
__device__ __forceinline__ bool bb_torsion(bb_vec p0, bb_vec p1, bb_vec p2, bb_vec p3, float& c, float& s) {
    const bb_vec b1 = bb_vsub(p1, p0), b2 = bb_vsub(p2, p1), b3 = bb_vsub(p3, p2);
    const bb_vec n1 = bb_cross(b1, b2), n2 = bb_cross(b2, b3);
    const float x = bb_dot(n1, n2);
    const float y = bb_mul(sqrtf(bb_dot(b2, b2)), bb_dot(b1, n2));
    const float rho = sqrtf(bb_add(bb_mul(x, x), bb_mul(y, y)));
    if (!(rho > 0.f && rho < INFINITY)) return false;
    c = bb_div(x, rho);
    s = bb_div(y, rho);
    return true;
}

// The cosine of the angle a - v - b at the vertex v: u = a - v, w = b - v, (u . w) / (|u| |w|).  -> false unless 0 < |u| |w| < inf.
__device__ __forceinline__ bool bb_cos_angle(bb_vec a, bb_vec v, bb_vec b, float& c) {
    const bb_vec u = bb_vsub(a, v), w = bb_vsub(b, v);
    const float den = bb_mul(sqrtf(bb_dot(u, u)), sqrtf(bb_dot(w, w)));
    if (!(den > 0.f && den < INFINITY)) return false;
    c = bb_div(bb_dot(u, w), den);
    return true;
}

// The DSSP energy of donor (N, H) and acceptor (C, O), section 6.10's arithmetic restated: 27.888 (((1 / r_ON + 1 / r_CH) - 1 / r_OH) - 1 / r_CN), -9.9 if a
// distance is below 0.5 A, never below -9.9
__device__ __forceinline__ float bb_hbond(bb_vec n, bb_vec h, bb_vec c, bb_vec o) {
    const float r_on = sqrtf(bb_d2(o, n)), r_ch = sqrtf(bb_d2(c, h)), r_oh = sqrtf(bb_d2(o, h)), r_cn = sqrtf(bb_d2(c, n));
    if (r_on < 0.5f || r_ch < 0.5f || r_oh < 0.5f || r_cn < 0.5f) return BB_CLAMP;
    const float e = bb_mul(BB_Q, bb_sub(bb_sub(bb_add(bb_div(1.f, r_on), bb_div(1.f, r_ch)), bb_div(1.f, r_oh)), bb_div(1.f, r_cn)));
    return e < BB_CLAMP ? BB_CLAMP : e;
}

__device__ __forceinline__ bb_vec bb_xyz(float4 v) { return bb_vec{v.x, v.y, v.z}; }

// bytes of dynamic LDS for L residues: five float4 per residue, the relation, the counts; every carve a multiple of 16
__host__ __device__ inline size_t bb_lds_words(int L) { return (size_t)L * ((L + 63) / 64); }
__host__ __device__ inline size_t bb_lds_bytes(int L) { return (size_t)L * 80 + ((bb_lds_words(L) * 8 + 15) & ~(size_t)15) + BB_COUNTS * 4 + (size_t)L * 4; }

// One workgroup of four waves per candidate (grid folded over x and y).  Phase 0: a thread per residue stages it in LDS as five float4 -- N + bits, CA, C, O, H
// (built from the previous residue's C and O in global memory).  Phase 1: a thread per residue forms its torsions, peptide geometry, Ramachandran class and
// peptide flags from its own record and its two neighbours', and writes them.  Phase 2: the directed relation hb(acceptor i -> donor j) as a bit matrix in LDS,
// a 64-bit word per (i, block of 64 donors): a wave keeps 64 donors in registers, a lane each, walks 64 acceptors by broadcast reads and one ballot per
// acceptor IS the word, stored once by lane 0 -- no atomic, no zeroing pass; the units (block of donors, block of acceptors) are dealt round to the four
// waves.  Phase 3: a thread per residue reads the n-turns at its index from the bits; phase 4: helices, "inside a turn" and, walking all j, the four bridge
// patterns.  The 24 counts are integers: every thread adds what it found to LDS counters (order-free), 24 threads store them.
__global__ __launch_bounds__(BB_THREADS) void backbone_kernel(const float* __restrict__ pos_all, const uint8_t* __restrict__ mask_all, int mask_shared,
                                                              const uint8_t* __restrict__ rows_all, const uint8_t* __restrict__ seq_all, int seq_shared,
                                                              const uint8_t* __restrict__ link_all, const float* __restrict__ regions, int K, float hb_cutoff,
                                                              int64_t N, int S, int L, int A, float* __restrict__ torsion_all, uint8_t* __restrict__ have_all,
                                                              float* __restrict__ bond_all, uint8_t* __restrict__ rama_all, uint8_t* __restrict__ ss_all,
                                                              uint8_t* __restrict__ state_all, int32_t* __restrict__ partner_all, int32_t* __restrict__ count_all) {
    extern __shared__ __attribute__((aligned(16))) char bb_raw[];
    const int64_t c = folded_block();
    if (c >= N) return;                                                         // the last row of a folded grid; block-uniform
    const int64_t g = c / S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = (L + 63) / 64;
    float4* p_n = reinterpret_cast<float4*>(bb_raw);
    float4* p_ca = p_n + L;
    float4* p_c = p_ca + L;
    float4* p_o = p_c + L;
    float4* p_h = p_o + L;
    unsigned long long* hb = reinterpret_cast<unsigned long long*>(p_h + L);
    int* cnt = reinterpret_cast<int*>(bb_raw + (size_t)L * 80 + ((bb_lds_words(L) * 8 + 15) & ~(size_t)15));
    int* turn = cnt + BB_COUNTS;                                                // [L]: bit n - 3 = an n-turn starts here
    const float* pos = pos_all + c * L * A * 3;
    const uint8_t* mask = mask_all + (mask_shared ? g : c) * L * A;
    const uint8_t* rows = rows_all + g * L;
    const uint8_t* seq = seq_all ? seq_all + (seq_shared ? g : c) * L : nullptr;
    const uint8_t* link = link_all ? link_all + g * L : nullptr;
    float* torsion = torsion_all + c * L * 6;
    float* bond = bond_all + c * L * 3;
    uint8_t* have = have_all + c * L;
    uint8_t* rama = rama_all + c * L;
    uint8_t* ss = ss_all + c * L;
    uint8_t* state = state_all + c * L;
    int32_t* partner = partner_all + c * L * 2;

    // ---- phase 0: stage
    if (tid < BB_COUNTS) cnt[tid] = 0;
    for (int r = tid; r < L; r += BB_THREADS) {
        bb_vec n, ca, cc, o;
        int bits = 0;
        if (bb_atom(pos, mask, r, A, 0, n)) bits |= BB_N;
        if (bb_atom(pos, mask, r, A, 1, ca)) bits |= BB_CA;
        if (bb_atom(pos, mask, r, A, 2, cc)) bits |= BB_C;
        if (bb_atom(pos, mask, r, A, 3, o)) bits |= BB_O;
        const int t = seq ? (int)seq[r] : 255;
        if (t == BB_PRO_T) bits |= BB_PRO;
        if (t == BB_GLY_T) bits |= BB_GLY;
        if (rows[r]) bits |= BB_ROW;
        if (r + 1 < L && (link == nullptr || link[r])) bits |= BB_LINK;
        bb_vec h = n;
        if (r >= 1 && (link == nullptr || link[r - 1]) && t != BB_PRO_T && (bits & BB_N)) {
            bb_vec pc, po;
            if (bb_atom(pos, mask, r - 1, A, 2, pc) && bb_atom(pos, mask, r - 1, A, 3, po)) {
                const bb_vec u = bb_vsub(pc, po);
                const float len = sqrtf(bb_dot(u, u));
                if (len > 0.f) {
                    h.x = bb_add(n.x, bb_div(u.x, len));
                    h.y = bb_add(n.y, bb_div(u.y, len));
                    h.z = bb_add(n.z, bb_div(u.z, len));
                    bits |= BB_H;
                }
            }
        }
        p_n[r] = make_float4(n.x, n.y, n.z, __int_as_float(bits));
        p_ca[r] = make_float4(ca.x, ca.y, ca.z, 0.f);
        p_c[r] = make_float4(cc.x, cc.y, cc.z, 0.f);
        p_o[r] = make_float4(o.x, o.y, o.z, 0.f);
        p_h[r] = make_float4(h.x, h.y, h.z, 0.f);
    }
    __syncthreads();

    // ---- phase 1: torsions, peptide geometry, Ramachandran class, peptide flags
    for (int r = tid; r < L; r += BB_THREADS) {
        const float4 nn = p_n[r];
        const int b = __float_as_int(nn.w);
        const int bp = r >= 1 ? __float_as_int(p_n[r - 1].w) : 0, bn = r + 1 < L ? __float_as_int(p_n[r + 1].w) : 0;
        float tor[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, geo[3] = {0.f, 0.f, 0.f};
        int hv = 0, cls = 255;
        if (b & BB_ROW) {
            const bb_vec n = bb_xyz(nn), ca = bb_xyz(p_ca[r]), cc = bb_xyz(p_c[r]);
            const bool own3 = (b & (BB_N | BB_CA | BB_C)) == (BB_N | BB_CA | BB_C);
            if ((bp & BB_LINK) && (bp & BB_C) && own3 && bb_torsion(bb_xyz(p_c[r - 1]), n, ca, cc, tor[0], tor[1])) hv |= HV_PHI;
            if (b & BB_LINK) {                                                  // implies r + 1 < L
                const bb_vec n1 = bb_xyz(p_n[r + 1]), ca1 = bb_xyz(p_ca[r + 1]);
                if (own3 && (bn & BB_N) && bb_torsion(n, ca, cc, n1, tor[2], tor[3])) hv |= HV_PSI;
                if ((b & (BB_CA | BB_C)) == (BB_CA | BB_C) && (bn & (BB_N | BB_CA)) == (BB_N | BB_CA) && bb_torsion(ca, cc, n1, ca1, tor[4], tor[5]))
                    hv |= HV_OMEGA;
                if ((b & BB_C) && (bn & BB_N)) {
                    const float len = sqrtf(bb_d2(cc, n1));
                    if (len < INFINITY) { geo[0] = len; hv |= HV_LEN; }
                    if ((b & BB_CA) && bb_cos_angle(ca, cc, n1, geo[1])) hv |= HV_ANG_C;
                    if ((bn & BB_CA) && bb_cos_angle(cc, n1, ca1, geo[2])) hv |= HV_ANG_N;
                }
            }
            if (!(hv & HV_PHI)) tor[0] = tor[1] = 0.f;                          // a torsion that came out undefined left nothing behind
            if (!(hv & HV_PSI)) tor[2] = tor[3] = 0.f;
            if (!(hv & HV_OMEGA)) tor[4] = tor[5] = 0.f;
            if (!(hv & HV_ANG_C)) geo[1] = 0.f;
            if (!(hv & HV_ANG_N)) geo[2] = 0.f;
            if (b & (BB_N | BB_CA | BB_C | BB_O)) atomicAdd(&cnt[CN_PART], 1);
            if ((hv & (HV_PHI | HV_PSI)) == (HV_PHI | HV_PSI)) {
                cls = K;
                for (int k = K - 1; k >= 0; --k) {                              // the FIRST matching region: walked downwards, the lowest k is kept
                    const float* q = regions + k * 8;
                    const bool in_phi = bb_sub(bb_mul(tor[1], q[0]), bb_mul(tor[0], q[1])) >= 0.f && bb_sub(bb_mul(tor[0], q[3]), bb_mul(tor[1], q[2])) >= 0.f;
                    const bool in_psi = bb_sub(bb_mul(tor[3], q[4]), bb_mul(tor[2], q[5])) >= 0.f && bb_sub(bb_mul(tor[2], q[7]), bb_mul(tor[3], q[6])) >= 0.f;
                    if (in_phi && in_psi) cls = k;
                }
                atomicAdd(&cnt[CN_PHIPSI], 1);
                if (cls < K) atomicAdd(&cnt[CN_REGION + cls], 1);
                else {
                    atomicAdd(&cnt[CN_OUTLIER], 1);
                    if (b & BB_GLY) atomicAdd(&cnt[CN_OUTLIER_GLY], 1);
                }
            }
            if (hv & HV_OMEGA) {
                atomicAdd(&cnt[CN_OMEGA], 1);
                if (tor[4] > 0.f) {
                    atomicAdd(&cnt[CN_CIS], 1);
                    if (!(bn & BB_PRO)) atomicAdd(&cnt[CN_CIS_NONPRO], 1);
                }
                if (fabsf(tor[5]) > 0.5f) atomicAdd(&cnt[CN_TWISTED], 1);
            }
        }
        for (int k = 0; k < 6; ++k) torsion[(int64_t)r * 6 + k] = tor[k];
        for (int k = 0; k < 3; ++k) bond[(int64_t)r * 3 + k] = geo[k];
        have[r] = (uint8_t)hv;
        rama[r] = (uint8_t)cls;
    }

    // ---- phase 2: the relation.  Unit u = (block of 64 donors jb, block of 64 acceptors ib); the word of (acceptor i, jb) holds donor jb 64 + lane in bit lane
    int n_don = 0, n_acc = 0;
    for (int u = wave; u < W * W; u += BB_THREADS / 64) {
        const int jb = u % W, ib = u / W;
        const int j = jb * 64 + lane;
        bb_vec dn{0.f, 0.f, 0.f}, dh = dn, dca = dn;
        int bj = 0;
        if (j < L) {
            const float4 nn = p_n[j];
            dn = bb_xyz(nn); dh = bb_xyz(p_h[j]); dca = bb_xyz(p_ca[j]);
            bj = __float_as_int(nn.w);
        }
        const bool donor = (bj & (BB_H | BB_CA)) == (BB_H | BB_CA);
        const int i1 = min(L, ib * 64 + 64);
        for (int i = ib * 64; i < i1; ++i) {                                    // wave-uniform
            const int bi = __float_as_int(p_n[i].w);                            // broadcast reads
            bool hit = false;
            if (donor && (bi & (BB_CA | BB_C | BB_O)) == (BB_CA | BB_C | BB_O) && i != j && !(j == i + 1 && (bi & BB_LINK)) && !(i == j + 1 && (bj & BB_LINK)) &&
                bb_d2(dca, bb_xyz(p_ca[i])) < 81.f)
                hit = bb_hbond(dn, dh, bb_xyz(p_c[i]), bb_xyz(p_o[i])) < hb_cutoff;
            const unsigned long long word = __ballot(hit);
            if (lane == 0) {
                hb[(size_t)i * W + jb] = word;
                if (bi & BB_ROW) n_acc += __popcll(word);
            }
            n_don += hit && (bj & BB_ROW);
        }
    }
    if (n_don) atomicAdd(&cnt[CN_DONOR], n_don);
    if (n_acc) atomicAdd(&cnt[CN_ACCEPTOR], n_acc);
    __syncthreads();

    // Hbond(i, j) = hb(acceptor i -> donor j), false outside the row
    auto hbond = [&](int i, int j) -> bool { return i >= 0 && j >= 0 && i < L && j < L && ((hb[(size_t)i * W + (j >> 6)] >> (j & 63)) & 1ull); };
    auto linked = [&](int r) -> bool { return r >= 0 && r < L && (__float_as_int(p_n[r].w) & BB_LINK); };

    // ---- phase 3: the n-turns that start at r: Hbond(r, r + n) with the steps r .. r + n - 1 linked
    for (int r = tid; r < L; r += BB_THREADS) {
        int run = 0;
        while (run < 5 && linked(r + run)) ++run;
        int t = 0;
        for (int n = 3; n <= 5; ++n)
            if (run >= n && hbond(r, r + n)) t |= 1 << (n - 3);
        turn[r] = t;
    }
    __syncthreads();

    // ---- phase 4: helices, bridges, states
    for (int r = tid; r < L; r += BB_THREADS) {
        const int b = __float_as_int(p_n[r].w);
        int bits = 0, st = 255, par = -1, anti = -1;
        if ((b & BB_ROW) && (b & (BB_N | BB_CA | BB_C | BB_O))) {
            for (int n = 3; n <= 5; ++n) {
                const int tb = 1 << (n - 3), helix = n == 3 ? SS_H3 : n == 4 ? SS_H4 : SS_H5;
                for (int i = r - n + 1; i <= r; ++i) {
                    if (i >= 1 && (turn[i - 1] & tb) && (turn[i] & tb)) bits |= helix;                 // helix_n on i .. i + n - 1
                    if (i >= 0 && i < r && (turn[i] & tb)) bits |= SS_TURN;                            // inside: i < r < i + n
                }
            }
            if (linked(r - 1) && linked(r)) {
                for (int j = 1; j + 1 < L; ++j) {
                    if (abs(j - r) < 3 || !linked(j - 1) || !linked(j)) continue;
                    if ((hbond(r - 1, j) && hbond(j, r + 1)) || (hbond(j - 1, r) && hbond(r, j + 1))) { bits |= SS_PAR; if (par < 0) par = j; }
                    if ((hbond(r, j) && hbond(j, r)) || (hbond(r - 1, j + 1) && hbond(j - 1, r + 1))) { bits |= SS_ANTI; if (anti < 0) anti = j; }
                }
            }
            st = (bits & SS_H4) ? 0 : (bits & (SS_PAR | SS_ANTI)) ? 1 : (bits & SS_H3) ? 2 : (bits & SS_H5) ? 3 : (bits & SS_TURN) ? 4 : 5;
            atomicAdd(&cnt[CN_STATE + st], 1);
        }
        ss[r] = (uint8_t)bits;
        state[r] = (uint8_t)st;
        partner[(int64_t)r * 2] = par;
        partner[(int64_t)r * 2 + 1] = anti;
    }
    __syncthreads();
    if (tid < BB_COUNTS) count_all[c * BB_COUNTS + tid] = cnt[tid];
}

}  // namespace abopt

using namespace abopt;

extern "C" int abopt_backbone_max_rows(void) { return BB_MAX_ROWS; }

extern "C" int abopt_backbone_conformation_grouped(const float* pos, const uint8_t* mask, int mask_shared, const uint8_t* rows, const uint8_t* seqs,
                                                   int seq_shared, const uint8_t* link, const float* regions, int K, int G, int S, int L, int A, float hb_cutoff,
                                                   void* torsion, void* have, void* bond, void* rama, void* ss, void* state, void* partner, void* count,
                                                   abopt_stream stream) {
    const char* name = "backbone_conformation_grouped";
    int rc = check_candidate_dims(name, G, S, L, A);
    if (rc != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(A >= 4, "backbone_conformation_grouped: A=%d atoms per residue, the slots 0 .. 3 are N, CA, C, O (expected 4 .. %d)", A, kMaxAtoms);
    ABOPT_CHECK_ARG(isfinite(hb_cutoff) && hb_cutoff <= 0.f, "backbone_conformation_grouped: hb_cutoff must be finite and <= 0 (got %g)", (double)hb_cutoff);
    ABOPT_CHECK_ARG(K >= 0 && K <= BB_MAX_REGIONS, "backbone_conformation_grouped: K=%d regions, expected 0 .. %d", K, BB_MAX_REGIONS);
    if (L > BB_MAX_ROWS) {
        set_error("backbone_conformation_grouped: L=%d residues exceed the %d whose hydrogen-bond relation fits a workgroup's LDS", L, BB_MAX_ROWS);
        return ABOPT_EUNSUPPORTED;
    }
    if (G == 0 || S == 0) return ABOPT_OK;
    if ((rc = check_group_count(name, G)) != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(pos && mask && rows && torsion && have && bond && rama && ss && state && partner && count && (regions || K == 0),
                    "backbone_conformation_grouped: NULL argument");
    static LdsConfig lds_cfg;                                                   // granted once, for the largest call there can be: nothing changes under a capture
    if ((rc = ensure_dynamic_lds(reinterpret_cast<const void*>(backbone_kernel), bb_lds_bytes(BB_MAX_ROWS), lds_cfg)) != ABOPT_OK) return rc;
    const int64_t N = (int64_t)G * S;
    hipLaunchKernelGGL(backbone_kernel, fold_grid(N, 1u), dim3(BB_THREADS), bb_lds_bytes(L), (hipStream_t)stream, pos, mask, mask_shared ? 1 : 0, rows, seqs,
                       seq_shared ? 1 : 0, link, regions, K, hb_cutoff, N, S, L, A, (float*)torsion, (uint8_t*)have, (float*)bond, (uint8_t*)rama, (uint8_t*)ss,
                       (uint8_t*)state, (int32_t*)partner, (int32_t*)count);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}
