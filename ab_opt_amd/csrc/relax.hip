// Relax of docked candidates on the device: a fixed number of Jacobi descent steps that move every movable residue as a rigid body, down
// the atom-level clashes and the peptide-bond / CA-CA violations, tethered to where the residue started.  Nothing in the reference is matched (its relax stage is
// OpenMM / Rosetta); this is no force field.  The definition is this library's own (include/abopt.h: abopt_relax_grouped).
// One launch, one workgroup per candidate, all iterations inside it.  Only the moved residues change, so only they live in LDS: each as its centre c (relative to
// the candidate's first participating atom o) and the offsets v_p = x_p - c of its atoms.  A rotation acts on the offsets and a shift on the centre, so the
// residue's internal distances are rounded at the size of the residue, not at the size of its coordinates.  Everything else is read from pos_in.
#include <math.h>
#include <limits.h>
#include <algorithm>
#include "abopt_common.h"
#include "candidate_common.h"
#include "kernels.h"

// plain operators, rounded one by one (guide.hip, sasa.hip): the compiler contracts nothing differently in different places
#pragma clang fp contract(off)

namespace abopt {

constexpr int RX_WAVES = 4;                // waves per workgroup
constexpr int RX_TILE = 512;               // bounding spheres of static residues staged at a time: 8 KB of LDS whatever L is
constexpr int RX_MAX_MOVED = 256;          // moved residues of a candidate at most: 154 KiB of LDS with 15 atom slots
constexpr int RX_MAX_ITERS = 1024;
constexpr float RX_BOND = 1.329f;          // C-N of a trans peptide bond, Angstrom
constexpr float RX_CA = 3.80f;             // CA-CA across a trans peptide bond, Angstrom
constexpr float RX_EPS = 1e-12f;           // a pair closer than 1e-6 A has no direction (the rule of abopt_guide_positions); also the smallest inertia that turns

struct RelaxKnobs { float w_bond, w_ca, w_clash, w_tether, clash_d, step, max_shift, max_angle; int iters; };

// The dynamic LDS of a workgroup, for `mx` moved residues at most, A atom slots and a tile of `tile` static spheres
struct RelaxLds {
    float4 *v, *v0, *cs, *c0, *u, *acc, *tile;
    int *idx, *list, *redi;
    __host__ __device__ static size_t bytes(int mx, int A, int tile) {
        return ((size_t)mx * (2 * A + 6) + tile) * sizeof(float4) + ((size_t)mx + RX_WAVES * 64 + 2 * RX_WAVES) * sizeof(int);
    }
    __device__ RelaxLds(char* raw, int mx, int A, int tl) {
        v = (float4*)raw;                  // [mx][A] offsets from the centre; w = 1 for a participating atom, else 0
        v0 = v + (size_t)mx * A;           // [mx][A] the input's offsets
        cs = v0 + (size_t)mx * A;          // [mx] centre c0 + u (relative to o), radius of the bounding sphere
        c0 = cs + mx;                      // [mx] the input's centre, inertia I
        u = c0 + mx;                       // [mx] the sum of the shifts so far: small numbers, so the centre does not collect the roundings of a large one
        acc = u + mx;                     // [mx][3] F, E_bond | tau, E_ca | E_clash, E_tether, n_a, -
        tile = acc + (size_t)mx * 3;       // [tl] spheres of the static residues of the current tile (radius -inf: none)
        idx = (int*)(tile + tl);           // [mx] the moved residues, ascending
        list = idx + mx;                   // [waves][64] the candidates that passed a wave's prune
        redi = list + RX_WAVES * 64;       // [2 waves]
    }
};

// atom t (= residue * A + slot) of the input takes part: its mask byte is set and its coordinates are finite
__device__ __forceinline__ bool rx_part(const float* pos, const uint8_t* mask, int64_t t) {
    return mask[t] && finite_f32(pos[t * 3]) && finite_f32(pos[t * 3 + 1]) && finite_f32(pos[t * 3 + 2]);
}
// ... and where it is, relative to o
__device__ __forceinline__ bool rx_atom(const float* pos, const uint8_t* mask, int64_t t, float3 o, float3& y) {
    if (!mask[t]) return false;
    const float a = pos[t * 3], b = pos[t * 3 + 1], c = pos[t * 3 + 2];
    if (!(finite_f32(a) && finite_f32(b) && finite_f32(c))) return false;
    y = make_float3(a - o.x, b - o.y, c - o.z);
    return true;
}

struct RxMoved {                           // the residue is moved: its byte of `move` is set and one of its atoms takes part
    const uint8_t* move; const float* pos; const uint8_t* mask; int A;
    __device__ __forceinline__ bool operator()(int r) const {
        if (!move[r]) return false;
        for (int p = 0; p < A; ++p)
            if (rx_part(pos, mask, (int64_t)r * A + p)) return true;
        return false;
    }
};

// the lane's share of a moved residue's force, torque and energies
struct RxPart { float fx, fy, fz, tx, ty, tz, e_bond, e_ca, e_clash, e_tether; };

// f acts on the atom at offset v from the centre
__device__ __forceinline__ void rx_push(RxPart& s, float3 v, float fx, float fy, float fz) {
    s.fx = s.fx + fx; s.fy = s.fy + fy; s.fz = s.fz + fz;
    s.tx = s.tx + (v.y * fz - v.z * fy); s.ty = s.ty + (v.z * fx - v.x * fz); s.tz = s.tz + (v.x * fy - v.y * fx);
}

// clash of the atom at yp (offset vp in its residue) with the atom at yq; count: the pair's energy is entered here
__device__ __forceinline__ void rx_clash(RxPart& s, float3 vp, float3 yp, float3 yq, float clash_d, float w2, bool count) {
    const float dx = yp.x - yq.x, dy = yp.y - yq.y, dz = yp.z - yq.z;
    const float d2 = dx * dx + dy * dy + dz * dz;
    const float d = sqrtf(d2);
    const float g = clash_d - d;
    if (!(g > 0.f)) return;
    if (count) s.e_clash = s.e_clash + g * g;
    if (d2 < RX_EPS) return;
    const float k = w2 * g / d;
    rx_push(s, vp, k * dx, k * dy, k * dz);
}

// Grid: the candidate folded over x and y; 4 waves; dynamic LDS (RelaxLds).
//   set-up    o = the first participating atom; the moved residues compacted by ballots (take, candidate_common.h) and staged: centre, offsets, inertia, radius.
//   a pass    forces at the current positions.  A wave owns one moved residue at a time.  Its lanes test the bounding spheres of the other moved residues, then of the
//             static residues tile by tile (the prune of interface.hip: conservative in fp32, a pruned pair would have added exactly +0), compact the survivors into
//             the wave's list, and take one (residue, atom) of the list each; every lane walks the owned residue's atoms (broadcast LDS reads) and keeps its share of
//             F, tau and the energies in registers.  Lanes 0-3 add the two bonds and the two CA springs, lanes 8.. the tethers.  One butterfly per residue and
//             stage, lane 0 adds into acc in a fixed order.
//   update    after a barrier, thread i turns residue i's offsets by Rot(omega) and adds the shift to u (the centre is c0 + u, rounded once); wave 0 sums the energies of the first and the last pass.
//   Two barriers per iteration while the static spheres fit one tile (L <= 512); beyond, two more per further tile.
__global__ __launch_bounds__(256) void relax_kernel(const float* pos_all, float* out_all, const uint8_t* __restrict__ mask_all, int mask_shared,
                                                    const uint8_t* __restrict__ move_all, const uint8_t* __restrict__ link_all, float* __restrict__ energy_all,
                                                    int N, int S, int L, int A, int mx, int tl, RelaxKnobs kn) {
    extern __shared__ __attribute__((aligned(16))) char rx_raw[];
    const int64_t c64 = folded_block();
    if (c64 >= N) return;                                                       // the last row of a folded grid; block-uniform
    const RelaxLds lds(rx_raw, mx, A, tl);
    const int g = (int)(c64 / S), tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t nat = (int64_t)L * A;
    const float* pos = pos_all + c64 * nat * 3;                                 // NOT restrict against out: the call may be in place
    float* out = out_all + c64 * nat * 3;
    const uint8_t* mask = mask_all + (mask_shared ? g : c64) * nat;
    const uint8_t* move = move_all + (int64_t)g * L;
    const uint8_t* link = link_all ? link_all + (int64_t)g * L : nullptr;
    float* energy = energy_all + c64 * 8;
    const bool in_place = pos == out;

    // ---- o: the first participating atom of the candidate
    int first = INT_MAX;
    for (int64_t t = tid; t < nat; t += 256)
        if (rx_part(pos, mask, t)) { first = (int)t; break; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off, 64));
    if (lane == 0) lds.redi[wave] = first;
    __syncthreads();
    first = min(min(lds.redi[0], lds.redi[1]), min(lds.redi[2], lds.redi[3]));

    // ---- the moved residues, ascending; every wave finds the same list, wave 0 stores it
    int M = 0;
    bool over = false;
    if (first != INT_MAX) {
        const RxMoved moved{move, pos, mask, A};
        int cur = 0;
        M = take(L, moved, cur, mx, lds.idx, wave == 0);
        over = take(L, moved, cur, 1, (int*)nullptr, false) > 0;               // more than the caller's bound: refused below
    }
    if (over || M == 0) {                                                       // block-uniform: nothing moves, every energy term is empty (refused: NaN)
        if (!in_place)
            for (int64_t t = tid; t < nat * 3; t += 256) out[t] = pos[t];       // bit for bit
        if (tid < 8) energy[tid] = over ? __uint_as_float(0x7fc00000u) : 0.f;
        return;
    }
    const float3 o = make_float3(pos[(int64_t)first * 3], pos[(int64_t)first * 3 + 1], pos[(int64_t)first * 3 + 2]);
    __syncthreads();                                                            // idx is written

    // ---- stage the moved residues: thread i owns residue i
    for (int i = tid; i < M; i += 256) {
        const int a = lds.idx[i];
        float sx = 0.f, sy = 0.f, sz = 0.f;
        int n = 0;
        for (int p = 0; p < A; ++p) {
            float3 y;
            const bool ok = rx_atom(pos, mask, (int64_t)a * A + p, o, y);
            if (ok) { sx = sx + y.x; sy = sy + y.y; sz = sz + y.z; ++n; }
            lds.v[(size_t)i * A + p] = ok ? make_float4(y.x, y.y, y.z, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float fn = (float)n, cx = sx / fn, cy = sy / fn, cz = sz / fn;    // n >= 1: the residue is moved
        float inertia = 0.f, r2 = 0.f;
        for (int p = 0; p < A; ++p) {
            float4 y = lds.v[(size_t)i * A + p];
            if (y.w != 0.f) {
                y.x = y.x - cx; y.y = y.y - cy; y.z = y.z - cz;
                const float d2 = y.x * y.x + y.y * y.y + y.z * y.z;
                inertia = inertia + d2;
                r2 = fmaxf(r2, d2);
            }
            lds.v[(size_t)i * A + p] = y;
            lds.v0[(size_t)i * A + p] = y;
        }
        lds.cs[i] = make_float4(cx, cy, cz, sqrtf(r2));
        lds.c0[i] = make_float4(cx, cy, cz, inertia);
        lds.u[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        lds.acc[(size_t)i * 3 + 2] = make_float4(0.f, 0.f, fn, 0.f);
    }

    const int tiles = (L + tl - 1) / tl;
    const float w2_clash = 2.f * kn.w_clash, w2_bond = 2.f * kn.w_bond, w2_ca = 2.f * kn.w_ca, w2_tether = 2.f * kn.w_tether;
    const float cap_shift2 = kn.max_shift * kn.max_shift, cap_angle2 = kn.max_angle * kn.max_angle;
    int* list = lds.list + wave * 64;
    bool staged = false;

    for (int k = 0; k <= kn.iters; ++k) {
        __syncthreads();                                                        // the staging / the previous update is done
        // ---- stage A: the other moved residues, the springs, the tethers
        for (int i = wave; i < M; i += RX_WAVES) {
            const int a = lds.idx[i];
            const float4 sa = lds.cs[i];
            RxPart s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int j0 = 0; j0 < M; j0 += 64) {
                const int j = j0 + lane;
                bool ok = j < M && j != i;
                if (ok) {
                    const int b = lds.idx[j];
                    if (link && ((b == a + 1 && link[a]) || (a == b + 1 && link[b]))) ok = false;
                    const float4 sb = lds.cs[j];
                    const float dx = sa.x - sb.x, dy = sa.y - sb.y, dz = sa.z - sb.z;
                    const float reach = ((sa.w + sb.w) + kn.clash_d) * (1.f + 1.52587890625e-5f) + 0.01f;
                    if (sqrtf(dx * dx + dy * dy + dz * dz) > reach) ok = false;
                }
                const unsigned long long hit = __ballot(ok);
                if (hit == 0ull) continue;                                      // wave-uniform
                if (ok) list[__popcll(hit & ((1ull << lane) - 1ull))] = j;
                wave_lds_sync();
                const int items = __popcll(hit) * A;
                for (int it = lane; it < items; it += 64) {
                    const int jj = list[it / A], q = it % A;
                    const float4 vq = lds.v[(size_t)jj * A + q];
                    if (vq.w == 0.f) continue;
                    const float4 cb = lds.cs[jj];
                    const float3 yq = make_float3(cb.x + vq.x, cb.y + vq.y, cb.z + vq.z);
                    const bool count = lds.idx[jj] > a;                         // a pair of two moved residues is counted at the lower one
                    for (int p = 0; p < A; ++p) {
                        const float4 vp = lds.v[(size_t)i * A + p];             // one broadcast read
                        if (vp.w == 0.f) continue;
                        rx_clash(s, make_float3(vp.x, vp.y, vp.z), make_float3(sa.x + vp.x, sa.y + vp.y, sa.z + vp.z), yq, kn.clash_d, w2_clash, count);
                    }
                }
                wave_lds_sync();                                                // the list is read before the next round overwrites it
            }
            if (link && lane < 4) {                                             // lane 0: bond to a + 1, 1: bond to a - 1, 2: CA to a + 1, 3: CA to a - 1
                const bool prev = lane & 1, ca = lane >> 1;
                const int nb = prev ? a - 1 : a + 1, j = prev ? i - 1 : i + 1;
                if (nb >= 0 && nb < L && link[prev ? nb : a]) {
                    const float4 vp = lds.v[(size_t)i * A + (ca ? 1 : prev ? 0 : 2)];
                    const int slot = ca ? 1 : prev ? 2 : 0;
                    const bool nb_moved = j >= 0 && j < M && lds.idx[j] == nb;
                    float3 yq;
                    bool ok;
                    if (nb_moved) {
                        const float4 vq = lds.v[(size_t)j * A + slot], cb = lds.cs[j];
                        ok = vq.w != 0.f;
                        yq = make_float3(cb.x + vq.x, cb.y + vq.y, cb.z + vq.z);
                    } else {
                        ok = rx_atom(pos, mask, (int64_t)nb * A + slot, o, yq);
                    }
                    if (ok && vp.w != 0.f) {
                        const float dx = (sa.x + vp.x) - yq.x, dy = (sa.y + vp.y) - yq.y, dz = (sa.z + vp.z) - yq.z;
                        const float d2 = dx * dx + dy * dy + dz * dz;
                        const float d = sqrtf(d2);
                        const float e = d - (ca ? RX_CA : RX_BOND);
                        if (!prev || !nb_moved) {                               // a spring of two moved residues is counted at the lower one
                            if (ca) s.e_ca = s.e_ca + e * e; else s.e_bond = s.e_bond + e * e;
                        }
                        if (!(d2 < RX_EPS)) {
                            const float kf = -(ca ? w2_ca : w2_bond) * e / d;
                            rx_push(s, make_float3(vp.x, vp.y, vp.z), kf * dx, kf * dy, kf * dz);
                        }
                    }
                }
            }
            if (lane >= 8 && lane < 8 + A) {
                const int p = lane - 8;
                const float4 vp = lds.v[(size_t)i * A + p];
                if (vp.w != 0.f) {
                    const float4 v0 = lds.v0[(size_t)i * A + p], us = lds.u[i];
                    const float tx = us.x + (vp.x - v0.x), ty = us.y + (vp.y - v0.y), tz = us.z + (vp.z - v0.z);
                    s.e_tether = s.e_tether + (tx * tx + ty * ty + tz * tz);
                    rx_push(s, make_float3(vp.x, vp.y, vp.z), -w2_tether * tx, -w2_tether * ty, -w2_tether * tz);
                }
            }
            const float fx = wave_sum_butterfly(s.fx), fy = wave_sum_butterfly(s.fy), fz = wave_sum_butterfly(s.fz), tx = wave_sum_butterfly(s.tx), ty = wave_sum_butterfly(s.ty), tz = wave_sum_butterfly(s.tz);
            const float eb = wave_sum_butterfly(s.e_bond), ec = wave_sum_butterfly(s.e_ca), el = wave_sum_butterfly(s.e_clash), et = wave_sum_butterfly(s.e_tether);
            if (lane == 0) {
                const float fn = lds.acc[(size_t)i * 3 + 2].z;
                lds.acc[(size_t)i * 3] = make_float4(fx, fy, fz, eb);
                lds.acc[(size_t)i * 3 + 1] = make_float4(tx, ty, tz, ec);
                lds.acc[(size_t)i * 3 + 2] = make_float4(el, et, fn, 0.f);
            }
        }
        // ---- stage B: the static residues, tile by tile
        for (int tile = 0; tile < tiles; ++tile) {
            const int base = tile * tl;
            if (tiles > 1 || !staged) {                                         // block-uniform
                if (staged) __syncthreads();                                    // the readers of the tile that is replaced are done
                for (int t = tid; t < tl; t += 256) {
                    const int r = base + t;
                    float4 sph = make_float4(0.f, 0.f, 0.f, -INFINITY);
                    if (r < L && !move[r]) {                                    // a residue with its byte of move set is moved, or has no atom that takes part
                        float sx = 0.f, sy = 0.f, sz = 0.f;
                        int n = 0;
                        for (int p = 0; p < A; ++p) {
                            float3 y;
                            if (rx_atom(pos, mask, (int64_t)r * A + p, o, y)) { sx = sx + y.x; sy = sy + y.y; sz = sz + y.z; ++n; }
                        }
                        if (n > 0) {
                            const float fn = (float)n, cx = sx / fn, cy = sy / fn, cz = sz / fn;
                            float r2 = 0.f;
                            for (int p = 0; p < A; ++p) {
                                float3 y;
                                if (rx_atom(pos, mask, (int64_t)r * A + p, o, y)) {
                                    const float dx = y.x - cx, dy = y.y - cy, dz = y.z - cz;
                                    r2 = fmaxf(r2, dx * dx + dy * dy + dz * dz);
                                }
                            }
                            sph = make_float4(cx, cy, cz, sqrtf(r2));
                        }
                    }
                    lds.tile[t] = sph;
                }
                staged = true;
                __syncthreads();
            }
            const int tn = min(tl, L - base);
            for (int i = wave; i < M; i += RX_WAVES) {
                const int a = lds.idx[i];
                const float4 sa = lds.cs[i];
                RxPart s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                bool any = false;                                               // wave-uniform
                for (int t0 = 0; t0 < tn; t0 += 64) {
                    const int t = t0 + lane, b = base + t;
                    bool ok = t < tn;
                    if (ok) {
                        const float4 sb = lds.tile[t];
                        if (link && ((b == a + 1 && link[a]) || (a == b + 1 && link[b]))) ok = false;
                        const float dx = sa.x - sb.x, dy = sa.y - sb.y, dz = sa.z - sb.z;
                        const float reach = ((sa.w + sb.w) + kn.clash_d) * (1.f + 1.52587890625e-5f) + 0.01f;     // -inf for a residue that is not static
                        if (!(sqrtf(dx * dx + dy * dy + dz * dz) <= reach)) ok = false;
                    }
                    const unsigned long long hit = __ballot(ok);
                    if (hit == 0ull) continue;                                  // wave-uniform
                    any = true;
                    if (ok) list[__popcll(hit & ((1ull << lane) - 1ull))] = b;
                    wave_lds_sync();
                    const int items = __popcll(hit) * A;
                    for (int it = lane; it < items; it += 64) {
                        const int b2 = list[it / A], q = it % A;
                        float3 yq;
                        if (!rx_atom(pos, mask, (int64_t)b2 * A + q, o, yq)) continue;
                        for (int p = 0; p < A; ++p) {
                            const float4 vp = lds.v[(size_t)i * A + p];         // one broadcast read
                            if (vp.w == 0.f) continue;
                            rx_clash(s, make_float3(vp.x, vp.y, vp.z), make_float3(sa.x + vp.x, sa.y + vp.y, sa.z + vp.z), yq, kn.clash_d, w2_clash, true);
                        }
                    }
                    wave_lds_sync();
                }
                if (!any) continue;                                             // every lane's share is +0
                const float fx = wave_sum_butterfly(s.fx), fy = wave_sum_butterfly(s.fy), fz = wave_sum_butterfly(s.fz), tx = wave_sum_butterfly(s.tx), ty = wave_sum_butterfly(s.ty), tz = wave_sum_butterfly(s.tz);
                const float el = wave_sum_butterfly(s.e_clash);
                if (lane == 0) {
                    float4 f = lds.acc[(size_t)i * 3], t = lds.acc[(size_t)i * 3 + 1], e = lds.acc[(size_t)i * 3 + 2];
                    f.x = f.x + fx; f.y = f.y + fy; f.z = f.z + fz;
                    t.x = t.x + tx; t.y = t.y + ty; t.z = t.z + tz;
                    e.x = e.x + el;
                    lds.acc[(size_t)i * 3] = f; lds.acc[(size_t)i * 3 + 1] = t; lds.acc[(size_t)i * 3 + 2] = e;
                }
            }
        }
        __syncthreads();                                                        // the forces are complete
        // ---- the energies of the input (k = 0) and of the output (k = iters): wave 0, lanes stride the residues, one butterfly
        if (wave == 0 && (k == 0 || k == kn.iters)) {
            float eb = 0.f, ec = 0.f, el = 0.f, et = 0.f;
            for (int i = lane; i < M; i += 64) {
                eb = eb + lds.acc[(size_t)i * 3].w; ec = ec + lds.acc[(size_t)i * 3 + 1].w;
                el = el + lds.acc[(size_t)i * 3 + 2].x; et = et + lds.acc[(size_t)i * 3 + 2].y;
            }
            eb = kn.w_bond * wave_sum_butterfly(eb); ec = kn.w_ca * wave_sum_butterfly(ec); el = kn.w_clash * wave_sum_butterfly(el); et = kn.w_tether * wave_sum_butterfly(et);
            if (lane == 0) {
                if (k == 0) { energy[0] = eb; energy[1] = ec; energy[2] = el; energy[3] = et; }
                if (k == kn.iters) { energy[4] = eb; energy[5] = ec; energy[6] = el; energy[7] = et; }
            }
        }
        if (k == kn.iters) break;                                               // block-uniform
        // ---- the update: thread i owns residue i
        for (int i = tid; i < M; i += 256) {
            const float4 f = lds.acc[(size_t)i * 3], t = lds.acc[(size_t)i * 3 + 1];
            const float fn = lds.acc[(size_t)i * 3 + 2].z, inertia = lds.c0[i].w;
            float dx = kn.step * f.x / fn, dy = kn.step * f.y / fn, dz = kn.step * f.z / fn;
            const float n2 = dx * dx + dy * dy + dz * dz;
            if (n2 > cap_shift2) { const float q = kn.max_shift / sqrtf(n2); dx = dx * q; dy = dy * q; dz = dz * q; }
            float wx = 0.f, wy = 0.f, wz = 0.f;
            if (!(inertia < RX_EPS)) { wx = kn.step * t.x / inertia; wy = kn.step * t.y / inertia; wz = kn.step * t.z / inertia; }
            float th2 = wx * wx + wy * wy + wz * wz;
            if (th2 > cap_angle2) { const float q = kn.max_angle / sqrtf(th2); wx = wx * q; wy = wy * q; wz = wz * q; th2 = wx * wx + wy * wy + wz * wz; }
            // Rodrigues: Rot(w) v = v + (sin th / th) w x v + ((1 - cos th) / th^2) w x (w x v), the second coefficient as 2 sin^2(th / 2) / th^2 (no cancellation)
            float ka = 1.f, kb = 0.5f;
            if (!(th2 < RX_EPS)) {
                const float th = sqrtf(th2), h = sinf(0.5f * th) / (0.5f * th);
                ka = sinf(th) / th;
                kb = 0.5f * h * h;
            }
            if (th2 != 0.f)
                for (int p = 0; p < A; ++p) {
                    float4 v = lds.v[(size_t)i * A + p];
                    if (v.w == 0.f) continue;
                    const float ux = wy * v.z - wz * v.y, uy = wz * v.x - wx * v.z, uz = wx * v.y - wy * v.x;
                    const float qx = wy * uz - wz * uy, qy = wz * ux - wx * uz, qz = wx * uy - wy * ux;
                    v.x = v.x + (ka * ux + kb * qx); v.y = v.y + (ka * uy + kb * qy); v.z = v.z + (ka * uz + kb * qz);
                    lds.v[(size_t)i * A + p] = v;
                }
            float4 us = lds.u[i];
            const float4 cc = lds.c0[i];
            us.x = us.x + dx; us.y = us.y + dy; us.z = us.z + dz;
            lds.u[i] = us;
            lds.cs[i] = make_float4(cc.x + us.x, cc.y + us.y, cc.z + us.z, lds.cs[i].w);
        }
    }

    // ---- the output: every atom that did not move keeps its bits; the last reads of pos (stage B) lie before the barrier that ended the last pass
    const bool copy_all = kn.iters == 0;                                        // iters = 0 copies the input, the moved residues too
    if (!in_place)
        for (int64_t t = tid; t < nat; t += 256) {
            const int r = (int)(t / A);
            if (!copy_all && move[r] && rx_part(pos, mask, t)) continue;        // a participating atom of a moved residue: written below
            out[t * 3] = pos[t * 3]; out[t * 3 + 1] = pos[t * 3 + 1]; out[t * 3 + 2] = pos[t * 3 + 2];
        }
    if (copy_all) return;
    for (int t = tid; t < M * A; t += 256) {
        const int i = t / A, p = t % A;
        const float4 v = lds.v[t], c = lds.cs[i];
        if (v.w == 0.f) continue;
        float* x = out + ((int64_t)lds.idx[i] * A + p) * 3;
        x[0] = (c.x + v.x) + o.x; x[1] = (c.y + v.y) + o.y; x[2] = (c.z + v.z) + o.z;
    }
}

}  // namespace abopt

using namespace abopt;

extern "C" int abopt_relax_max_moved(void) { return RX_MAX_MOVED; }

extern "C" int abopt_relax_grouped(const float* pos_in, float* pos_out, const uint8_t* mask, int mask_shared, const uint8_t* move, const uint8_t* link,
                                   int G, int S, int L, int A, int max_moved, float w_bond, float w_ca, float w_clash, float w_tether, float clash_d, float step,
                                   float max_shift, float max_angle, int iters, float* energy, abopt_stream stream) {
    int rc = check_candidate_dims("relax_grouped", G, S, L, A);
    if (rc != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(A >= 3, "relax_grouped: atom slots 0, 1, 2 are N, CA, C (A >= 3, got %d)", A);
    const float sc[8] = {w_bond, w_ca, w_clash, w_tether, clash_d, step, max_shift, max_angle};
    static const char* const names[8] = {"w_bond", "w_ca", "w_clash", "w_tether", "clash_d", "step", "max_shift", "max_angle"};
    if ((rc = check_nonnegative("relax_grouped", names, sc, 8)) != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(max_shift > 0.f, "relax_grouped: max_shift must be > 0 (got %g)", (double)max_shift);
    ABOPT_CHECK_ARG(max_angle > 0.f, "relax_grouped: max_angle must be > 0 (got %g)", (double)max_angle);
    ABOPT_CHECK_ARG(iters >= 0 && iters <= RX_MAX_ITERS, "relax_grouped: iters must be 0 .. %d (got %d)", RX_MAX_ITERS, iters);
    ABOPT_CHECK_ARG(max_moved >= 1, "relax_grouped: max_moved must be >= 1 (got %d)", max_moved);
    const int mx = std::min(max_moved, L);
    if (mx > RX_MAX_MOVED) {
        set_error("relax_grouped: max_moved=%d moved residues per candidate exceed the maximum of %d", mx, RX_MAX_MOVED);
        return ABOPT_EUNSUPPORTED;
    }
    if (G == 0 || S == 0) return ABOPT_OK;
    if ((rc = check_group_count("relax_grouped", G)) != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(pos_in && pos_out && mask && move && energy, "relax_grouped: NULL argument");
    const int tl = std::min(RX_TILE, (L + 63) & ~63);
    static LdsConfig lds_cfg;                                                   // granted once, for the largest call there can be: nothing changes under a capture
    if ((rc = ensure_dynamic_lds(reinterpret_cast<const void*>(relax_kernel), RelaxLds::bytes(RX_MAX_MOVED, kMaxAtoms, RX_TILE), lds_cfg)) != ABOPT_OK) return rc;
    const RelaxKnobs kn = {w_bond, w_ca, w_clash, w_tether, clash_d, step, max_shift, max_angle, iters};
    hipLaunchKernelGGL(relax_kernel, fold_grid((int64_t)G * S, 1u), dim3(256), RelaxLds::bytes(mx, A, tl), (hipStream_t)stream, pos_in, pos_out, mask,
                       mask_shared ? 1 : 0, move, link, energy, G * S, S, L, A, mx, tl, kn);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}
