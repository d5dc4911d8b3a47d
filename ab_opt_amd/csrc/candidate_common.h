// What the kernels that work on docked candidates share (interface.hip, sasa.hip, guide.hip, relax.hip, develop.hip, interface_energy.hip, backbone.hip; DESIGN.md sections 3.12, 6.3, 6.6, 6.8, 6.9, 6.10, 6.13): G groups of S
// candidates of L residues with A atom slots, a row per group that names the residues' sides or flags them, a grid of (candidate folded over x and y, slice in z),
// and the argument checks of their entry points.  sasa.hip, guide.hip, relax.hip, develop.hip, interface_energy.hip and backbone.hip compile under `#pragma clang fp contract(off)` and include this header BEFORE
// the pragma.  d2_fma is the only floating-point arithmetic of this file: its fmaf chain is spelled out, so it means the same on either side of the pragma
// (guide.hip and develop.hip use it; sasa.hip, relax.hip, interface_energy.hip and backbone.hip, whose every step is rounded once, do not).
// similarity.hip (section 6.11) and superpose.hip (section 6.12), which compare rows of two panels and have no groups, take the folded grid and compact_ranks
// from here (similarity.hip d2_fma too).
#pragma once
#include <math.h>
#include <algorithm>
#include "abopt_common.h"

namespace abopt {

constexpr int kMaxAtoms = 15;              // atoms per residue: the project's maximum (pos_heavyatom)
constexpr int kMaxGroups = 65535;          // groups of one call
constexpr int kMaxSlices = 64;             // workgroups a candidate is split over at most
constexpr int kGridX = 1 << 22;            // workgroups along x: the rest folds into y (x times the 256 threads of a workgroup has to stay under 2^32)

// ---------------------------------------------------------------- device side
// The ONE fused distance: fmaf(dz, dz, fmaf(dy, dy, dx dx)) with every step rounded once, spelled so that the compiler contracts nothing differently in
// different places.  (x - y)^2 == (y - x)^2, so d2(p, q) == d2(q, p) bit for bit.  The three-argument form takes the differences.
__device__ __forceinline__ float d2_fma(float dx, float dy, float dz) { return fmaf(dz, dz, fmaf(dy, dy, __fmul_rn(dx, dx))); }
__device__ __forceinline__ float d2_fma(float ax, float ay, float az, float bx, float by, float bz) {
    return d2_fma(__fsub_rn(ax, bx), __fsub_rn(ay, by), __fsub_rn(az, bz));
}

// false for a NaN and for +-inf: a comparison, no arithmetic
__device__ __forceinline__ bool finite_f32(float x) { return fabsf(x) < INFINITY; }

// index of the workgroup in a grid folded by fold_grid: the caller returns if its candidate (or unit) lies beyond the last one, in the grid's last row
__device__ __forceinline__ int64_t folded_block() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }

// predicates on a residue index, for take and slice_ranks
struct OnSide {                            // the residue is on `side` of its group row
    const int32_t* grp;
    int side;
    __device__ __forceinline__ bool operator()(int r) const { return grp[r] == side; }
};
struct OnEitherSide {                      // the residue takes part: side 1 or 2
    const int32_t* grp;
    __device__ __forceinline__ bool operator()(int r) const { const int s = grp[r]; return s == 1 || s == 2; }
};

// Wave-uniform: append the residues r >= cur of the row [0, L) with pred(r) to idx[0 .. cap), in index order, until `cap` are found or the row ends; cur moves
// past the last residue taken.  Every wave of the workgroup runs this with the same arguments and gets the same answer (no exchange needed); `write` picks the
// one that stores.  idx == nullptr with write == false just skips `cap` such residues.
template <class Pred>
__device__ __forceinline__ int take(int L, Pred pred, int& cur, int cap, int* idx, bool write) {
    const int lane = threadIdx.x & 63;
    int n = 0;
    while (n < cap && cur < L) {
        const int r = cur + lane;
        const bool f = r < L && pred(r);
        const unsigned long long b = __ballot(f);
        const int pos = n + __popcll(b & ((1ull << lane) - 1ull));
        if (write && f && pos < cap) idx[pos] = r;
        const int tot = __popcll(b);
        if (n + tot >= cap) {
            cur += __ffsll((long long)__ballot(f && pos == cap - 1));            // the lane that filled the last place: 1-based, so this is "one past it"
            n = cap;
        } else {
            n += tot;
            cur += 64;
        }
    }
    return n;
}

// Wave-uniform: the residues with pred(r) are numbered in index order and slice s of `slices` owns the ranks [n s / slices, n (s + 1) / slices).  Returns how
// many this slice owns and leaves cur at the first of them, for take.  Every wave counts the row itself (no exchange).
template <class Pred>
__device__ __forceinline__ int slice_ranks(int L, Pred pred, int slice, int slices, int& cur) {
    const int lane = threadIdx.x & 63;
    int n = 0;
    for (int r0 = 0; r0 < L; r0 += 64) n += __popcll(__ballot(r0 + lane < L && pred(r0 + lane)));
    const int lo = (int)((int64_t)n * slice / slices), hi = (int)((int64_t)n * (slice + 1) / slices);
    cur = 0;
    if (lo < hi) take(L, pred, cur, lo, nullptr, false);
    return hi - lo;
}

// Wave-uniform: the elements k < n of a row with mask[k] != 0 (mask == NULL: all), in order, are numbered 0 .. len - 1 and put(rank, k) is called for each by the
// lane that holds it.  -> len.  The ranks come from a ballot prefix per 64 elements.
template <class Put>
__device__ __forceinline__ int compact_ranks(const uint8_t* __restrict__ mask, int n, Put put) {
    const int lane = threadIdx.x & 63;
    int len = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const bool f = k < n && (mask == nullptr || mask[k] != 0);
        const unsigned long long b = __ballot(f);
        if (f) put(len + __popcll(b & ((1ull << lane) - 1ull)), k);
        len += __popcll(b);
    }
    return len;
}

// ---------------------------------------------------------------- host side
// `blocks` workgroups along x, folded into y beyond kGridX; z as given
inline dim3 fold_grid(int64_t blocks, unsigned z) {
    const int64_t x = std::min<int64_t>(blocks, kGridX);
    return dim3((unsigned)x, (unsigned)((blocks + x - 1) / x), z);
}

// Slices in z: enough for `per_cu` workgroups on every CU when there are `units` in x and y, no more than the work of one unit splits into, at most `max`.
inline int slice_count(int cus, int per_cu, int64_t units, int64_t split, int max = kMaxSlices) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(max, split), ((int64_t)cus * per_cu + units - 1) / units));
}

// G groups of S candidates of L residues with 1 .. kMaxAtoms atom slots
inline int check_candidate_dims(const char* name, int G, int S, int L, int A) {
    ABOPT_CHECK_ARG(G >= 0 && S >= 0 && L >= 1 && A >= 1 && (int64_t)G * S <= 0x7fffffff && (int64_t)L * A * 3 <= 0x7fffffff,
                    "%s: bad dims G=%d S=%d L=%d A=%d", name, G, S, L, A);
    ABOPT_CHECK_ARG(A <= kMaxAtoms, "%s: A=%d atoms per residue exceed the maximum of %d", name, A, kMaxAtoms);
    return ABOPT_OK;
}

// after the G == 0 || S == 0 no-op of the caller: a group is a row of some grid
inline int check_group_count(const char* name, int G) {
    ABOPT_CHECK_ARG(G <= kMaxGroups, "%s: G=%d groups exceed one launch (max %d)", name, G, kMaxGroups);
    return ABOPT_OK;
}

// each of the n named scalars is finite and >= 0
inline int check_nonnegative(const char* name, const char* const* names, const float* v, int n) {
    for (int k = 0; k < n; ++k) ABOPT_CHECK_ARG(isfinite(v[k]) && v[k] >= 0.f, "%s: %s must be finite and >= 0 (got %g)", name, names[k], (double)v[k]);
    return ABOPT_OK;
}

inline int check_workspace(const char* name, const void* ws, int align, size_t ws_bytes, size_t need) {
    ABOPT_CHECK_ARG(((uintptr_t)ws & (uintptr_t)(align - 1)) == 0, "%s: the workspace must be %d-byte aligned", name, align);
    if (ws_bytes < need) { set_error("%s: workspace too small (%zu bytes given, %zu needed)", name, ws_bytes, need); return ABOPT_EWORKSPACE; }
    return ABOPT_OK;
}

}  // namespace abopt
