// Greedy clustering of docked poses on the device: the step every docking tool puts after its sampler -- near-duplicate
// poses are merged into binding modes, each reported by one representative and its population.  Nothing in the reference is matched; the
// definition is this project's own (include/abopt.h: abopt_cluster_poses_grouped):
//   distance   RMSD over the n points WITHOUT superposition (commonness_kernel's distance: all poses of a complex live in the antigen's frame)
//   neighbours ssd(a, b) = sum_k |a_k - b_k|^2 <= cutoff^2 n; the diagonal is always set
//   greedy     the alive structure with the most alive neighbours (ties: lowest index) becomes a centre, its alive neighbours its members
// Two launches: pose_adjacency_kernel writes the neighbour relation as a bit matrix (and every row's population), greedy_cluster_kernel walks it.
// Designed sequences are clustered by the same walk over the Hamming relation of seq_adjacency_kernel, and sequence_profile_kernel counts a group's
// per-position composition (abopt_cluster_sequences_grouped, abopt_sequence_profile_grouped).  Loop shapes are clustered by the walk
// over a third relation, the RMSD after best-fit superposition of shape_adjacency_kernel (abopt_cluster_shapes_grouped).
#include <math.h>
#include "abopt_common.h"
#include "kernels.h"
#include "superpose.h"

namespace abopt {

constexpr int CL_MAX_S = 16384;            // structures per group: the greedy kernel's LDS state (4 S + S / 4 bytes) stays under 160 KB
constexpr int CL_KC = 48;                  // coordinates (16 points) of 64 rows and 64 columns staged in LDS at a time: 24.3 KB, any n
constexpr int CL_ROWS = 16;                // rows a wave carries at once: 4 waves x 16 = the 64-row tile
constexpr int CL_THREADS = 1024;

// bit (row a, column b) of group g = ssd(a, b) <= thr, or a == b.  Grid (64-row tile, group), 4 waves: a wave owns 16 rows of the tile and walks the
// group's columns 64 at a time; lane j carries ssd(row, column 64 cb + j) of each of its rows as ONE fmaf chain over the 3 n coordinates in index order.
// (x - y)^2 == (y - x)^2 in floating point and the order is the same for (a, b) and (b, a), so the relation and the optional rmsd matrix are symmetric
// bit for bit.  The workgroup stages 48 coordinates of its 64 rows and of the 64 columns in LDS per step (coalesced loads, each column read once per
// 64 rows; a short last chunk is zero-filled: fmaf(0, 0, s) == s, the chain's bits do not change); the row operand is a broadcast read, the column
// operand is one read per 16 fmaf (stride 49: conflict-free).  __ballot IS the 64-bit word of the bit row (columns past S: 0); lane 0 stores it and, at
// the end of the row, the row's population.
__global__ __launch_bounds__(256) void pose_adjacency_kernel(const float* __restrict__ x_all, unsigned long long* __restrict__ bits_all,
                                                             int32_t* __restrict__ pop_all, float* __restrict__ rmsd_all, int S, int n, float thr) {
    __shared__ __attribute__((aligned(16))) float row_sh[64][CL_KC];
    __shared__ float col_sh[64][CL_KC + 1];
    const int g = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int W = (S + 63) >> 6, n3 = n * 3, r0 = blockIdx.x * 64;
    const float* x = x_all + (int64_t)g * S * n3;
    int pop[CL_ROWS];
#pragma unroll
    for (int q = 0; q < CL_ROWS; ++q) pop[q] = 0;
    for (int cb = 0; cb < W; ++cb) {
        float s[CL_ROWS];
#pragma unroll
        for (int q = 0; q < CL_ROWS; ++q) s[q] = 0.f;
        for (int k0 = 0; k0 < n3; k0 += CL_KC) {
            __syncthreads();                                                   // the previous chunk's reads are done
            for (int idx = tid; idx < 64 * CL_KC; idx += 256) {
                const int rr = idx / CL_KC, k = idx % CL_KC;
                const bool in = k0 + k < n3;
                const int r = min(r0 + rr, S - 1), c = min(cb * 64 + rr, S - 1);   // rows / columns past S read the last structure and are masked below
                row_sh[rr][k] = in ? x[(int64_t)r * n3 + k0 + k] : 0.f;
                col_sh[rr][k] = in ? x[(int64_t)c * n3 + k0 + k] : 0.f;
            }
            __syncthreads();
#pragma unroll 4
            for (int k = 0; k < CL_KC; ++k) {
                const float c = col_sh[lane][k];
#pragma unroll
                for (int q = 0; q < CL_ROWS; ++q) { const float d = row_sh[wave * CL_ROWS + q][k] - c; s[q] = fmaf(d, d, s[q]); }
            }
        }
        const int col = cb * 64 + lane;
        const bool valid = col < S;
#pragma unroll
        for (int q = 0; q < CL_ROWS; ++q) {
            const int r = r0 + wave * CL_ROWS + q;
            if (r >= S) break;                                                  // wave-uniform
            const unsigned long long word = __ballot(valid && (s[q] <= thr || col == r));
            if (lane == 0) bits_all[((int64_t)g * S + r) * W + cb] = word;
            pop[q] += __popcll(word);
            if (rmsd_all && valid) rmsd_all[((int64_t)g * S + r) * S + col] = sqrtf(s[q] / (float)n);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < CL_ROWS; ++q) {
            const int r = r0 + wave * CL_ROWS + q;
            if (r < S) pop_all[(int64_t)g * S + r] = pop[q];
        }
    }
}

// 64-bit max over the workgroup's 16 waves; every thread gets the result.  red[16]; two barriers.
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* red) {
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    __syncthreads();                                                           // the previous round's reads of red[] are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = red[0];
#pragma unroll
    for (int w = 1; w < CL_THREADS / 64; ++w) m = red[w] > m ? red[w] : m;
    return m;
}

// ONE 1024-thread workgroup per group.  LDS: cnt[S] (alive neighbours of every alive structure, itself included), alive[W], mem[W] (the members of
// the cluster being cut out).  Per iteration:
//   pick     max over the alive structures of the key (cnt << 32 | ~index): count descending, index ascending; S / 1024 keys per thread + one
//            16-wave reduction.  Deterministic: integers.
//   cut      mem = row(centre) & alive; alive &= ~mem; the cluster's size is cnt[centre] (the invariant above).
//   update   INCREMENTAL: every member m is visited once (a wave per member, its bit row read ONCE in the whole call) and takes 1 off cnt[j] of every
//            surviving neighbour j (row(m) & alive; the relation is symmetric, so these are the structures that counted m).  LDS integer atomics: the
//            order does not matter.  Over the whole call that is one pass over the bit matrix (S W words) + one LDS atomic per (dying, surviving)
//            neighbour pair, against S W words PER ITERATION for a recount.
//   tail     once the largest count is 1 every structure left is a singleton: they are numbered in index order in ONE pass (a docking run's tail of
//            isolated poses is most of the iterations otherwise).
// An iteration costs 4 barriers, S / 1024 LDS reads per thread and W / 64 word loads per wave and member.
__global__ __launch_bounds__(CL_THREADS) void greedy_cluster_kernel(const unsigned long long* __restrict__ bits_all, const int32_t* __restrict__ pop_all,
                                                                    int32_t* __restrict__ label_all, int32_t* __restrict__ centre_all,
                                                                    int32_t* __restrict__ size_all, int32_t* __restrict__ count_all, int S, int max_clusters) {
    extern __shared__ unsigned long long cl_lds[];
    const int g = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int W = (S + 63) >> 6;
    unsigned long long* alive = cl_lds;                  // [W]
    unsigned long long* mem = alive + W;                 // [W]
    unsigned long long* red = mem + W;                   // [16]
    int* cnt = (int*)(red + CL_THREADS / 64);            // [S]
    const unsigned long long* bits = bits_all + (int64_t)g * S * W;
    int32_t* label = label_all + (int64_t)g * S;
    int32_t* centre = centre_all + (int64_t)g * S;
    int32_t* size = size_all + (int64_t)g * S;
    for (int i = tid; i < S; i += CL_THREADS) cnt[i] = pop_all[(int64_t)g * S + i];
    for (int w = tid; w < W; w += CL_THREADS) alive[w] = (w * 64 + 64 <= S) ? ~0ull : ((1ull << (S - w * 64)) - 1ull);
    __syncthreads();
    const int cap = max_clusters > 0 ? min(max_clusters, S) : S;
    int found = 0;
    while (found < cap) {
        unsigned long long key = 0ull;
        for (int i = tid; i < S; i += CL_THREADS)
            if ((alive[i >> 6] >> (i & 63)) & 1ull) {
                const unsigned long long k = ((unsigned long long)(unsigned)cnt[i] << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
                key = k > key ? k : key;
            }
        key = block_max_u64(key, red);
        if (key == 0ull) break;                                                 // nobody alive (block-uniform)
        if ((key >> 32) == 1ull) {
            // the largest count is 1: nobody alive has an alive neighbour but itself, so the rest are singletons and the picks would take them in index order.
            // One pass instead of one iteration each: cluster number = found + rank among the alive (a prefix sum over the words' populations, in mem[]).
            for (int w = tid; w < W; w += CL_THREADS) mem[w] = (unsigned long long)__popcll(alive[w]);
            __syncthreads();
            if (tid == 0) {
                unsigned long long run = 0ull;
                for (int w = 0; w < W; ++w) { const unsigned long long t = mem[w]; mem[w] = run; run += t; }
                red[0] = run;
            }
            __syncthreads();
            const int rest = (int)red[0];
            for (int i = tid; i < S; i += CL_THREADS) {
                const unsigned long long a = alive[i >> 6];
                if (!((a >> (i & 63)) & 1ull)) continue;
                const int cl = found + (int)mem[i >> 6] + __popcll(a & ((1ull << (i & 63)) - 1ull));
                label[i] = cl < cap ? cl : -1;                                  // past the cap: left over
                if (cl < cap) { centre[cl] = i; size[cl] = 1; }
            }
            __syncthreads();
            for (int w = tid; w < W; w += CL_THREADS) alive[w] = 0ull;
            found = min(cap, found + rest);
            __syncthreads();
            break;
        }
        const int c = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
        if (tid == 0) { centre[found] = c; size[found] = (int)(key >> 32); }
        for (int w = tid; w < W; w += CL_THREADS) {
            const unsigned long long a = alive[w], m = bits[(int64_t)c * W + w] & a;
            mem[w] = m;
            alive[w] = a & ~m;
        }
        __syncthreads();
        for (int w = wave; w < W; w += CL_THREADS / 64) {
            unsigned long long mw = mem[w];                                     // wave-uniform
            while (mw) {
                const int m = w * 64 + __ffsll((long long)mw) - 1;
                mw &= mw - 1ull;
                if (lane == 0) label[m] = found;
                const unsigned long long* mrow = bits + (int64_t)m * W;
                for (int ww = lane; ww < W; ww += 64) {
                    unsigned long long nb = mrow[ww] & alive[ww];
                    while (nb) {
                        const int j = ww * 64 + __ffsll((long long)nb) - 1;
                        nb &= nb - 1ull;
                        atomicSub(&cnt[j], 1);
                    }
                }
            }
        }
        __syncthreads();
        ++found;
    }
    // structures still alive at the cap keep label -1; centre / size are padded with -1 / 0
    for (int i = tid; i < S; i += CL_THREADS) {
        if ((alive[i >> 6] >> (i & 63)) & 1ull) label[i] = -1;
        if (i >= found) { centre[i] = -1; size[i] = 0; }
    }
    if (tid == 0) count_all[g] = found;
}

// ---- Sequence clustering: the same greedy walk over another relation.
//   distance   d(a, b) = number of positions whose bytes differ (Hamming; the bytes are compared for equality only)
//   neighbours d(a, b) <= max_mismatch; the diagonal is always set
constexpr int SQ_KW = 16;                  // 4-byte words (64 residues) of 64 rows and 64 columns staged in LDS at a time: 8.3 KB, any n

// number of non-zero bytes of x: bit 7 of every byte of ((x & 0x7f..) + 0x7f..) | x is set iff the byte is non-zero (no carry leaves a byte)
__device__ __forceinline__ int nonzero_bytes(unsigned x) {
    return __popc((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u);
}

// 4 consecutive residues of a sequence as one word; positions past n read as 0 on both sides of every comparison, so the padding adds no mismatch
__device__ __forceinline__ unsigned seq_word(const uint8_t* __restrict__ row, int k, int n) {
    unsigned w = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (k + b < n) w |= (unsigned)row[k + b] << (8 * b);
    return w;
}

// The sequence twin of pose_adjacency_kernel: the same grid (64-row tile, group), the same 4 waves x 16 rows, lane j = column 64 cb + j, the same outputs
// (bit rows through __ballot, row populations, every word written once by lane 0).  The workgroup stages 64 residues of its 64 rows and of the 64 columns per
// step as 16 packed words each (lane-adjacent byte loads; a short last chunk only stages and walks the words it has); the row operand is a broadcast read,
// the column operand one read per 16 comparisons (stride 17: conflict-free).  A comparison is XOR + nonzero_bytes: 4 residues per 5 integer instructions.
// Integers only: d is exact and d(a, b) == d(b, a), so the relation and the optional dist matrix are symmetric.
__global__ __launch_bounds__(256) void seq_adjacency_kernel(const uint8_t* __restrict__ seq_all, unsigned long long* __restrict__ bits_all,
                                                            int32_t* __restrict__ pop_all, int32_t* __restrict__ dist_all, int S, int n, int max_mismatch) {
    __shared__ unsigned row_sh[64][SQ_KW];
    __shared__ unsigned col_sh[64][SQ_KW + 1];
    const int g = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int W = (S + 63) >> 6, r0 = blockIdx.x * 64;
    const uint8_t* x = seq_all + (int64_t)g * S * n;
    int pop[CL_ROWS];
#pragma unroll
    for (int q = 0; q < CL_ROWS; ++q) pop[q] = 0;
    for (int cb = 0; cb < W; ++cb) {
        int d[CL_ROWS];
#pragma unroll
        for (int q = 0; q < CL_ROWS; ++q) d[q] = 0;
        for (int k0 = 0; k0 < n; k0 += 4 * SQ_KW) {
            const int kw = min(SQ_KW, (n - k0 + 3) >> 2);                      // words this chunk holds (block-uniform)
            __syncthreads();                                                   // the previous chunk's reads are done
            for (int idx = tid; idx < 64 * kw; idx += 256) {
                const int rr = idx / kw, w = idx % kw;
                const int r = min(r0 + rr, S - 1), c = min(cb * 64 + rr, S - 1);   // rows / columns past S read the last sequence and are masked below
                row_sh[rr][w] = seq_word(x + (int64_t)r * n, k0 + 4 * w, n);
                col_sh[rr][w] = seq_word(x + (int64_t)c * n, k0 + 4 * w, n);
            }
            __syncthreads();
            for (int w = 0; w < kw; ++w) {
                const unsigned c = col_sh[lane][w];
#pragma unroll
                for (int q = 0; q < CL_ROWS; ++q) d[q] += nonzero_bytes(row_sh[wave * CL_ROWS + q][w] ^ c);
            }
        }
        const int col = cb * 64 + lane;
        const bool valid = col < S;
#pragma unroll
        for (int q = 0; q < CL_ROWS; ++q) {
            const int r = r0 + wave * CL_ROWS + q;
            if (r >= S) break;                                                  // wave-uniform
            const unsigned long long word = __ballot(valid && (d[q] <= max_mismatch || col == r));
            if (lane == 0) bits_all[((int64_t)g * S + r) * W + cb] = word;
            pop[q] += __popcll(word);
            if (dist_all && valid) dist_all[((int64_t)g * S + r) * S + col] = d[q];
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < CL_ROWS; ++q) {
            const int r = r0 + wave * CL_ROWS + q;
            if (r < S) pop_all[(int64_t)g * S + r] = pop[q];
        }
    }
}

// ---- Shape clustering: the same greedy walk over a third relation, the RMSD AFTER best-fit superposition on all n points.
//   distance   ss(a, b) = min over proper rotations and translations of sum_k |R a_k + t - b_k|^2, by superpose_pair (superpose.h) in double
//   neighbours ss(a, b) <= cutoff^2 n; the diagonal is always set
constexpr int SH_MAXLEN = 256;             // points of a structure: the row length abopt_superposed_rmsd takes

struct RowPoint {                          // the k-th point of a structure in global memory, as double
    const float* row;
    __device__ __forceinline__ void operator()(int k, double p[3]) const { p[0] = (double)row[3 * k]; p[1] = (double)row[3 * k + 1]; p[2] = (double)row[3 * k + 2]; }
};

constexpr int SH_ROWS = 4;                 // rows of a workgroup: one per wave

// The shape twin of pose_adjacency_kernel: the same outputs (bit rows through __ballot, lane j = column 64 cb + j, row populations, every word written once by
// lane 0).  A lane computes its pair from start to finish with superpose_pair and shares nothing, so nothing is staged and a workgroup gains nothing from many
// rows: grid (4-row tile, group), a wave per row -- S / 4 workgroups, where the 64-row tile of the pose kernel would leave three quarters of the CUs idle at
// S = 4096 and one wave per SIMD at S = 16384.  The rows come straight from global memory (a wave's 64 columns are 64 runs of 12 n bytes that the tile's 4 waves
// read together, out of the caches; three passes over them).  The greedy kernel needs a relation that is symmetric bit for bit and a best fit is not symmetric
// in floating point, so the pair (a, b) is ALWAYS evaluated as (x = row min(a, b), y = row max(a, b)): the lanes that own (a, b) and (b, a) run the same
// instructions on the same values.  A structure holding a NaN has ss = NaN against everything, which is no neighbour; its diagonal bit is set like every other.
__global__ __launch_bounds__(SH_ROWS * 64) void shape_adjacency_kernel(const float* __restrict__ x_all, unsigned long long* __restrict__ bits_all,
                                                                       int32_t* __restrict__ pop_all, float* __restrict__ rmsd_all, int S, int n, double thr) {
    const int g = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int W = (S + 63) >> 6, n3 = n * 3, r = blockIdx.x * SH_ROWS + wave;
    if (r >= S) return;                                                         // wave-uniform; this kernel has no barrier
    const float* x = x_all + (int64_t)g * S * n3;
    int pop = 0;
    for (int cb = 0; cb < W; ++cb) {
        const int col = cb * 64 + lane;
        const bool valid = col < S;
        const int c = min(col, S - 1);                                          // columns past S read the last structure and are masked below
        const int lo = min(r, c), hi = max(r, c);
        const RowPoint a{x + (int64_t)lo * n3}, b{x + (int64_t)hi * n3};
        double rot[9], tr[3];
        const double ss = superpose_pair(n, n, a, b, a, b, rot, tr);
        const unsigned long long word = __ballot(valid && (ss <= thr || col == r));
        if (lane == 0) bits_all[((int64_t)g * S + r) * W + cb] = word;
        pop += __popcll(word);
        if (rmsd_all && valid) rmsd_all[((int64_t)g * S + r) * S + col] = col == r ? 0.f : superposed_rmsd_of(ss, n);
    }
    if (lane == 0) pop_all[(int64_t)g * S + r] = pop;
}

constexpr int PF_TILE = 64;                // positions a workgroup owns
constexpr int PF_BINS = 21;                // the 20 residue types + everything else

// counts[g, p, t] = how many of the group's S sequences hold type t at position p (bin 20: every byte >= 20).  Grid (64-position tile, group), 256 threads:
// the workgroup walks its S x tile bytes in index order -- lane-adjacent bytes along n, whole rows back to back when the tile holds all of n -- and counts
// into an LDS histogram with LDS integer atomics; the tile's counts are one contiguous run of the output and leave by plain stores.
__global__ __launch_bounds__(256) void sequence_profile_kernel(const uint8_t* __restrict__ seq_all, int32_t* __restrict__ counts_all, int S, int n) {
    __shared__ int hist[PF_TILE * PF_BINS];
    const int g = blockIdx.y, tid = threadIdx.x, p0 = blockIdx.x * PF_TILE;
    const int tl = min(PF_TILE, n - p0);
    const uint8_t* x = seq_all + (int64_t)g * S * n + p0;
    for (int i = tid; i < tl * PF_BINS; i += 256) hist[i] = 0;
    __syncthreads();
    const int64_t total = (int64_t)S * tl;
    for (int64_t e = tid; e < total; e += 256) {
        const int s = (int)(e / tl), p = (int)(e - (int64_t)s * tl);
        const int t = min((int)x[(int64_t)s * n + p], PF_BINS - 1);
        atomicAdd(&hist[p * PF_BINS + t], 1);
    }
    __syncthreads();
    int32_t* out = counts_all + ((int64_t)g * n + p0) * PF_BINS;
    for (int i = tid; i < tl * PF_BINS; i += 256) out[i] = hist[i];
}

static LdsConfig g_cluster_lds;

// The greedy kernel's dynamic LDS for groups of S, made available before anything is launched ...
static int greedy_prepare(int S, size_t* lds) {
    const int W = (S + 63) / 64;
    *lds = (size_t)(2 * W + CL_THREADS / 64) * 8 + (size_t)S * 4;
    return ensure_dynamic_lds((const void*)greedy_cluster_kernel, *lds, g_cluster_lds);
}

// ... and its launch on a neighbour relation (bit matrix + populations) some adjacency kernel has written to the workspace: all three entries end here
static int greedy_launch(const unsigned long long* bits, const int32_t* pop, void* label, void* centre, void* size, void* count, int G, int S, int max_clusters,
                         size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(greedy_cluster_kernel, dim3((unsigned)G), dim3(CL_THREADS), lds, st, bits, pop, (int32_t*)label, (int32_t*)centre, (int32_t*)size,
                       (int32_t*)count, S, max_clusters);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}

}  // namespace abopt

using namespace abopt;

// bit matrix [G, S, ceil(S / 64)] of 8-byte words | populations [G, S] int32
extern "C" size_t abopt_cluster_ws_bytes(int G, int S) {
    if (G <= 0 || S <= 0 || S > CL_MAX_S) return 0;                             // nothing to do / unsupported: the call itself says which
    const size_t W = ((size_t)S + 63) / 64;
    return (size_t)G * S * W * 8 + (((size_t)G * S * 4 + 7) & ~(size_t)7);
}

extern "C" int abopt_cluster_poses_grouped(const float* structs, int G, int S, int n, float cutoff, int max_clusters, void* ws, size_t ws_bytes,
                                           void* label, void* centre, void* size, void* count, float* rmsd, abopt_stream stream) {
    ABOPT_CHECK_ARG(G >= 0 && S >= 1 && n >= 1 && max_clusters >= 0 && (int64_t)G * S <= 0x7fffffff && (int64_t)n * 3 <= 0x7fffffff,
                    "cluster_poses_grouped: bad dims G=%d S=%d n=%d max_clusters=%d", G, S, n, max_clusters);
    if (S > CL_MAX_S) { set_error("cluster_poses_grouped: S=%d structures per group exceed the greedy kernel's LDS state (max %d)", S, CL_MAX_S); return ABOPT_EUNSUPPORTED; }
    ABOPT_CHECK_ARG(isfinite(cutoff) && cutoff >= 0.f, "cluster_poses_grouped: the cutoff must be finite and >= 0 (got %g)", (double)cutoff);
    if (G == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(G <= 65535, "cluster_poses_grouped: G=%d groups exceed one launch (max 65535)", G);
    ABOPT_CHECK_ARG(structs && ws && label && centre && size && count, "cluster_poses_grouped: NULL argument");
    ABOPT_CHECK_ARG(((uintptr_t)ws & 7) == 0, "cluster_poses_grouped: the workspace must be 8-byte aligned");
    if (ws_bytes < abopt_cluster_ws_bytes(G, S)) { set_error("cluster_poses_grouped: workspace too small (%zu bytes given)", ws_bytes); return ABOPT_EWORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    const int W = (S + 63) / 64;
    unsigned long long* bits = (unsigned long long*)ws;
    int32_t* pop = (int32_t*)(bits + (size_t)G * S * W);
    const float thr = (float)((double)cutoff * (double)cutoff * (double)n);      // +inf for a huge cutoff: every finite pair is a neighbour
    size_t lds;
    int rc = greedy_prepare(S, &lds);
    if (rc != ABOPT_OK) return rc;
    hipLaunchKernelGGL(pose_adjacency_kernel, dim3((unsigned)W, (unsigned)G), dim3(256), 0, st, structs, bits, pop, rmsd, S, n, thr);
    ABOPT_LAUNCH_CHECK();
    return greedy_launch(bits, pop, label, centre, size, count, G, S, max_clusters, lds, st);
}

extern "C" int abopt_cluster_shapes_grouped(const float* structs, int G, int S, int n, float cutoff, int max_clusters, void* ws, size_t ws_bytes,
                                            void* label, void* centre, void* size, void* count, float* rmsd, abopt_stream stream) {
    ABOPT_CHECK_ARG(G >= 0 && S >= 1 && n >= 3 && max_clusters >= 0 && (int64_t)G * S <= 0x7fffffff,
                    "cluster_shapes_grouped: bad dims G=%d S=%d n=%d max_clusters=%d (a best fit takes n >= 3 points)", G, S, n, max_clusters);
    if (S > CL_MAX_S) { set_error("cluster_shapes_grouped: S=%d structures per group exceed the greedy kernel's LDS state (max %d)", S, CL_MAX_S); return ABOPT_EUNSUPPORTED; }
    if (n > SH_MAXLEN) { set_error("cluster_shapes_grouped: n=%d points per structure exceed the maximum of %d", n, SH_MAXLEN); return ABOPT_EUNSUPPORTED; }
    ABOPT_CHECK_ARG(isfinite(cutoff) && cutoff >= 0.f, "cluster_shapes_grouped: the cutoff must be finite and >= 0 (got %g)", (double)cutoff);
    if (G == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(G <= 65535, "cluster_shapes_grouped: G=%d groups exceed one launch (max 65535)", G);
    ABOPT_CHECK_ARG(structs && ws && label && centre && size && count, "cluster_shapes_grouped: NULL argument");
    ABOPT_CHECK_ARG(((uintptr_t)ws & 7) == 0, "cluster_shapes_grouped: the workspace must be 8-byte aligned");
    if (ws_bytes < abopt_cluster_ws_bytes(G, S)) { set_error("cluster_shapes_grouped: workspace too small (%zu bytes given)", ws_bytes); return ABOPT_EWORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    const int W = (S + 63) / 64;
    unsigned long long* bits = (unsigned long long*)ws;
    int32_t* pop = (int32_t*)(bits + (size_t)G * S * W);
    const double thr = (double)cutoff * (double)cutoff * (double)n;             // finite for every finite cutoff: a huge one makes every finite pair a neighbour
    size_t lds;
    int rc = greedy_prepare(S, &lds);
    if (rc != ABOPT_OK) return rc;
    hipLaunchKernelGGL(shape_adjacency_kernel, dim3((unsigned)((S + SH_ROWS - 1) / SH_ROWS), (unsigned)G), dim3(SH_ROWS * 64), 0, st, structs, bits, pop, rmsd, S, n, thr);
    ABOPT_LAUNCH_CHECK();
    return greedy_launch(bits, pop, label, centre, size, count, G, S, max_clusters, lds, st);
}

extern "C" int abopt_cluster_sequences_grouped(const uint8_t* seqs, int G, int S, int n, int max_mismatch, int max_clusters, void* ws, size_t ws_bytes,
                                               void* label, void* centre, void* size, void* count, void* dist, abopt_stream stream) {
    ABOPT_CHECK_ARG(G >= 0 && S >= 1 && n >= 1 && max_clusters >= 0 && (int64_t)G * S <= 0x7fffffff,
                    "cluster_sequences_grouped: bad dims G=%d S=%d n=%d max_clusters=%d", G, S, n, max_clusters);
    if (S > CL_MAX_S) { set_error("cluster_sequences_grouped: S=%d sequences per group exceed the greedy kernel's LDS state (max %d)", S, CL_MAX_S); return ABOPT_EUNSUPPORTED; }
    ABOPT_CHECK_ARG(max_mismatch >= 0, "cluster_sequences_grouped: max_mismatch must be >= 0 (got %d)", max_mismatch);
    if (G == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(G <= 65535, "cluster_sequences_grouped: G=%d groups exceed one launch (max 65535)", G);
    ABOPT_CHECK_ARG(seqs && ws && label && centre && size && count, "cluster_sequences_grouped: NULL argument");
    ABOPT_CHECK_ARG(((uintptr_t)ws & 7) == 0, "cluster_sequences_grouped: the workspace must be 8-byte aligned");
    if (ws_bytes < abopt_cluster_ws_bytes(G, S)) { set_error("cluster_sequences_grouped: workspace too small (%zu bytes given)", ws_bytes); return ABOPT_EWORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    const int W = (S + 63) / 64;
    unsigned long long* bits = (unsigned long long*)ws;
    int32_t* pop = (int32_t*)(bits + (size_t)G * S * W);
    size_t lds;
    int rc = greedy_prepare(S, &lds);
    if (rc != ABOPT_OK) return rc;
    hipLaunchKernelGGL(seq_adjacency_kernel, dim3((unsigned)W, (unsigned)G), dim3(256), 0, st, seqs, bits, pop, (int32_t*)dist, S, n, max_mismatch);
    ABOPT_LAUNCH_CHECK();
    return greedy_launch(bits, pop, label, centre, size, count, G, S, max_clusters, lds, st);
}

extern "C" int abopt_sequence_profile_grouped(const uint8_t* seqs, int G, int S, int n, void* counts, abopt_stream stream) {
    ABOPT_CHECK_ARG(G >= 0 && S >= 1 && n >= 1 && (int64_t)G * n * PF_BINS <= 0x7fffffff, "sequence_profile_grouped: bad dims G=%d S=%d n=%d", G, S, n);
    if (G == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(G <= 65535, "sequence_profile_grouped: G=%d groups exceed one launch (max 65535)", G);
    ABOPT_CHECK_ARG(seqs && counts, "sequence_profile_grouped: NULL argument");
    hipLaunchKernelGGL(sequence_profile_kernel, dim3((unsigned)((n + PF_TILE - 1) / PF_TILE), (unsigned)G), dim3(256), 0, (hipStream_t)stream, seqs,
                       (int32_t*)counts, S, n);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}
