// Similarity of designs to reference sequences and loops on the device: the two numbers the reference's `eval` stage writes beside dG,
// `seqid` and `rmsd`, for sequences and residue lists of DIFFERENT lengths -- every one of Q query rows against every one of R reference rows.
//   abopt_align_sequences   global alignment with a substitution table and affine gaps, end gaps free (Gotoh 1982): score, matches, columns -- integers only;
//   abopt_gapped_rmsd       the reference's gapped CA sum of squared deviations (tools/eval/similarity.py: reslist_rmsd), no superposition: fp32 in a fixed order.
// One launch each, nothing allocated, no workspace, nothing synchronised, no atomic, every output written whole by plain stores.  Both are dynamic programmes
// with a data dependence along two axes: a wave owns a pair and walks the table as an anti-diagonal wavefront, a lane owning four columns and lagging its
// neighbour by one row; what crosses a lane boundary travels by one shuffle per step, and a wave runs in lockstep, so the wavefront needs no barrier.
// The definitions are in include/abopt.h; numpy restates them (tests/similarity_statement.py), the integers exactly and the fp32 sum bit for bit.
#include <math.h>
#include <algorithm>
#include "abopt_common.h"
#include "candidate_common.h"

// d2_fma of candidate_common.h, included BEFORE the pragma, is an explicit fmaf chain; the one other fp32 step of this file is the addition of a cell.
#pragma clang fp contract(off)

namespace abopt {

constexpr int SM_MAXLEN = 256;             // elements of a row: four per lane of the pair's wave
constexpr int SM_WAVES = 4;                // pairs of a workgroup
constexpr int SM_MAXT = 32;                // rows of a substitution table at most
// The three integers an alignment carries, all additive along its path, as ONE int64: score 2^32 + matches 2^16 - columns.  matches <= 256 and columns <= 512, so
// the low 32 bits never borrow from the score and the signed comparison of two such numbers is the lexicographic one of (score, matches, -columns): a
// transition is one 64-bit add and one max.
constexpr long long SM_SCORE = 1ll << 32;
constexpr long long SM_NEG = -(1ll << 62); // "no such alignment": far below every real one (|score| < 2^25), and 512 further steps of -32767 do not wrap it

__device__ __forceinline__ long long sm_max(long long a, long long b) { return a > b ? a : b; }

// ---------------------------------------------------------------- sequence alignment
// Grid folded over x and y, four waves, a wave per pair (query row q, reference row r).  The table is staged once per workgroup as int16 (entries are clamped
// into -32767 .. 32767), the two compacted sequences per wave.  The query runs down the rows (1 .. n) and the reference along the columns (1 .. m) of the Gotoh
// table; lane l owns the columns 4 l + 1 .. 4 l + 4 and computes row `step - l` at step `step`, so it finds the row above in its own registers and the column to
// its left -- H and Y of the row it is about to compute -- in what lane l - 1 left one step earlier.
//   H best alignment of the two prefixes; X the best one that ends with a query residue against a gap; Y the best one that ends with a gap against a reference residue
//   X[i][j] = max(H[i-1][j] + open, X[i-1][j] + extend),  Y[i][j] = max(H[i][j-1] + open, Y[i][j-1] + extend),  H = max(H[i-1][j-1] + pair, X, Y)
// (H holds X and Y themselves, so a run may also be continued at the price of opening one: never better, because gap_open <= gap_extend.)  Free end gaps: the
// first row and column cost nothing but their columns, and the result is the best of the last row and the last column, each with the overhang counted.
__global__ __launch_bounds__(SM_WAVES * 64) void align_sequences_kernel(const uint8_t* __restrict__ q_all, const uint8_t* __restrict__ qmask_all,
                                                                         const uint8_t* __restrict__ r_all, const uint8_t* __restrict__ rmask_all,
                                                                         const int32_t* __restrict__ table, int T, int gap_open, int gap_extend, int64_t pairs,
                                                                         int R, int na, int nb, int32_t* __restrict__ score_all,
                                                                         int32_t* __restrict__ matches_all, int32_t* __restrict__ columns_all) {
    __shared__ int16_t tab[SM_MAXT * SM_MAXT];
    __shared__ __attribute__((aligned(4))) uint8_t seq_a[SM_WAVES][SM_MAXLEN], seq_b[SM_WAVES][SM_MAXLEN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < T * T; k += SM_WAVES * 64) tab[k] = (int16_t)min(max(table[k], -32767), 32767);
    __syncthreads();                                                            // the one barrier: before any wave leaves
    const int64_t p = folded_block() * SM_WAVES + wave;
    if (p >= pairs) return;                                                     // wave-uniform
    const int64_t qi = p / R, ri = p - qi * R;
    uint8_t* a = seq_a[wave];
    uint8_t* b = seq_b[wave];
    for (int k = lane; k < SM_MAXLEN; k += 64) { a[k] = 0; b[k] = 0; }          // what lies past a sequence's end is read (by idle columns), never used
    wave_lds_sync();
    const uint8_t* qrow = q_all + qi * na;
    const uint8_t* rrow = r_all + ri * nb;
    const int n = compact_ranks(qmask_all ? qmask_all + qi * na : nullptr, na, [&](int rank, int k) { a[rank] = qrow[k]; });
    const int m = compact_ranks(rmask_all ? rmask_all + ri * nb : nullptr, nb, [&](int rank, int k) { b[rank] = rrow[k]; });
    wave_lds_sync();
    long long best = -(long long)(n + m);                                       // nothing aligned: every residue against a free gap
    if (n > 0 && m > 0) {
        const long long d_open = (long long)gap_open * SM_SCORE - 1, d_ext = (long long)gap_extend * SM_SCORE - 1;
        int braw[4], bidx[4];
        long long h[4], x[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            braw[c] = b[4 * lane + c];
            bidx[c] = min(braw[c], T - 1);
            h[c] = -(long long)(4 * lane + c + 1);                              // row 0: a free leading gap of j columns
            x[c] = SM_NEG;
        }
        long long diag_in = -(long long)(4 * lane);                             // H[i-1][4 l]
        long long out_h = SM_NEG, out_y = SM_NEG;                               // H and Y of the lane's last column, of the row it computed last
        const int lanes = (m + 3) >> 2;                                         // lanes that own a column <= m
        const int lane_m = (m - 1) >> 2, c_m = (m - 1) & 3;                     // who owns column m
        long long last_col = SM_NEG;
        for (int step = 1; step < n + lanes; ++step) {
            long long in_h = __shfl_up(out_h, 1, 64), in_y = __shfl_up(out_y, 1, 64);
            const int i = step - lane;
            if (lane == 0) { in_h = -(long long)i; in_y = SM_NEG; }             // column 0: a free leading gap of i columns
            if (i >= 1 && i <= n && lane < lanes) {
                const int araw = a[i - 1];
                const int16_t* row = tab + min(araw, T - 1) * T;
                long long left_h = in_h, left_y = in_y, diag = diag_in;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const long long pair = (long long)row[bidx[c]] * SM_SCORE + (araw == braw[c] ? 65536 : 0) - 1;
                    const long long xv = sm_max(h[c] + d_open, x[c] + d_ext);
                    const long long yv = sm_max(left_h + d_open, left_y + d_ext);
                    const long long hv = sm_max(diag + pair, sm_max(xv, yv));
                    diag = h[c];
                    h[c] = hv;
                    x[c] = xv;
                    left_h = hv;
                    left_y = yv;
                }
                diag_in = in_h;
                out_h = left_h;
                out_y = left_y;
                const long long hm = c_m == 0 ? h[0] : c_m == 1 ? h[1] : c_m == 2 ? h[2] : h[3];
                if (lane == lane_m) last_col = sm_max(last_col, hm - (long long)(n - i));      // a free trailing gap of n - i columns
            }
        }
        long long v = lane == lane_m ? last_col : SM_NEG;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = 4 * lane + c + 1;
            if (j <= m) v = sm_max(v, h[c] - (long long)(m - j));               // the last row: a free trailing gap of m - j columns
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = sm_max(v, __shfl_xor(v, off, 64));
        best = sm_max(best, v);
    }
    if (lane == 0) {
        const int cols = (int)((65536 - (best & 0xffff)) & 0xffff);
        const long long up = best + cols;
        score_all[p] = (int32_t)(up >> 32);
        matches_all[p] = (int32_t)((up >> 16) & 0xffff);
        columns_all[p] = cols;
    }
}

// ---------------------------------------------------------------- gapped RMSD
// The same grid.  s is the shorter list (M residues; the query when the lengths are equal) and l the longer (N); W = N - M + 1 placements of a residue.  With
// k = j - i the reference's table is a band, T_i[k] = SD[i][i + k] for k < W:
//   T_{M-1}[k] = d(M-1, M-1+k),   T_i[k] = min(d(i, i+k) + T_{i+1}[k], T_i[k+1]) with T_i[W] = +inf,   sd = min_k T_0[k]
// -- the boundary diagonal k = W - 1 by the same recurrence, min(x, +inf) = x.  Lane l owns k = 4 l .. 4 l + 3 and runs the rows from i = M - 1 down, one row
// behind lane l + 1, whose first column it needs.  A cell is one fp32 add and one min; nothing else is rounded after d.
__global__ __launch_bounds__(SM_WAVES * 64) void gapped_rmsd_kernel(const float* __restrict__ qca_all, const uint8_t* __restrict__ qmask_all,
                                                                     const float* __restrict__ rca_all, const uint8_t* __restrict__ rmask_all, int64_t pairs, int R,
                                                                     int na, int nb, float* __restrict__ sd_all, int32_t* __restrict__ m_all) {
    __shared__ float ca[SM_WAVES][2][3][SM_MAXLEN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p = folded_block() * SM_WAVES + wave;
    if (p >= pairs) return;                                                     // wave-uniform; this kernel has no barrier
    const int64_t qi = p / R, ri = p - qi * R;
    const float* qrow = qca_all + qi * na * 3;
    const float* rrow = rca_all + ri * nb * 3;
    float (*ca_q)[SM_MAXLEN] = ca[wave][0];
    float (*ca_r)[SM_MAXLEN] = ca[wave][1];
    const int nq = compact_ranks(qmask_all ? qmask_all + qi * na : nullptr, na, [&](int rank, int k) {
        ca_q[0][rank] = qrow[3 * k]; ca_q[1][rank] = qrow[3 * k + 1]; ca_q[2][rank] = qrow[3 * k + 2]; });
    const int nr = compact_ranks(rmask_all ? rmask_all + ri * nb : nullptr, nb, [&](int rank, int k) {
        ca_r[0][rank] = rrow[3 * k]; ca_r[1][rank] = rrow[3 * k + 1]; ca_r[2][rank] = rrow[3 * k + 2]; });
    wave_lds_sync();
    if (nq == 0 || nr == 0) {
        if (lane == 0) { sd_all[p] = -1.f; m_all[p] = 0; }
        return;
    }
    const bool q_short = nq <= nr;
    float (*s)[SM_MAXLEN] = q_short ? ca_q : ca_r;
    float (*l)[SM_MAXLEN] = q_short ? ca_r : ca_q;
    const int M = min(nq, nr), N = max(nq, nr), W = N - M + 1;
    const int lanes = (W + 3) >> 2;                                             // lanes that own a placement < W
    float t[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    float out_t = INFINITY;                                                     // the lane's first column, of the row it computed last
    for (int step = 0; step < M + lanes - 1; ++step) {
        const float in_t = __shfl_down(out_t, 1, 64);
        const int row = step - (lanes - 1 - lane);                              // rows counted from the last residue of s
        if (row >= 0 && row < M && lane < lanes) {
            const int i = M - 1 - row;
            const float sx = s[0][i], sy = s[1][i], sz = s[2][i];
            float right = lane == lanes - 1 ? INFINITY : in_t;
#pragma unroll
            for (int c = 3; c >= 0; --c) {
                const int k = 4 * lane + c;
                float v = INFINITY;
                if (k < W) {                                                    // i + k <= N - 1
                    const float d = d2_fma(sx, sy, sz, l[0][i + k], l[1][i + k], l[2][i + k]);
                    v = row == 0 ? d : fminf(d + t[c], right);
                }
                t[c] = v;
                right = v;
            }
            out_t = t[0];
        }
    }
    float v = fminf(fminf(t[0], t[1]), fminf(t[2], t[3]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    if (lane == 0) { sd_all[p] = v; m_all[p] = M; }
}

// Q query rows of na elements against R reference rows of nb: the checks both entry points make, in the order of candidate_common.h (dims, what is not
// supported, then -- after the caller's value checks -- the no-op and the pointers)
static int check_similarity_dims(const char* name, int Q, int R, int na, int nb) {
    ABOPT_CHECK_ARG(Q >= 0 && R >= 0 && na >= 1 && nb >= 1 && (int64_t)Q * R <= 0x7fffffff, "%s: bad dims Q=%d R=%d na=%d nb=%d", name, Q, R, na, nb);
    if (na > SM_MAXLEN || nb > SM_MAXLEN) {
        set_error("%s: na=%d, nb=%d elements per row exceed the maximum of %d", name, na, nb, SM_MAXLEN);
        return ABOPT_EUNSUPPORTED;
    }
    return ABOPT_OK;
}

}  // namespace abopt

using namespace abopt;

extern "C" int abopt_align_sequences(const uint8_t* q, const uint8_t* qmask, const uint8_t* r, const uint8_t* rmask, const int32_t* table, int T, int gap_open,
                                     int gap_extend, int Q, int R, int na, int nb, void* score, void* matches, void* columns, abopt_stream stream) {
    int rc = check_similarity_dims("align_sequences", Q, R, na, nb);
    if (rc != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(T >= 1 && T <= SM_MAXT, "align_sequences: T=%d rows of the table, expected 1 .. %d", T, SM_MAXT);
    ABOPT_CHECK_ARG(gap_open >= -32767 && gap_open <= gap_extend && gap_extend <= 0,
                    "align_sequences: expected -32767 <= gap_open <= gap_extend <= 0 (got gap_open=%d, gap_extend=%d)", gap_open, gap_extend);
    if (Q == 0 || R == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(q && r && table && score && matches && columns, "align_sequences: NULL argument");
    const int64_t pairs = (int64_t)Q * R;
    hipLaunchKernelGGL(align_sequences_kernel, fold_grid((pairs + SM_WAVES - 1) / SM_WAVES, 1u), dim3(SM_WAVES * 64), 0, (hipStream_t)stream, q, qmask, r, rmask,
                       table, T, gap_open, gap_extend, pairs, R, na, nb, (int32_t*)score, (int32_t*)matches, (int32_t*)columns);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}

extern "C" int abopt_gapped_rmsd(const float* qca, const uint8_t* qmask, const float* rca, const uint8_t* rmask, int Q, int R, int na, int nb, void* sd, void* m,
                                 abopt_stream stream) {
    int rc = check_similarity_dims("gapped_rmsd", Q, R, na, nb);
    if (rc != ABOPT_OK) return rc;
    if (Q == 0 || R == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(qca && rca && sd && m, "gapped_rmsd: NULL argument");
    const int64_t pairs = (int64_t)Q * R;
    hipLaunchKernelGGL(gapped_rmsd_kernel, fold_grid((pairs + SM_WAVES - 1) / SM_WAVES, 1u), dim3(SM_WAVES * 64), 0, (hipStream_t)stream, qca, qmask, rca, rmask,
                       pairs, R, na, nb, (float*)sd, (int32_t*)m);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}
