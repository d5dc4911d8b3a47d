// The alignment itself on the device: which residue of a query row is paired with which residue of a reference row, and the RMSD after
// superposition on those pairs.
//   abopt_align_traceback          the forward pass of abopt_align_sequences (similarity.hip: same carrier, same staging, same wavefront) that also keeps one
//                                  byte of tightness bits per cell in LDS, then a bounded backward walk over SETS of states: ops, qmap, rmap -- integers only;
//   abopt_superposed_rmsd_mapped   superpose_pair (superpose.h, unchanged) on the pairs a map names, one lane per pair.
// One launch each, nothing allocated, no workspace, nothing synchronised, no atomic, every output written whole by plain stores.  The definitions are in
// include/abopt.h; numpy restates them (tests/alignment_trace_statement.py), the integers exactly.
#include <math.h>
#include <algorithm>
#include "abopt_common.h"
#include "candidate_common.h"
#include "superpose.h"

namespace abopt {

constexpr int AT_MAXLEN = 256;             // elements of a row: four per lane of the pair's wave
constexpr int AT_WAVES = 4;                // pairs of a workgroup at most; the host takes fewer when their bits do not fit
constexpr int AT_MAXT = 32;                // rows of a substitution table at most
constexpr int AT_LDS = 160 * 1024;         // LDS of a CU: a workgroup may hold all of it
// similarity.hip's carrier: score 2^32 + matches 2^16 - columns in one int64, compared as signed numbers
constexpr long long AT_SCORE = 1ll << 32;
constexpr long long AT_NEG = -(1ll << 62);

// what a cell's byte records: which of the maxima of its three states are attained by which argument
constexpr unsigned AT_HD = 1, AT_HX = 2, AT_HY = 4;      // H = diagonal + pair;  H = X;  H = Y
constexpr unsigned AT_XO = 8, AT_XE = 16;                // X = H above + open;   X = X above + extend
constexpr unsigned AT_YO = 32, AT_YE = 64;               // Y = H left + open;    Y = Y left + extend
// the states of the walk
constexpr unsigned AT_SH = 1, AT_SX = 2, AT_SY = 4, AT_STA = 8, AT_STB = 16;

struct AtWave {                            // a wave's own LDS
    long long last_col[AT_MAXLEN + 1];     // H[i][m], i = 0 .. n
    uint8_t seq_a[AT_MAXLEN], seq_b[AT_MAXLEN];       // the compacted sequences
    uint8_t idx_a[AT_MAXLEN], idx_b[AT_MAXLEN];       // rank -> element index
    uint8_t last_row[AT_MAXLEN + 4];       // j = 0 .. m: H[n][j] - (m - j) is the optimum
    uint8_t ops[2 * AT_MAXLEN];
    int16_t qmap[AT_MAXLEN], rmap[AT_MAXLEN];
};
constexpr size_t AT_STATIC = AT_WAVES * sizeof(AtWave) + AT_MAXT * AT_MAXT * sizeof(int16_t);

__host__ __device__ inline int at_stride(int nb) { return (nb + 7) & ~7; }     // bytes between two rows of bits: lane l's dword of step s lies at dword
                                                                                // (s - 1) stride / 4 + l (1 - stride / 4), an odd multiple of l: 32 lanes, 32 banks

__device__ __forceinline__ long long at_max(long long a, long long b) { return a > b ? a : b; }

// Grid folded over x and y, `blockDim.x / 64` waves, a wave per pair.  The forward pass is align_sequences_kernel's, cell for cell; the bits of row i, columns
// 4 l + 1 .. 4 l + 4 are one dword store of lane l.  The walk is run by every lane alike on wave-uniform values (LDS reads of one address broadcast); lane 0 stores.
__global__ __launch_bounds__(AT_WAVES * 64) void align_traceback_kernel(const uint8_t* __restrict__ q_all, const uint8_t* __restrict__ qmask_all,
                                                                         const uint8_t* __restrict__ r_all, const uint8_t* __restrict__ rmask_all,
                                                                         const int32_t* __restrict__ table, int T, int gap_open, int gap_extend,
                                                                         const int32_t* __restrict__ pair_list, int64_t pairs, int Q, int R, int na, int nb,
                                                                         int32_t* __restrict__ score_all, int32_t* __restrict__ matches_all,
                                                                         int32_t* __restrict__ columns_all, uint8_t* __restrict__ ops_all,
                                                                         int16_t* __restrict__ qmap_all, int16_t* __restrict__ rmap_all) {
    extern __shared__ __attribute__((aligned(8))) uint8_t at_bits[];            // [wave][na][at_stride(nb)]
    __shared__ int16_t tab[AT_MAXT * AT_MAXT];
    __shared__ AtWave wave_lds[AT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    for (int k = tid; k < T * T; k += blockDim.x) tab[k] = (int16_t)min(max(table[k], -32767), 32767);
    __syncthreads();                                                            // the one barrier: before any wave leaves
    const int64_t p = folded_block() * waves + wave;
    if (p >= pairs) return;                                                     // wave-uniform
    int64_t qi, ri;
    if (pair_list) { qi = pair_list[2 * p]; ri = pair_list[2 * p + 1]; }
    else { qi = p / R; ri = p - qi * R; }
    AtWave& w = wave_lds[wave];
    const int stride = at_stride(nb);
    uint8_t* bits = at_bits + (size_t)wave * na * stride;
    for (int k = lane; k < AT_MAXLEN; k += 64) { w.seq_a[k] = 0; w.seq_b[k] = 0; w.qmap[k] = -1; w.rmap[k] = -1; }
    for (int k = lane; k < 2 * AT_MAXLEN; k += 64) w.ops[k] = 0;
    wave_lds_sync();
    int n = 0, m = 0;
    const bool inside = qi >= 0 && qi < Q && ri >= 0 && ri < R;                 // wave-uniform; a pair outside the panels reads nothing
    if (inside) {
        const uint8_t* qrow = q_all + qi * na;
        const uint8_t* rrow = r_all + ri * nb;
        n = compact_ranks(qmask_all ? qmask_all + qi * na : nullptr, na, [&](int rank, int k) { w.seq_a[rank] = qrow[k]; w.idx_a[rank] = (uint8_t)k; });
        m = compact_ranks(rmask_all ? rmask_all + ri * nb : nullptr, nb, [&](int rank, int k) { w.seq_b[rank] = rrow[k]; w.idx_b[rank] = (uint8_t)k; });
    }
    wave_lds_sync();
    long long best = -(long long)(n + m);                                       // nothing aligned: every residue against a free gap
    if (n > 0 && m > 0) {
        const uint8_t* a = w.seq_a;
        const uint8_t* b = w.seq_b;
        const long long d_open = (long long)gap_open * AT_SCORE - 1, d_ext = (long long)gap_extend * AT_SCORE - 1;
        int braw[4], bidx[4];
        long long h[4], x[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            braw[c] = b[4 * lane + c];
            bidx[c] = min(braw[c], T - 1);
            h[c] = -(long long)(4 * lane + c + 1);                              // row 0: a free leading gap of j columns
            x[c] = AT_NEG;
        }
        long long diag_in = -(long long)(4 * lane);                             // H[i-1][4 l]
        long long out_h = AT_NEG, out_y = AT_NEG;                               // H and Y of the lane's last column, of the row it computed last
        const int lanes = (m + 3) >> 2;                                         // lanes that own a column <= m
        const int lane_m = (m - 1) >> 2, c_m = (m - 1) & 3;                     // who owns column m
        long long last_col = AT_NEG;
        if (lane == 0) w.last_col[0] = -(long long)m;                           // H[0][m]
        for (int step = 1; step < n + lanes; ++step) {
            long long in_h = __shfl_up(out_h, 1, 64), in_y = __shfl_up(out_y, 1, 64);
            const int i = step - lane;
            if (lane == 0) { in_h = -(long long)i; in_y = AT_NEG; }             // column 0: a free leading gap of i columns
            if (i >= 1 && i <= n && lane < lanes) {
                const int araw = a[i - 1];
                const int16_t* row = tab + min(araw, T - 1) * T;
                long long left_h = in_h, left_y = in_y, diag = diag_in;
                unsigned cell = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const long long pair = (long long)row[bidx[c]] * AT_SCORE + (araw == braw[c] ? 65536 : 0) - 1;
                    const long long xo = h[c] + d_open, xe = x[c] + d_ext, yo = left_h + d_open, ye = left_y + d_ext, hd = diag + pair;
                    const long long xv = at_max(xo, xe);
                    const long long yv = at_max(yo, ye);
                    const long long hv = at_max(hd, at_max(xv, yv));
                    const unsigned t = (hd == hv ? AT_HD : 0u) | (xv == hv ? AT_HX : 0u) | (yv == hv ? AT_HY : 0u) | (xo == xv ? AT_XO : 0u) |
                                       (xe == xv ? AT_XE : 0u) | (yo == yv ? AT_YO : 0u) | (ye == yv ? AT_YE : 0u);
                    cell |= t << (8 * c);
                    diag = h[c];
                    h[c] = hv;
                    x[c] = xv;
                    left_h = hv;
                    left_y = yv;
                }
                *(unsigned*)(bits + (size_t)(i - 1) * stride + 4 * lane) = cell;  // 4 lane + 3 < 4 lanes <= stride, i - 1 < na
                diag_in = in_h;
                out_h = left_h;
                out_y = left_y;
                const long long hm = c_m == 0 ? h[0] : c_m == 1 ? h[1] : c_m == 2 ? h[2] : h[3];
                if (lane == lane_m) {
                    last_col = at_max(last_col, hm - (long long)(n - i));       // a free trailing gap of n - i columns
                    w.last_col[i] = hm;
                }
            }
        }
        long long v = lane == lane_m ? last_col : AT_NEG;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = 4 * lane + c + 1;
            if (j <= m) v = at_max(v, h[c] - (long long)(m - j));               // the last row: a free trailing gap of m - j columns
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = at_max(v, __shfl_xor(v, off, 64));
        best = at_max(best, v);
        // where a free trailing run may begin: behind (n, j) along the last row, behind (i, m) along the last column; the first such j < m and i < n
        int minb = m, mina = n;
        if (lane == 0) {
            const bool ok = -(long long)(n + m) == best;                        // H[n][0] = -n
            w.last_row[0] = ok;
            if (ok) minb = 0;
        }
#pragma unroll
        for (int c = 3; c >= 0; --c) {
            const int j = 4 * lane + c + 1;
            if (j <= m) {
                const bool ok = h[c] - (long long)(m - j) == best;
                w.last_row[j] = ok;
                if (ok && j < m) minb = min(minb, j);
            }
        }
        wave_lds_sync();
        for (int i = lane; i < n; i += 64)
            if (w.last_col[i] - (long long)(n - i) == best) mina = min(mina, i);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mina = min(mina, __shfl_xor(mina, off, 64));
            minb = min(minb, __shfl_xor(minb, off, 64));
        }
        // The walk, from the last column of the word to the first.  S: the states at (i, j) from which the letters already written complete an optimal word.
        const int cols = (int)((65536 - (best & 0xffff)) & 0xffff);            // <= n + m: the trip count depends on no tie
        int i = n, j = m;
        unsigned S = (w.last_col[n] == best ? AT_SH : 0u) | (mina < n ? AT_STA : 0u) | (minb < m ? AT_STB : 0u);
        for (int c = cols - 1; c >= 0; --c) {
            const unsigned t = (i >= 1 && j >= 1) ? bits[(size_t)(i - 1) * stride + (j - 1)] : 0u;
            if (S & AT_SH) S |= ((t & AT_HX) ? AT_SX : 0u) | ((t & AT_HY) ? AT_SY : 0u);      // the ties X = H, Y = H
            unsigned op = 0, oa = 0, ob = 0;                                    // the predecessors over a tight edge, by the letter it writes
            if (S & AT_SH) {
                if (i >= 1 && j >= 1) op |= (t & AT_HD) ? AT_SH : 0u;
                else if (i >= 1) oa |= AT_SH;                                   // column 0: the free leading run of A
                else ob |= AT_SH;                                               // row 0: the free leading run of B
            }
            if (S & AT_SX) oa |= ((t & AT_XO) ? AT_SH : 0u) | ((t & AT_XE) ? AT_SX : 0u);
            if (S & AT_SY) ob |= ((t & AT_YO) ? AT_SH : 0u) | ((t & AT_YE) ? AT_SY : 0u);
            if ((S & AT_STA) && i >= 1) oa |= (w.last_col[i - 1] - (long long)(n - i + 1) == best ? AT_SH : 0u) | (mina < i - 1 ? AT_STA : 0u);
            if ((S & AT_STB) && j >= 1) ob |= (w.last_row[j - 1] ? AT_SH : 0u) | (minb < j - 1 ? AT_STB : 0u);
            int letter;
            if (op) { letter = 1; S = op; }
            else if (oa) { letter = 2; S = oa; }
            else if (ob) { letter = 3; S = ob; }
            else { letter = i >= 1 ? 2 : 3; S = AT_SH; }                        // unreachable (every state has a tight predecessor); keeps i, j >= 0
            if (lane == 0) {
                w.ops[c] = (uint8_t)letter;
                if (letter == 1) {
                    const int ka = w.idx_a[i - 1], kb = w.idx_b[j - 1];
                    w.qmap[ka] = (int16_t)kb;
                    w.rmap[kb] = (int16_t)ka;
                }
            }
            if (letter != 3) i = max(i - 1, 0);
            if (letter != 2) j = max(j - 1, 0);
        }
    } else if (inside) {
        for (int k = lane; k < n + m; k += 64) w.ops[k] = n > 0 ? 2 : 3;        // an empty side: the other one against free gaps
    }
    wave_lds_sync();
    if (lane == 0) {
        const int cols = inside ? (int)((65536 - (best & 0xffff)) & 0xffff) : 0;
        const long long up = best + cols;
        score_all[p] = (int32_t)(up >> 32);
        matches_all[p] = (int32_t)((up >> 16) & 0xffff);
        columns_all[p] = cols;
    }
    if (ops_all) for (int k = lane; k < na + nb; k += 64) ops_all[p * (na + nb) + k] = w.ops[k];
    if (qmap_all) for (int k = lane; k < na; k += 64) qmap_all[p * na + k] = w.qmap[k];
    if (rmap_all) for (int k = lane; k < nb; k += 64) rmap_all[p * nb + k] = w.rmap[k];
}

// ---------------------------------------------------------------- mapped superposition
// The k-th pair of a map row that passes a mask on either side, found by a cursor that only moves forward: superpose_pair asks for k = 0, 1, 2 ... in order
// (each of its passes from 0 again), the mobile point first, then the target of the same k.  Straight from memory (L2): a lane's rows are its own.
struct MapCursor {
    const int16_t* map;
    const uint8_t* qm;
    const uint8_t* rm;
    int na, nb;
    __device__ __forceinline__ bool pair_at(int k) const {
        const int j = map[k];
        return j >= 0 && j < nb && (qm == nullptr || qm[k] != 0) && (rm == nullptr || rm[j] != 0);    // a j outside [0, nb) is never dereferenced
    }
    __device__ __forceinline__ int count() const {
        int c = 0;
        for (int k = 0; k < na; ++k) c += pair_at(k);
        return c;
    }
};
struct MappedMobile {
    const MapCursor& m;
    const float* x;
    int& cur;
    __device__ __forceinline__ void operator()(int k, double p[3]) const {
        cur = k == 0 ? 0 : cur + 1;
        while (cur < m.na - 1 && !m.pair_at(cur)) ++cur;                        // the caller counted the pairs: the k-th exists
        const float* a = x + 3 * cur;
        p[0] = (double)a[0]; p[1] = (double)a[1]; p[2] = (double)a[2];
    }
};
struct MappedTarget {
    const MapCursor& m;
    const float* y;
    const int& cur;
    __device__ __forceinline__ void operator()(int, double p[3]) const {
        const int j = min(max((int)m.map[cur], 0), m.nb - 1);
        const float* a = y + 3 * j;
        p[0] = (double)a[0]; p[1] = (double)a[1]; p[2] = (double)a[2];
    }
};

constexpr int MS_THREADS = 64;

__global__ __launch_bounds__(MS_THREADS) void superposed_rmsd_mapped_kernel(const float* __restrict__ q_all, const float* __restrict__ r_all,
                                                                             const int16_t* __restrict__ qmap_all, const int32_t* __restrict__ pair_list,
                                                                             const uint8_t* __restrict__ qfit, const uint8_t* __restrict__ qscore,
                                                                             const uint8_t* __restrict__ rfit, const uint8_t* __restrict__ rscore, int64_t pairs,
                                                                             int Q, int R, int na, int nb, float* __restrict__ rmsd_all,
                                                                             int32_t* __restrict__ nfit_all, int32_t* __restrict__ nscore_all,
                                                                             float* __restrict__ rot_all, float* __restrict__ trans_all) {
    const int64_t p = folded_block() * MS_THREADS + threadIdx.x;
    if (p >= pairs) return;                                                     // no barrier in this kernel
    int64_t qi, ri;
    if (pair_list) { qi = pair_list[2 * p]; ri = pair_list[2 * p + 1]; }
    else { qi = p / R; ri = p - qi * R; }
    double rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tr[3] = {0, 0, 0};
    float rmsd = -1.f;
    int nf = 0, ns = 0;
    if (qi >= 0 && qi < Q && ri >= 0 && ri < R) {
        const uint8_t* qs = qscore ? qscore : qfit;                             // a NULL score mask is that side's fit mask
        const uint8_t* rs = rscore ? rscore : rfit;
        const MapCursor fit{qmap_all + p * na, qfit ? qfit + qi * na : nullptr, rfit ? rfit + ri * nb : nullptr, na, nb};
        const MapCursor score{qmap_all + p * na, qs ? qs + qi * na : nullptr, rs ? rs + ri * nb : nullptr, na, nb};
        nf = fit.count();
        ns = score.count();
        if (nf >= 3 && ns >= 1) {
            const float* x = q_all + qi * na * 3;
            const float* y = r_all + ri * nb * 3;
            int cf = 0, cs = 0;
            const double ss = superpose_pair(nf, ns, MappedMobile{fit, x, cf}, MappedTarget{fit, y, cf}, MappedMobile{score, x, cs}, MappedTarget{score, y, cs}, rot, tr);
            rmsd = superposed_rmsd_of(ss, ns);
        } else {
            nf = ns = 0;
        }
    }
    rmsd_all[p] = rmsd;
    nfit_all[p] = nf;
    nscore_all[p] = ns;
    if (rot_all) {
#pragma unroll
        for (int k = 0; k < 9; ++k) rot_all[p * 9 + k] = (float)rot[k];
    }
    if (trans_all) {
#pragma unroll
        for (int k = 0; k < 3; ++k) trans_all[p * 3 + k] = (float)tr[k];
    }
}

static LdsConfig g_traceback_lds;

// Q query rows of na elements against R reference rows of nb, P listed pairs (or all Q R): dims, then what is not supported
static int check_trace_dims(const char* name, int Q, int R, int na, int nb, int P, bool listed) {
    ABOPT_CHECK_ARG(Q >= 0 && R >= 0 && na >= 1 && nb >= 1 && (int64_t)Q * R <= 0x7fffffff && (!listed || P >= 0), "%s: bad dims Q=%d R=%d na=%d nb=%d P=%d", name, Q,
                    R, na, nb, P);
    if (na > AT_MAXLEN || nb > AT_MAXLEN) {
        set_error("%s: na=%d, nb=%d elements per row exceed the maximum of %d", name, na, nb, AT_MAXLEN);
        return ABOPT_EUNSUPPORTED;
    }
    return ABOPT_OK;
}

}  // namespace abopt

using namespace abopt;

extern "C" int abopt_align_traceback(const uint8_t* q, const uint8_t* qmask, const uint8_t* r, const uint8_t* rmask, const int32_t* table, int T, int gap_open,
                                     int gap_extend, const int32_t* pairs, int P, int Q, int R, int na, int nb, void* score, void* matches, void* columns, void* ops,
                                     void* qmap, void* rmap, abopt_stream stream) {
    int rc = check_trace_dims("align_traceback", Q, R, na, nb, P, pairs != nullptr);
    if (rc != ABOPT_OK) return rc;
    ABOPT_CHECK_ARG(T >= 1 && T <= AT_MAXT, "align_traceback: T=%d rows of the table, expected 1 .. %d", T, AT_MAXT);
    ABOPT_CHECK_ARG(gap_open >= -32767 && gap_open <= gap_extend && gap_extend <= 0,
                    "align_traceback: expected -32767 <= gap_open <= gap_extend <= 0 (got gap_open=%d, gap_extend=%d)", gap_open, gap_extend);
    const int64_t count = pairs ? (int64_t)P : (int64_t)Q * R;
    if (count == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(table && score && matches && columns && (pairs || (q && r)), "align_traceback: NULL argument");
    ABOPT_CHECK_ARG(Q == 0 || R == 0 || (q && r), "align_traceback: NULL argument");
    const size_t per_wave = (size_t)na * at_stride(nb);                         // <= 64 KiB
    int waves = AT_WAVES;
    while (waves > 1 && AT_STATIC + waves * per_wave > (size_t)AT_LDS) waves >>= 1;
    const size_t lds = waves * per_wave;
    rc = ensure_dynamic_lds((const void*)align_traceback_kernel, lds, g_traceback_lds);
    if (rc != ABOPT_OK) return rc;
    hipLaunchKernelGGL(align_traceback_kernel, fold_grid((count + waves - 1) / waves, 1u), dim3(waves * 64), lds, (hipStream_t)stream, q, qmask, r, rmask, table, T,
                       gap_open, gap_extend, pairs, count, Q, R, na, nb, (int32_t*)score, (int32_t*)matches, (int32_t*)columns, (uint8_t*)ops, (int16_t*)qmap,
                       (int16_t*)rmap);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}

extern "C" int abopt_superposed_rmsd_mapped(const float* q, const float* r, void* qmap, const int32_t* pairs, int P, const uint8_t* qfit, const uint8_t* qscore,
                                            const uint8_t* rfit, const uint8_t* rscore, int Q, int R, int na, int nb, void* rmsd, void* n_fit, void* n_score,
                                            void* rot, void* trans, abopt_stream stream) {
    int rc = check_trace_dims("superposed_rmsd_mapped", Q, R, na, nb, P, pairs != nullptr);
    if (rc != ABOPT_OK) return rc;
    const int64_t count = pairs ? (int64_t)P : (int64_t)Q * R;
    if (count == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(qmap && rmsd && n_fit && n_score && (pairs || (q && r)), "superposed_rmsd_mapped: NULL argument");
    ABOPT_CHECK_ARG(Q == 0 || R == 0 || (q && r), "superposed_rmsd_mapped: NULL argument");
    hipLaunchKernelGGL(superposed_rmsd_mapped_kernel, fold_grid((count + MS_THREADS - 1) / MS_THREADS, 1u), dim3(MS_THREADS), 0, (hipStream_t)stream, q, r,
                       (const int16_t*)qmap, pairs, qfit, qscore, rfit, rscore, count, Q, R, na, nb, (float*)rmsd, (int32_t*)n_fit, (int32_t*)n_score, (float*)rot,
                       (float*)trans);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}
