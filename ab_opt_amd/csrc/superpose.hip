// RMSD after best-fit superposition on the device: every one of Q query rows against every one of R reference rows, fitted on one
// subset of the paired points and measured on another -- the loop designer's "is this the same loop shape", the framework-aligned CDR RMSD, the distance of a
// design to a panel of known loops.  One launch, nothing allocated, no workspace, nothing synchronised, no atomic, every output written whole by plain stores.
// The definition is in include/abopt.h (abopt_superposed_rmsd); numpy restates it in float64 (tests/superpose_statement.py).
//
// 256 threads own a 16 x 16 tile of pairs; one lane computes one pair from start to finish with superpose_pair (superpose.h), out of LDS:
//   coordinates  the 16 query rows and 16 reference rows of the tile as they lie in memory, row stride 3 n | 1 floats (dynamic LDS: 64 (3 n | 1) bytes a side)
//   rank lists   per row, the indices of its fit-true and of its score-true elements in order, one byte each (an index is < 256), row stride 260 bytes
// A wave holds 4 query rows x 16 reference rows.  The 32 lanes of a ds_read_b32 group read the same element rank of 16 different reference rows -- odd row
// strides (in dwords: 3 n | 1 and 65) put them on 16 different banks -- and of 2 query rows, a broadcast each.  With masks the coordinate read goes through the
// rank list and the banks are whatever the masks make them; without, they are conflict-free.
#include <math.h>
#include "abopt_common.h"
#include "candidate_common.h"
#include "superpose.h"

namespace abopt {

constexpr int SP_MAXLEN = 256;             // elements of a row: an index fits a byte
constexpr int SP_TILE = 16;                // rows of a side a workgroup holds
constexpr int SP_IDX = 260;                // bytes between two rank lists: 65 dwords
constexpr int SP_THREADS = SP_TILE * SP_TILE;

__host__ __device__ inline int sp_stride(int n) { return (3 * n) | 1; }

// the k-th listed point of a staged row, as double
struct RankedPoint {
    const float* row;
    const uint8_t* idx;
    __device__ __forceinline__ void operator()(int k, double p[3]) const {
        const float* a = row + 3 * (int)idx[k];
        p[0] = (double)a[0]; p[1] = (double)a[1]; p[2] = (double)a[2];
    }
};

__global__ __launch_bounds__(SP_THREADS) void superposed_rmsd_kernel(const float* __restrict__ q_all, const uint8_t* __restrict__ qfit, const uint8_t* __restrict__ qscore,
                                                                     const float* __restrict__ r_all, const uint8_t* __restrict__ rfit, const uint8_t* __restrict__ rscore,
                                                                     int Q, int R, int na, int nb, int64_t tiles, int tiles_r, float* __restrict__ rmsd_all,
                                                                     int32_t* __restrict__ nfit_all, int32_t* __restrict__ nscore_all, float* __restrict__ rot_all,
                                                                     float* __restrict__ trans_all) {
    extern __shared__ float sp_pts[];                                           // [16][3 na | 1] query rows, then [16][3 nb | 1] reference rows
    __shared__ __attribute__((aligned(4))) uint8_t idx_sh[2][2][SP_TILE][SP_IDX];   // [side: query, reference][list: fit, score][row][rank]
    __shared__ int len_sh[2][2][SP_TILE];
    const int64_t tile = folded_block();
    if (tile >= tiles) return;                                                  // block-uniform, ahead of the barrier
    const int tid = threadIdx.x, wave = tid >> 6;
    const int q0 = (int)(tile / tiles_r) * SP_TILE, r0 = (int)(tile % tiles_r) * SP_TILE;
    const int sq = sp_stride(na), sr = sp_stride(nb);
    float* pts_q = sp_pts;
    float* pts_r = sp_pts + SP_TILE * sq;
    {   // the tile's rows are one contiguous run of each panel
        const int nq = min(SP_TILE, Q - q0) * 3 * na, nr = min(SP_TILE, R - r0) * 3 * nb;
        const float* src_q = q_all + (int64_t)q0 * 3 * na;
        const float* src_r = r_all + (int64_t)r0 * 3 * nb;
        for (int i = tid; i < nq; i += SP_THREADS) pts_q[(i / (3 * na)) * sq + i % (3 * na)] = src_q[i];
        for (int i = tid; i < nr; i += SP_THREADS) pts_r[(i / (3 * nb)) * sr + i % (3 * nb)] = src_r[i];
    }
    // 2 sides x 2 lists x 16 rows = 64 rank lists, 16 per wave.  A score mask that is NULL is the row's fit mask; a row past the panel's end has no element.
    for (int job = wave; job < 4 * SP_TILE; job += SP_THREADS / 64) {
        const int side = job >> 5, list = (job >> 4) & 1, row = job & (SP_TILE - 1);
        const int g = (side ? r0 : q0) + row, n = side ? nb : na;
        const uint8_t* fit = side ? rfit : qfit;
        const uint8_t* score = side ? rscore : qscore;
        const uint8_t* mask = (list && score) ? score : fit;
        uint8_t* idx = idx_sh[side][list][row];
        int len = 0;
        if (g < (side ? R : Q)) len = compact_ranks(mask ? mask + (int64_t)g * n : nullptr, n, [&](int rank, int k) { idx[rank] = (uint8_t)k; });
        if ((tid & 63) == 0) len_sh[side][list][row] = len;
    }
    __syncthreads();
    const int qi = tid >> 4, ri = tid & (SP_TILE - 1);
    if (q0 + qi >= Q || r0 + ri >= R) return;
    const int nf = len_sh[0][0][qi], ns = len_sh[0][1][qi];
    const bool scored = nf == len_sh[1][0][ri] && ns == len_sh[1][1][ri] && nf >= 3 && ns >= 1;
    double rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tr[3] = {0, 0, 0};
    float rmsd = -1.f;
    if (scored) {
        const float* xq = pts_q + qi * sq;
        const float* yr = pts_r + ri * sr;
        const double ss = superpose_pair(nf, ns, RankedPoint{xq, idx_sh[0][0][qi]}, RankedPoint{yr, idx_sh[1][0][ri]}, RankedPoint{xq, idx_sh[0][1][qi]},
                                         RankedPoint{yr, idx_sh[1][1][ri]}, rot, tr);
        rmsd = superposed_rmsd_of(ss, ns);
    }
    const int64_t p = (int64_t)(q0 + qi) * R + r0 + ri;
    rmsd_all[p] = rmsd;
    nfit_all[p] = scored ? nf : 0;
    nscore_all[p] = scored ? ns : 0;
    if (rot_all) {
#pragma unroll
        for (int k = 0; k < 9; ++k) rot_all[p * 9 + k] = (float)rot[k];
    }
    if (trans_all) {
#pragma unroll
        for (int k = 0; k < 3; ++k) trans_all[p * 3 + k] = (float)tr[k];
    }
}

static LdsConfig g_superpose_lds;

}  // namespace abopt

using namespace abopt;

extern "C" int abopt_superposed_rmsd(const float* q, const uint8_t* qfit, const uint8_t* qscore, const float* r, const uint8_t* rfit, const uint8_t* rscore, int Q,
                                     int R, int na, int nb, void* rmsd, void* n_fit, void* n_score, void* rot, void* trans, abopt_stream stream) {
    ABOPT_CHECK_ARG(Q >= 0 && R >= 0 && na >= 1 && nb >= 1 && (int64_t)Q * R <= 0x7fffffff, "superposed_rmsd: bad dims Q=%d R=%d na=%d nb=%d", Q, R, na, nb);
    if (na > SP_MAXLEN || nb > SP_MAXLEN) {
        set_error("superposed_rmsd: na=%d, nb=%d elements per row exceed the maximum of %d", na, nb, SP_MAXLEN);
        return ABOPT_EUNSUPPORTED;
    }
    if (Q == 0 || R == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(q && r && rmsd && n_fit && n_score, "superposed_rmsd: NULL argument");
    const int tiles_r = (R + SP_TILE - 1) / SP_TILE;
    const int64_t tiles = (int64_t)((Q + SP_TILE - 1) / SP_TILE) * tiles_r;
    const size_t lds = (size_t)SP_TILE * (sp_stride(na) + sp_stride(nb)) * sizeof(float);
    int rc = ensure_dynamic_lds((const void*)superposed_rmsd_kernel, lds, g_superpose_lds);
    if (rc != ABOPT_OK) return rc;
    hipLaunchKernelGGL(superposed_rmsd_kernel, fold_grid(tiles, 1u), dim3(SP_THREADS), lds, (hipStream_t)stream, q, qfit, qscore, r, rfit, rscore, Q, R, na, nb,
                       tiles, tiles_r, (float*)rmsd, (int32_t*)n_fit, (int32_t*)n_score, (float*)rot, (float*)trans);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}
