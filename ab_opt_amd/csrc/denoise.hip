// Per-step diffusion transitions and sampler initialisation for CDNA4.
//
// Replaces (reference AbDock/src/, identical maths in AbDesign/diffab/):
//   PositionTransition.pred_noise_from_start / denoise      modules/diffusion/transition.py:42-50, 80-101
//   RotationTransition.denoise                              modules/diffusion/transition.py:146-160
//   ApproxAngularDistribution.sample, random_normal_so3     modules/common/so3.py:111-146
//   AminoacidCategoricalTransition.posterior/denoise/_sample modules/diffusion/transition.py:166-245
//   pRMSDCa.compute_prmsd, calc_perplexity                  modules/common/prmsd.py:31-47, modules/diffusion/dpm_full.py:380-399
//   FullDPM.sample initial state                            modules/diffusion/dpm_full.py:255-269
//   calc_per_rmsd / rank_commoness score                    tools/runner/design_for_testset.py:556-589
// The reference gathers an (N*L, 8192) histogram copy per step and calls multinomial on it (240 ms at
// N=4, L=256 on CPU); here one 8191-entry CDF row is binary-searched per residue.
#include "denoise_row.h"

namespace abopt {

__device__ __forceinline__ float torch_linspace(float a, float b, int steps, int i) {
    // at::linspace: symmetric evaluation around the midpoint
    const float step = (b - a) / (float)(steps - 1);
    return (i < steps / 2) ? a + step * (float)i : b - step * (float)(steps - 1 - i);
}

// one workgroup per sample n; threads stride over residues; block-reduce the two per-sample scalars.
__global__ __launch_bounds__(256) void denoise_step_kernel(abopt_step_params sp, abopt_step_noise nz, uint64_t seed, uint64_t offset,
                                                           const uint64_t* __restrict__ seed_dev,
                                                           const float* __restrict__ v_t, const float* __restrict__ p_t,
                                                           const int64_t* __restrict__ s_t, const float* __restrict__ v_net,
                                                           const float* __restrict__ p_net, const float* __restrict__ c_net,
                                                           const float* __restrict__ prmsd_logits, const uint8_t* __restrict__ mask_generate,
                                                           const float* __restrict__ igX, const float* __restrict__ igCdf, int bins, int num_bins,
                                                           float* __restrict__ v_next, float* __restrict__ p_next, int64_t* __restrict__ s_next,
                                                           float* __restrict__ prmsd, float* __restrict__ ppl, float* __restrict__ post_out,
                                                           float* __restrict__ p_next_norm, const int32_t* __restrict__ aa_allowed, int L, int ppl_masked) {
    const int n = blockIdx.x, tid = threadIdx.x;
    const bool injected = nz.axis != nullptr;
    if (seed_dev) { seed = seed_dev[0]; offset = seed_dev[1]; }     // graph replays: the stream position comes from device memory
    const Philox rng(seed);
    float ppl_num = 0.f, ppl_den = 0.f;
    // The histogram bin is the only long dependent chain of a residue (13 probes of the 8191-entry CDF row): the row is staged in LDS by
    // coalesced loads first (same comparisons on the same values), and not searched at all where its result cannot reach the output
    // (Gaussian branch of so3.py:129-138, the step that lands on 0: e = 0, injected noise).
    __shared__ float cdf_s[8192];
    const bool need_bin = !injected && !sp.igso3_gaussian && sp.t_prev > 0;
    const bool cdf_lds = need_bin && bins - 1 <= 8192;
    if (cdf_lds) {
        for (int k = tid; k < bins - 1; k += 256) cdf_s[k] = igCdf[k];
        __syncthreads();
    }

    const DenoiseRowIO io{v_t, p_t, s_t, v_net, p_net, c_net, mask_generate, aa_allowed, igX, igCdf, bins, v_next, p_next, s_next, post_out, p_next_norm};
    for (int l = tid; l < L; l += 256) {
        const int64_t i = (int64_t)n * L + l;
        float nx_, ny_, nz_;
        denoise_row(i, sp, nz, injected, rng, offset, io, cdf_lds ? cdf_s : nullptr, need_bin, ppl_masked, ppl_num, ppl_den, nx_, ny_, nz_);
    }

    // ---- per-sample scalars
    __shared__ float red[2][4];
    ppl_num = wave_sum(ppl_num); ppl_den = wave_sum(ppl_den);
    if ((tid & 63) == 0) { red[0][tid >> 6] = ppl_num; red[1][tid >> 6] = ppl_den; }
    __syncthreads();
    if (tid == 0) {
        if (ppl) ppl[n] = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / (red[1][0] + red[1][1] + red[1][2] + red[1][3]);
        if (prmsd && prmsd_logits) {
            float mx = -INFINITY;
            for (int b = 0; b < num_bins; ++b) mx = fmaxf(mx, prmsd_logits[(int64_t)n * num_bins + b]);
            float sm = 0.f;
            for (int b = 0; b < num_bins; ++b) sm += expf(prmsd_logits[(int64_t)n * num_bins + b] - mx);
            float acc = 0.f;
            for (int b = 0; b < num_bins; ++b)
                acc += (expf(prmsd_logits[(int64_t)n * num_bins + b] - mx) / sm) * torch_linspace(sp.dist_min, sp.dist_max, num_bins, b);
            prmsd[n] = acc;
        }
    }
}

// FullDPM.sample init (dpm_full.py:255-269)
__global__ __launch_bounds__(256) void sample_init_kernel(const float* __restrict__ v, const float* __restrict__ p, const int64_t* __restrict__ s,
                                                          const uint8_t* __restrict__ mask_generate, const float* __restrict__ q4,
                                                          const float* __restrict__ pn, const int64_t* __restrict__ sr, uint64_t seed, uint64_t offset,
                                                          float scale, float m0, float m1, float m2, int sample_structure, int sample_sequence,
                                                          float* __restrict__ v_init, float* __restrict__ p_init, int64_t* __restrict__ s_init,
                                                          const int32_t* __restrict__ aa_allowed, int64_t rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const bool gen = mask_generate[i] != 0;
    const uint32_t allow = aa_allowed_set(aa_allowed, i, gen);
    const float mean[3] = {m0, m1, m2};
    float q[4], g[3];
    int64_t srand_;
    if (q4) {
        q[0] = q4[i * 4]; q[1] = q4[i * 4 + 1]; q[2] = q4[i * 4 + 2]; q[3] = q4[i * 4 + 3];
        g[0] = pn[i * 3]; g[1] = pn[i * 3 + 1]; g[2] = pn[i * 3 + 2];
        srand_ = sr ? sr[i] : 0;
    } else {
        const Philox rng(seed);
        const uint4 r0 = rng(offset + (uint64_t)i, 0xFFFF00ull), r1 = rng(offset + (uint64_t)i, 0xFFFF01ull);
        float d0;
        box_muller(r0.x, r0.y, q[0], q[1]);
        box_muller(r0.z, r0.w, q[2], q[3]);
        box_muller(r1.x, r1.y, g[0], g[1]);
        box_muller(r1.z, r1.w, g[2], d0);
        const Philox rng2(seed ^ 0x5bd1e995ull);
        // randint_like(low=0, high=19): TYR never drawn.  Under a constraint: uniform over the allowed types among 0..18, the (r % count)-th set bit (r % 19 itself
        // when all are allowed); TYR only where nothing else is allowed
        const uint32_t r = rng2(offset + (uint64_t)i, 0xFFFF02ull).x;
        uint32_t low = allow & (AA_ALL >> 1);
        const uint32_t nth = low ? r % (uint32_t)__popc(low) : 0u;
        for (uint32_t c = 0; c < nth; ++c) low &= low - 1u;                       // drop the nth lowest allowed types: the next one is the draw
        srand_ = low ? (int64_t)(__ffs((int)low) - 1) : (int64_t)(KAA - 1);
        if (sr) srand_ = sr[i];      // sample_structure = False draws the sequence alone (dpm_full.py:262-267): it can be injected alone
    }
    // random_uniform_so3: F.normalize then quaternion_to_rotation_matrix (which normalises again), so3.py:66-68
    const float nq = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
    const Vec3 w = so3_log(quat_to_rot(q[0] / nq, q[1] / nq, q[2] / nq, q[3] / nq), false);
    const float wr[3] = {w.x, w.y, w.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float pnorm = (p[i * 3 + k] - mean[k]) / scale;
        const bool rnd = gen && sample_structure;
        v_init[i * 3 + k] = rnd ? wr[k] : v[i * 3 + k];
        p_init[i * 3 + k] = (rnd ? g[k] : pnorm) * scale + mean[k];
    }
    s_init[i] = (gen && sample_sequence && allow != 0u) ? srand_ : s[i];        // an empty set: the type is frozen
}

// Forward noising of all three modalities (transition.py:62-78,120-144,179-200); one thread per residue.
__global__ __launch_bounds__(256) void add_noise_kernel(const int64_t* __restrict__ t, const float* __restrict__ alpha_bars,
                                                        const float* __restrict__ fstd, const uint8_t* __restrict__ fapprox,
                                                        const float* __restrict__ fX, const float* __restrict__ fcdf, int bins,
                                                        abopt_addnoise_noise nz, uint64_t seed, uint64_t offset, const uint64_t* __restrict__ seed_dev,
                                                        const float* __restrict__ v_0, const float* __restrict__ p_0, const int64_t* __restrict__ s_0,
                                                        const uint8_t* __restrict__ mask_generate, float scale, float m0, float m1, float m2,
                                                        int noise_structure, int noise_sequence, int grad_mode,
                                                        float* __restrict__ v_noisy, float* __restrict__ p_noisy, int64_t* __restrict__ s_noisy,
                                                        float* __restrict__ eps_p, float* __restrict__ c_noisy, const int32_t* __restrict__ aa_allowed,
                                                        int L, int64_t rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const int64_t tt = t[i / L];
    const bool gen = mask_generate[i] != 0;
    const uint32_t allow = aa_allowed_set(aa_allowed, i, gen);
    const float abar = alpha_bars[tt];
    const float c0 = sqrtf(abar), c1 = sqrtf(1.f - abar);
    const float mean[3] = {m0, m1, m2};
    float ax = 0.f, ay = 0.f, az = 0.f, ubin = 0.f, gss = 0.f, ex = 0.f, ey = 0.f, ez = 0.f, useq = 0.f;
    int64_t bin = 0;
    // injected draws: all of them, or -- when the structure is not noised (dpm_full.py:169-173 draws nothing for it) -- s_noisy alone
    const bool injected = nz.axis != nullptr || (!noise_structure && nz.s_noisy != nullptr);
    if (nz.axis) {
        ax = nz.axis[i * 3]; ay = nz.axis[i * 3 + 1]; az = nz.axis[i * 3 + 2];
        bin = nz.bin[i]; ubin = nz.ubin[i]; gss = nz.gauss[i];
        ex = nz.pos[i * 3]; ey = nz.pos[i * 3 + 1]; ez = nz.pos[i * 3 + 2];
    } else if (!injected) {
        if (seed_dev) { seed = seed_dev[0]; offset = seed_dev[1]; }
        const Philox rng(seed);
        const uint4 r0 = rng(offset + (uint64_t)i, 0xA00000ull), r1 = rng(offset + (uint64_t)i, 0xA00001ull), r2 = rng(offset + (uint64_t)i, 0xA00002ull);
        float d0;
        box_muller(r0.x, r0.y, ax, ay);
        box_muller(r0.z, r0.w, az, gss);
        box_muller(r1.x, r1.y, ex, ey);
        box_muller(r1.z, r1.w, ez, d0);
        ubin = u01(r2.x); useq = u01(r2.y);
        const float ub = u01(r2.z);
        const float* cdf = fcdf + tt * (int64_t)(bins - 1);
        int lo = 0, hi = bins - 2;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (cdf[mid] > ub) hi = mid; else lo = mid + 1; }
        bin = lo;
    }
    // rotation
    const float vx = v_0[i * 3], vy = v_0[i * 3 + 1], vz = v_0[i * 3 + 2];
    float nvx = vx, nvy = vy, nvz = vz;
    if (noise_structure) {
        const float* X = fX + tt * (int64_t)bins;
        const float sd = fstd[tt];
        const float nrm = fmaxf(sqrtf(ax * ax + ay * ay + az * az), 1e-12f);
        const float hist = X[bin] + ubin * (X[bin + 1] - X[bin]);
        const float gau = fmodf(fabsf(sd * 2.f + gss * sd), PI_F);
        const float th = fapprox[tt] ? gau : hist;
        const Mat3 E = so3_exp(ax / nrm * th, ay / nrm * th, az / nrm * th);
        const Mat3 Rn = matmul3(E, so3_exp(c0 * vx, c0 * vy, c0 * vz));
        const Vec3 w = so3_log(Rn, grad_mode != 0);
        if (gen) { nvx = w.x; nvy = w.y; nvz = w.z; }
    }
    v_noisy[i * 3] = nvx; v_noisy[i * 3 + 1] = nvy; v_noisy[i * 3 + 2] = nvz;
    // position
    const float en[3] = {ex, ey, ez};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p0n = (p_0[i * 3 + k] - mean[k]) / scale;
        const float pn = (gen && noise_structure) ? c0 * p0n + c1 * en[k] : p0n;
        p_noisy[i * 3 + k] = pn * scale + mean[k];
        if (eps_p) eps_p[i * 3 + k] = noise_structure ? en[k] : 0.f;
    }
    // sequence
    const int64_t s0 = s_0[i];
    int64_t sn = s0;
    if (noise_sequence) {
        const bool ok = s0 >= 0 && s0 < KAA;
        float tot = 0.f, c[KAA];
#pragma unroll
        for (int k = 0; k < KAA; ++k) {
            const float oh = (ok && s0 == k) ? 1.f : 0.f;
            const float ck = gen ? (abar * oh) + ((1.f - abar) / (float)KAA) : oh;       // c_t, transition.py:196-198
            if (c_noisy) c_noisy[i * KAA + k] = ck;
            c[k] = ((allow >> k) & 1u) ? ck + 1e-8f : 0.f;                                 // _sample adds 1e-8 (transition.py:179); a disallowed class is skipped
            tot += c[k];                                                                   // (c_noisy above stays the reference's unconstrained c_t)
        }
        if (injected) sn = nz.s_noisy[i];
        else {
            const float target = useq * tot;
            float cum = 0.f;
            sn = aa_last_allowed(allow);
            for (int k = 0; k < KAA; ++k) { cum += c[k]; if (((allow >> k) & 1u) && cum > target) { sn = k; break; } }
        }
        if (allow == 0u) sn = s0;                                                          // an empty set: the type is frozen
    } else if (c_noisy) {
#pragma unroll
        for (int k = 0; k < KAA; ++k) c_noisy[i * KAA + k] = (s0 == k) ? 1.f : 0.f;      // c_0 = clampped_one_hot(s_0), transition.py:189
    }
    s_noisy[i] = sn;
}

// ---- IGSO(3) angle histograms for arbitrary standard deviations (include/abopt.h: abopt_igso3_tables): what ApproxAngularDistribution builds on the host at
// construction (so3.py:82-109; 8192 x 1024-element fp32 tensor ops per row), for the strides of a respaced loop, whose sigmas are chosen per call.
// One lane per bin, a wave per 64 consecutive bins; the l-dependent factor a_l of a row is staged in LDS once per workgroup.  Every lane walks l upwards on its own, in
// fp64: no cross-lane reduction, so the order of the sum is fixed, and the factors that do not depend on l (c and the denominator of b) multiply the finished sum.
constexpr int IG_CHUNK = 1024;
constexpr double PI_D = 3.14159265358979323846;

// at::linspace(0, pi, bins)[i] in fp32, bit for bit: fl(step i) below the midpoint and pi - step (bins - 1 - i) in one rounding from it on; step = fl(fl(pi) / (bins - 1))
__device__ __forceinline__ float linspace_0_pi(float step, int bins, int i) {
    return (i < bins / 2) ? step * (float)i : fmaf(-step, (float)(bins - 1 - i), PI_F);
}

__global__ __launch_bounds__(256) void igso3_hist_kernel(const float* __restrict__ stddevs, int bins, int iters, float step, float* __restrict__ X, float* __restrict__ Y) {
    const int r = blockIdx.y, tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * 256 + tid;
    const bool live = b < bins;
    __shared__ double a_s[IG_CHUNK];
    const double sd = (double)stddevs[r], var = sd * sd;
    const float xf = linspace_0_pi(step, bins, live ? (int)b : 0);
    const double x = (double)xf;
    double acc = 0.0;
    for (int l0 = 0; l0 < iters; l0 += IG_CHUNK) {
        const int n = min(IG_CHUNK, iters - l0);
        __syncthreads();
        for (int k = tid; k < n; k += 256) {
            const double l = (double)(l0 + k);
            a_s[k] = (2.0 * l + 1.0) * exp(-l * (l + 1.0) * var);
        }
        __syncthreads();
        if (live)
            for (int k = 0; k < n; ++k) acc += a_s[k] * (sin(((double)(l0 + k) + 0.5) * x) + 1e-6);
    }
    if (!live) return;
    const double c = (1.0 - cos(x)) / PI_D, den = sin(x / 2.0) + 1e-6;
    float y = (float)(c * acc / den);
    if (y != y) y = 0.f;                                        // nan_to_num, clamp_min(0)
    y = fminf(fmaxf(y, 0.f), 3.402823466e+38f);
    const int64_t o = (int64_t)r * bins + b;
    Y[o] = y;
    if (X) X[o] = xf;
}

// cdf[r, :] = cumsum(Y[r, :bins-1]) / sum(Y[r, :bins-1]) in fp64 (ApproxAngularDistribution.cdf); one workgroup per row, a contiguous run of cells per thread
__global__ __launch_bounds__(256) void igso3_cdf_kernel(const float* __restrict__ Y, int bins, float* __restrict__ cdf) {
    const int tid = threadIdx.x;
    const int64_t n = (int64_t)bins - 1, per = (n + 255) / 256;
    const int64_t lo = min((int64_t)tid * per, n), hi = min(lo + per, n);
    const float* y = Y + (int64_t)blockIdx.x * bins;
    float* c = cdf + (int64_t)blockIdx.x * n;
    __shared__ double part[256];
    __shared__ double total;
    double s = 0.0;
    for (int64_t k = lo; k < hi; ++k) s += (double)y[k];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        double run = 0.0;
        for (int i = 0; i < 256; ++i) { const double v = part[i]; part[i] = run; run += v; }
        total = run;
    }
    __syncthreads();
    const double tot = total > 0.0 ? total : 1.0;
    double run = part[tid];
    for (int64_t k = lo; k < hi; ++k) { run += (double)y[k]; c[k] = (float)(run / tot); }
}

// score[b] = sum_b' sqrt(mean_n |x_b - x_b'|^2) / (B - 1)   (design_for_testset.py:556-563,586-588)
__global__ __launch_bounds__(256) void commonness_kernel(const float* __restrict__ x, float* __restrict__ score, int B, int n) {
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ float part[4];
    float tot = 0.f;
    for (int o = wave; o < B; o += 4) {
        float s = 0.f;
        for (int k = lane; k < n * 3; k += 64) { const float d = x[((int64_t)b * n) * 3 + k] - x[((int64_t)o * n) * 3 + k]; s = fmaf(d, d, s); }
        s = wave_sum(s);
        tot += sqrtf(s / (float)n);
    }
    if (lane == 0) part[wave] = tot;
    __syncthreads();
    if (tid == 0) score[b] = (part[0] + part[1] + part[2] + part[3]) / (float)(B - 1);
}

// G groups of S in one launch: workgroup c scores structure c within its group; commonness_kernel's arithmetic on the group's base pointer
// (bit-identical to a launch of commonness_kernel per group)
__global__ __launch_bounds__(256) void commonness_grouped_kernel(const float* __restrict__ x_all, float* __restrict__ score_all, int S, int n) {
    const int g = blockIdx.x / S, b = blockIdx.x % S, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* x = x_all + (int64_t)g * S * n * 3;
    __shared__ float part[4];
    float tot = 0.f;
    for (int o = wave; o < S; o += 4) {
        float s = 0.f;
        for (int k = lane; k < n * 3; k += 64) { const float d = x[((int64_t)b * n) * 3 + k] - x[((int64_t)o * n) * 3 + k]; s = fmaf(d, d, s); }
        s = wave_sum(s);
        tot += sqrtf(s / (float)n);
    }
    if (lane == 0) part[wave] = tot;
    __syncthreads();
    if (tid == 0) score_all[blockIdx.x] = (part[0] + part[1] + part[2] + part[3]) / (float)(S - 1);
}

}  // namespace abopt

using namespace abopt;

// The step's checks, shared with abopt_eps_net_step (api.hip): nz = the injected draws, or all NULL for the device stream
int abopt::check_step_args(const abopt_step_params* sp, const abopt_step_noise* noise, const float* igso3_X, const float* igso3_cdf, int igso3_bins, abopt_step_noise* nz) {
    ABOPT_CHECK_ARG(sp, "denoise_step: NULL argument");
    ABOPT_CHECK_ARG(igso3_X && igso3_bins >= 2, "denoise_step: IGSO(3) histogram row missing");
    ABOPT_CHECK_ARG(sp->t_prev >= 0 && sp->t_prev < sp->t, "denoise_step: the step must land below where it starts (t=%d t_prev=%d)", sp->t, sp->t_prev);
    if (sp->tempered) {         // (the comparisons refuse a NaN too)
        ABOPT_CHECK_ARG(sp->seq_temperature >= 0.f && sp->seq_temperature < INFINITY && (sp->seq_temperature == 0.f || sp->seq_temperature >= 1e-3f),
                        "denoise_step: seq_temperature must be 0 or a finite value >= 1e-3 (got %g)", (double)sp->seq_temperature);
        ABOPT_CHECK_ARG(sp->noise_scale >= 0.f && sp->noise_scale < INFINITY, "denoise_step: noise_scale must be finite and >= 0 (got %g)", (double)sp->noise_scale);
    }
    *nz = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (noise && noise->axis) {
        ABOPT_CHECK_ARG(noise->bin && noise->ubin && noise->gauss && noise->z && noise->s_next, "denoise_step: injected noise must provide all six draws");
        *nz = *noise;
    } else {
        ABOPT_CHECK_ARG(igso3_cdf, "denoise_step: device RNG path needs the CDF row");
    }
    return ABOPT_OK;
}

extern "C" int abopt_denoise_step(const abopt_step_params* sp, const abopt_step_noise* noise, uint64_t seed, uint64_t offset,
                                  const float* v_t, const float* p_t, const int64_t* s_t,
                                  const float* v_net, const float* p_net, const float* c_net, const float* prmsd_logits,
                                  const uint8_t* mask_generate, const float* igso3_X, const float* igso3_cdf, int igso3_bins, int num_bins,
                                  float* v_next, float* p_next, int64_t* s_next, float* prmsd, float* perplexity,
                                  float* post_out, float* p_next_norm, const uint64_t* seed_offset_dev, const int32_t* aa_allowed,
                                  int N, int L, abopt_stream stream) {
    ABOPT_CHECK_ARG(sp && v_t && p_t && s_t && v_net && p_net && c_net && mask_generate && v_next && p_next && s_next, "denoise_step: NULL argument");
    abopt_step_noise nz;
    if (int rc = check_step_args(sp, noise, igso3_X, igso3_cdf, igso3_bins, &nz)) return rc;
    if (N == 0 || L == 0) return ABOPT_OK;
    hipLaunchKernelGGL(denoise_step_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, *sp, nz, seed, offset, seed_offset_dev, v_t, p_t, s_t, v_net, p_net, c_net,
                       prmsd_logits, mask_generate, igso3_X, igso3_cdf, igso3_bins, num_bins, v_next, p_next, s_next, prmsd, perplexity, post_out,
                       p_next_norm, aa_allowed, L, sp->ppl_masked);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}

extern "C" int abopt_igso3_tables(const float* stddevs, int rows, int bins, int iters, float* X, float* Y, float* cdf, abopt_stream stream) {
    ABOPT_CHECK_ARG(stddevs && Y && cdf, "igso3_tables: NULL argument");
    ABOPT_CHECK_ARG(rows >= 0 && rows <= 65535 && bins >= 2 && iters >= 1, "igso3_tables: bad sizes (rows=%d bins=%d iters=%d)", rows, bins, iters);
    if (rows == 0) return ABOPT_OK;
    const float step = PI_F / (float)(bins - 1);
    hipLaunchKernelGGL(igso3_hist_kernel, dim3((unsigned)((bins + 255) / 256), (unsigned)rows), dim3(256), 0, (hipStream_t)stream, stddevs, bins, iters, step, X, Y);
    ABOPT_LAUNCH_CHECK();
    hipLaunchKernelGGL(igso3_cdf_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, Y, bins, cdf);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}

extern "C" int abopt_sample_init(const float* v, const float* p, const int64_t* s, const uint8_t* mask_generate,
                                 const float* q4, const float* pn, const int64_t* sr, uint64_t seed, uint64_t offset,
                                 float position_scale, const float* position_mean, int sample_structure, int sample_sequence,
                                 float* v_init, float* p_init, int64_t* s_init, const int32_t* aa_allowed, int N, int L, abopt_stream stream) {
    ABOPT_CHECK_ARG(v && p && s && mask_generate && v_init && p_init && s_init && position_mean, "sample_init: NULL argument");
    ABOPT_CHECK_ARG((q4 == nullptr) == (pn == nullptr), "sample_init: q4 and pn must be given together");
    const int64_t rows = (int64_t)N * L;
    if (rows == 0) return ABOPT_OK;
    hipLaunchKernelGGL(sample_init_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v, p, s, mask_generate, q4, pn, sr,
                       seed, offset, position_scale, position_mean[0], position_mean[1], position_mean[2], sample_structure, sample_sequence,
                       v_init, p_init, s_init, aa_allowed, rows);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}

extern "C" int abopt_add_noise(const int64_t* t, const float* alpha_bars, const float* fwd_stddevs, const uint8_t* fwd_approx,
                               const float* fwd_X, const float* fwd_cdf, int bins, int num_sched,
                               const abopt_addnoise_noise* noise, uint64_t seed, uint64_t offset,
                               const float* v_0, const float* p_0, const int64_t* s_0, const uint8_t* mask_generate,
                               float position_scale, const float* position_mean, int noise_structure, int noise_sequence, int grad_mode,
                               float* v_noisy, float* p_noisy, int64_t* s_noisy, float* eps_p, float* c_noisy, const uint64_t* seed_offset_dev,
                               const int32_t* aa_allowed, int N, int L, abopt_stream stream) {
    ABOPT_CHECK_ARG(t && alpha_bars && fwd_stddevs && fwd_approx && fwd_X && v_0 && p_0 && s_0 && mask_generate && position_mean &&
                    v_noisy && p_noisy && s_noisy && bins >= 2 && num_sched >= 1, "add_noise: bad arguments");
    abopt_addnoise_noise nz = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (noise && noise->axis) {
        ABOPT_CHECK_ARG(noise->bin && noise->ubin && noise->gauss && noise->pos && (noise->s_noisy || !noise_sequence), "add_noise: injected noise must provide every draw");
        nz = *noise;
    } else if (noise && noise->s_noisy && !noise_structure) {
        nz.s_noisy = noise->s_noisy;          // sequence-only noising (train_structure = False): the one draw this mode makes
    } else {
        ABOPT_CHECK_ARG(fwd_cdf, "add_noise: device RNG path needs the CDF table");
    }
    const int64_t rows = (int64_t)N * L;
    if (rows == 0) return ABOPT_OK;
    hipLaunchKernelGGL(add_noise_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, alpha_bars, fwd_stddevs, fwd_approx,
                       fwd_X, fwd_cdf, bins, nz, seed, offset, seed_offset_dev, v_0, p_0, s_0, mask_generate, position_scale, position_mean[0], position_mean[1],
                       position_mean[2], noise_structure, noise_sequence, grad_mode, v_noisy, p_noisy, s_noisy, eps_p, c_noisy, aa_allowed, L, rows);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}

extern "C" int abopt_commonness_score(const float* structs, float* score, int B, int n, abopt_stream stream) {
    ABOPT_CHECK_ARG(structs && score && B >= 2 && n >= 1, "commonness_score: bad arguments (B=%d n=%d)", B, n);
    hipLaunchKernelGGL(commonness_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, structs, score, B, n);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}

extern "C" int abopt_commonness_score_grouped(const float* structs, float* score, int G, int S, int n, abopt_stream stream) {
    ABOPT_CHECK_ARG(structs && score && G >= 0 && S >= 2 && n >= 1 && (int64_t)G * S <= 0x7fffffff,
                    "commonness_score_grouped: bad arguments (G=%d S=%d n=%d)", G, S, n);
    if (G == 0) return ABOPT_OK;
    hipLaunchKernelGGL(commonness_grouped_kernel, dim3((unsigned)(G * S)), dim3(256), 0, (hipStream_t)stream, structs, score, S, n);
    ABOPT_LAUNCH_CHECK();
    return ABOPT_OK;
}
