// One residue of a denoising step (the loop body of FullDPM.sample after the network, dpm_full.py:284-297): the three transitions
//   RotationTransition.denoise (transition.py:146-160, so3.py:111-146), PositionTransition.denoise / pred_noise_from_start (transition.py:42-50,80-101),
//   AminoacidCategoricalTransition.denoise (transition.py:202-245), and the residue's perplexity term (dpm_full.py:392-396)
// as device functions shared by denoise_step_kernel (denoise.hip: one workgroup per sample, the pieces back to back in denoise_row) and by the fused tail of a step
// (heads.hip: step_tail_kernel runs the pieces on different waves of the heads' workgroup) -- the same arithmetic in the same order, bit for bit.
//
// Allowed residue types (include/abopt.h: aa_allowed): one int32 word per residue, bit k = type k may be drawn, read on generated residues only.  A disallowed
// class leaves the categorical BEFORE it is normalised (its unnormalised product becomes 0), so post_out, the draw and the perplexity term all see the distribution
// that is sampled; with every bit set each operation below is the unconstrained one on the same values in the same order.
//
// Sampling at a temperature (include/abopt.h: abopt_step_params.tempered): behind the wave-uniform sp.tempered the rotation noise angle and the
// position noise's sigma are multiplied by sp.noise_scale and the row's prediction is tempered before the posterior is formed; with the flag clear every function below
// is the code of the earlier ABIs.
#pragma once
#include "abopt_common.h"
#include "kernels.h"

namespace abopt {

constexpr int KAA = ABOPT_AA;
constexpr float PI_F = 3.14159265358979323846f;
constexpr uint32_t AA_ALL = (1u << KAA) - 1u;

// The set a residue's type is drawn from: every type where there is no constraint or the residue is not generated; bits KAA.. of the word are ignored.
// 0 (an empty word on a generated residue) freezes the residue's type.
__device__ __forceinline__ uint32_t aa_allowed_set(const int32_t* aa_allowed, int64_t i, bool gen) {
    return (aa_allowed && gen) ? ((uint32_t)aa_allowed[i] & AA_ALL) : AA_ALL;
}
// highest allowed class: where an inverse-CDF walk ends when rounding leaves it short of its target (KAA - 1 without a constraint)
__device__ __forceinline__ int aa_last_allowed(uint32_t allow) { return 31 - __clz((int)allow); }

struct DenoiseRowIO {
    const float* v_t; const float* p_t; const int64_t* s_t; const float* v_net; const float* p_net; const float* c_net; const uint8_t* mask_generate; const int32_t* aa_allowed;
    const float* igX; const float* igCdf; int bins;
    float* v_next; float* p_next; int64_t* s_next; float* post_out; float* p_next_norm;
};

// The row's chain in pieces, cut where a value is complete (a raw draw, a select, the result of an addition or a division: nothing hipcc could contract across the
// cut): denoise_row below calls them back to back, the fused tail of a step (heads.hip: step_tail_kernel) runs them on different waves with LDS in between.
// a product rounded to fp32 HERE, whatever follows it (the compiler may not contract it into an fma)
__device__ __forceinline__ float rounded_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
struct RowDraws { float ax, ay, az, ubin, gss, zx, zy, zz, useq; int64_t bin; };

// ---- draws.  cdf_s: the CDF row staged in LDS (or nullptr: searched in global memory, when need_bin)
__device__ __forceinline__ RowDraws denoise_draws(int64_t i, const abopt_step_params& sp, const abopt_step_noise& nz, bool injected, const Philox& rng, uint64_t offset,
                                                  const float* igCdf, int bins, const float* cdf_s, bool need_bin) {
    RowDraws d;
    d.bin = 0;
    if (injected) {
        d.ax = nz.axis[i * 3]; d.ay = nz.axis[i * 3 + 1]; d.az = nz.axis[i * 3 + 2];
        d.bin = nz.bin[i]; d.ubin = nz.ubin[i]; d.gss = nz.gauss[i];
        d.zx = nz.z[i * 3]; d.zy = nz.z[i * 3 + 1]; d.zz = nz.z[i * 3 + 2];
        d.useq = 0.f;
    } else {
        const uint64_t ctr = offset + (uint64_t)i;
        const uint4 r0 = rng(ctr, ((uint64_t)sp.t << 8) | 0u), r1 = rng(ctr, ((uint64_t)sp.t << 8) | 1u), r2 = rng(ctr, ((uint64_t)sp.t << 8) | 2u);
        float d0;
        box_muller(r0.x, r0.y, d.ax, d.ay);
        box_muller(r0.z, r0.w, d.az, d.gss);
        box_muller(r1.x, r1.y, d.zx, d.zy);
        box_muller(r1.z, r1.w, d.zz, d0);
        d.ubin = u01(r2.x); d.useq = u01(r2.y);
        const float ub = u01(r2.z);
        // inverse CDF over bins-1 histogram cells == multinomial(Y[t, :-1]) (so3.py:122)
        int lo = 0, hi = bins - 2;
        if (cdf_s) { while (lo < hi) { const int mid = (lo + hi) >> 1; if (cdf_s[mid] > ub) hi = mid; else lo = mid + 1; } }
        else if (need_bin) { while (lo < hi) { const int mid = (lo + hi) >> 1; if (igCdf[mid] > ub) hi = mid; else lo = mid + 1; } }
        d.bin = lo;
    }
    return d;
}

// ---- rotation noise (transition.py:146-160, so3.py:111-146): the normalised axis times its IGSO(3) angle; 0 on the step that lands on 0
__device__ __forceinline__ void denoise_rot_noise(const RowDraws& d, const abopt_step_params& sp, const float* igX, float& ex, float& ey, float& ez) {
    const float ax = d.ax, ay = d.ay, az = d.az;
    const float nrm = fmaxf(sqrtf(ax * ax + ay * ay + az * az), 1e-12f);
    const float hist = igX[d.bin] + d.ubin * (igX[d.bin + 1] - igX[d.bin]);
    const float gau = fmodf(fabsf(fmaf(d.gss, sp.igso3_std, sp.igso3_std * 2.f)), PI_F);      // std 2 + gss std: the doubling is exact, the one rounding is the fma's
    float th = sp.igso3_gaussian ? gau : hist;
    if (sp.tempered) th = rounded_mul(th, sp.noise_scale);       // the angle at the noise scale lambda (include/abopt.h: noise_scale); x 1 is exact
    ex = ax / nrm * th; ey = ay / nrm * th; ez = az / nrm * th;
    if (!(sp.t_prev > 0)) { ex = 0.f; ey = 0.f; ez = 0.f; }       // no noise on the step that lands on 0 (the reference's t > 1: t_prev = t - 1 there)
}

// ---- rotation: log(exp(e) exp(v_net)) on generated residues.  vt / vn: the row's three values of v_t / v_net
__device__ __forceinline__ void denoise_rotation(float ex, float ey, float ez, const float* vt, const float* vn, bool gen, float& nvx, float& nvy, float& nvz) {
    nvx = vt[0]; nvy = vt[1]; nvz = vt[2];
    const Mat3 E = so3_exp(ex, ey, ez);
    const Mat3 Rn = matmul3(E, so3_exp(vn[0], vn[1], vn[2]));
    const Vec3 w = so3_log(Rn, false);
    if (gen) { nvx = w.x; nvy = w.y; nvz = w.z; }
}

// ---- position (transition.py:42-50, 80-101); state is kept in Angstrom like the reference traj.  pa / pnet / zn: the row's three values of p_t / p_net / the noise
__device__ __forceinline__ void denoise_position(const abopt_step_params& sp, const float* pa, const float* pnet_row, const float* zn, bool gen, float* pn, float* pt) {
    const float c0 = 1.0f / sqrtf(sp.alpha_clamped + 1e-8f);
    const float c1 = (1.f - sp.alpha_clamped) / sqrtf(1.f - sp.alpha_bar + 1e-8f);
    const float sigma = sp.tempered ? rounded_mul(sp.sigma, sp.noise_scale) : sp.sigma;       // sigma_eff = sigma lambda, rounded once (include/abopt.h: noise_scale)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pt[k] = (pa[k] - sp.position_mean[k]) / sp.position_scale;
        const float pnet = pnet_row[k];
        float eps = pnet;
        if (sp.pred_x0) eps = gen ? (sp.sqrt_recip_abar * pt[k] - pnet) / sp.sqrt_recipm1_abar : pt[k];
        const float zk = (sp.t_prev > 0) ? zn[k] : 0.f;
        // c0 (pt - c1 eps) + sigma z with the product that is rounded and the one that is fused spelled out: left to the compiler, the choice between the two
        // contractions follows the operand order its passes leave, which differs between the kernels this function is inlined into
        const float nx = fmaf(sigma, zk, rounded_mul(c0, pt[k] - c1 * eps));
        pn[k] = gen ? nx : pt[k];
    }
}

// the row's next position in Angstrom and, normalised again, as the next step feeds the network (dpm_full.py:276 normalises the STORED Angstrom value): saves the host two launches per step
__device__ __forceinline__ void denoise_store_position(int64_t i, const abopt_step_params& sp, const float* pn, float* p_next, float* p_next_norm) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float pa_next = pn[k] * sp.position_scale + sp.position_mean[k];
        p_next[i * 3 + k] = pa_next;
        if (p_next_norm) p_next_norm[i * 3 + k] = (pa_next - sp.position_mean[k]) / sp.position_scale;
    }
}

// ---- the row's prediction at the temperature tau = sp.seq_temperature (include/abopt.h: seq_temperature) into cp[0..19]: cn itself where the row does not draw, tau is 1
// or there is nothing to sharpen.  Every product is rounded where it stands and every c'_k is the result of a division: nothing contracts into what follows.
__device__ __forceinline__ void denoise_temper(const abopt_step_params& sp, const float* cn, uint32_t allow, bool draws, float* cp) {
    const float tau = sp.seq_temperature;
    float m = 0.f;                                  // max over the allowed classes of max(c_k, 0): fmaxf drops a NaN
#pragma unroll
    for (int k = 0; k < KAA; ++k) m = ((allow >> k) & 1u) ? fmaxf(m, cn[k]) : m;
    const bool temper = draws && tau != 1.f && m > 0.f && m < INFINITY;
    const bool greedy = tau == 0.f;
    const float lm = log2f(m), rtau = 1.f / tau;
    float esum = 0.f;
    bool found = false;
#pragma unroll
    for (int k = 0; k < KAA; ++k) {
        const bool ok = ((allow >> k) & 1u) != 0u;
        const float ck = fmaxf(cn[k], 0.f);
        const bool first = ok && !found && ck == m;                                             // tau = 0: all mass on the lowest-index maximum
        found = found || first;
        const float e = greedy ? (first ? 1.f : 0.f) : (ok ? exp2f(rounded_mul(log2f(ck) - lm, rtau)) : 0.f);
        cp[k] = e;
        esum += e;
    }
#pragma unroll
    for (int k = 0; k < KAA; ++k) cp[k] = temper ? cp[k] / esum : cn[k];
}

// the unnormalised posterior of a row from its prediction c (cn, or the tempered one: c may be post itself), disallowed classes zeroed; returns the sum
__device__ __forceinline__ float denoise_posterior_raw(float ab, float unif, bool st_ok, int64_t st, const float* c, uint32_t allow, float* post) {
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < KAA; ++k) {
        const float ct = (st_ok && st == k) ? 1.f : 0.f;
        const float raw = ((ab * ct) + unif) * ((ab * c[k]) + unif);
        const bool ok = ((allow >> k) & 1u) != 0u;
        tot = ok ? tot + raw : tot;                 // `tot + raw` as the unconstrained code spells it: the compiler contracts it to the same fma
        post[k] = ok ? raw : 0.f;
    }
    return tot;
}

// ---- sequence (transition.py:202-245): NOTE alpha_bar_t multiplies both factors (reference quirk).  cn: the row's 20 values of c_net.  Leaves the posterior in post
// (and post_out) and its maximum in pmax; returns what s_next takes
__device__ __forceinline__ int64_t denoise_sequence(int64_t i, const abopt_step_params& sp, const abopt_step_noise& nz, bool injected, float useq, int64_t st, const float* cn,
                                                    uint32_t allow, bool gen, float* post_out, float* post, float& pmax) {
    const bool st_ok = st >= 0 && st < KAA;
    const bool draws = gen && allow != 0u;          // an empty set: the type is frozen, its posterior is onehot(s_t) like a context residue's (the structure above still moved)
    float tot;
    const float ab = sp.alpha_bar, unif = (1.f - ab) / (float)KAA;
    if (sp.tempered) {                              // wave-uniform: the untempered step runs the code below the else, as every earlier ABI
        denoise_temper(sp, cn, allow, draws, post);
        tot = denoise_posterior_raw(ab, unif, st_ok, st, post, allow, post);
    } else tot = denoise_posterior_raw(ab, unif, st_ok, st, cn, allow, post);
    pmax = -INFINITY;
#pragma unroll
    for (int k = 0; k < KAA; ++k) {
        const float ct = (st_ok && st == k) ? 1.f : 0.f;
        post[k] = draws ? post[k] / (tot + 1e-8f) : ct;
        pmax = fmaxf(pmax, post[k]);
        if (post_out) post_out[i * KAA + k] = post[k];
    }
    int64_t sn;
    if (injected) sn = nz.s_next[i];
    else {
        float cum = 0.f, total = 0.f;
#pragma unroll
        for (int k = 0; k < KAA; ++k) total += ((allow >> k) & 1u) ? post[k] + 1e-8f : 0.f;
        const float target = useq * total;
        sn = aa_last_allowed(allow);
        for (int k = 0; k < KAA; ++k) {
            const bool ok = ((allow >> k) & 1u) != 0u;
            cum += ok ? post[k] + 1e-8f : 0.f;
            if (ok && cum > target) { sn = k; break; }
        }
    }
    return (sp.sample_sequence && allow != 0u) ? sn : st;
}

// cdf_s: the CDF row staged in LDS (or nullptr: searched in global memory).  Returns the next orientation vector through (nvx, nvy, nvz) as well.
__device__ __forceinline__ void denoise_row(int64_t i, const abopt_step_params& sp, const abopt_step_noise& nz, bool injected, const Philox& rng, uint64_t offset,
                                            const DenoiseRowIO& io, const float* cdf_s, bool need_bin, int ppl_masked, float& ppl_num, float& ppl_den,
                                            float& nvx_out, float& nvy_out, float& nvz_out) {
    const bool gen = io.mask_generate[i] != 0;
    const RowDraws d = denoise_draws(i, sp, nz, injected, rng, offset, io.igCdf, io.bins, cdf_s, need_bin);
    float ex, ey, ez, nvx, nvy, nvz;
    denoise_rot_noise(d, sp, io.igX, ex, ey, ez);
    denoise_rotation(ex, ey, ez, io.v_t + i * 3, io.v_net + i * 3, gen, nvx, nvy, nvz);
    const float zn[3] = {d.zx, d.zy, d.zz};
    float pn[3], pt[3];
    denoise_position(sp, io.p_t + i * 3, io.p_net + i * 3, zn, gen, pn, pt);
    if (!sp.sample_structure) { nvx = io.v_t[i * 3]; nvy = io.v_t[i * 3 + 1]; nvz = io.v_t[i * 3 + 2]; pn[0] = pt[0]; pn[1] = pt[1]; pn[2] = pt[2]; }
    io.v_next[i * 3] = nvx; io.v_next[i * 3 + 1] = nvy; io.v_next[i * 3 + 2] = nvz;
    denoise_store_position(i, sp, pn, io.p_next, io.p_next_norm);
    const uint32_t allow = aa_allowed_set(io.aa_allowed, i, gen);
    float post[KAA], pmax;
    const int64_t st = io.s_t[i];
    io.s_next[i] = denoise_sequence(i, sp, nz, injected, d.useq, st, io.c_net + i * KAA, allow, gen, io.post_out, post, pmax);
    // perplexity term: max softmax(post) (dpm_full.py:392-396)
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < KAA; ++k) se += expf(post[k] - pmax);
    const float w = (!ppl_masked || gen) ? 1.f : 0.f;
    ppl_num += (1.f / se) * w;
    ppl_den += w;
    nvx_out = nvx; nvy_out = nvy; nvz_out = nvz;
}

}  // namespace abopt
