// C-ABI entry points that orchestrate kernel launches (declared in include/abopt.h).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include "ipa_common.h"
#include "kernels.h"

namespace abopt {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static std::mutex g_dev_mu;
int device_cu_count(int* cus) {
    static int cached[kMaxDevices] = {};
    int dev = 0;
    ABOPT_HIP(hipGetDevice(&dev));
    ABOPT_CHECK_ARG(dev >= 0 && dev < kMaxDevices, "device ordinal %d out of range", dev);
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (!cached[dev]) {
        hipDeviceProp_t prop;
        ABOPT_HIP(hipGetDeviceProperties(&prop, dev));
        cached[dev] = prop.multiProcessorCount;
    }
    *cus = cached[dev];
    return ABOPT_OK;
}
int ensure_dynamic_lds(const void* kernel, size_t bytes, LdsConfig& cfg) {
    int dev = 0;
    ABOPT_HIP(hipGetDevice(&dev));
    ABOPT_CHECK_ARG(dev >= 0 && dev < kMaxDevices, "device ordinal %d out of range", dev);
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (bytes > cfg.bytes[dev]) {
        ABOPT_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        cfg.bytes[dev] = bytes;
    }
    return ABOPT_OK;
}

// bump allocator over the caller's workspace, 256-byte aligned carves
struct Carver {
    char* base; size_t cap, off = 0; bool ok = true;
    Carver(void* p, size_t n) : base((char*)p), cap(n) {}
    float* f(size_t nfloat) {
        const size_t bytes = (nfloat * sizeof(float) + 255) & ~(size_t)255;
        if (base && off + bytes > cap) { ok = false; return nullptr; }
        float* r = base ? (float*)(base + off) : nullptr;
        off += bytes;
        return r;
    }
};

constexpr int F = 128, FI = F + 4;
constexpr int OUT_KSPLIT = 2;     // out_transform (K = 1824, N = 128) has only M/64 * 2 tiles: split K so it fills the chip

// kvf / qf [0]: the fragment pair of its own; [1]: a second pair for carried fragments (forward_plan.h: frag_slot), aliased onto proj | feat -- carved back to back,
// and idle while carried fragments are live: their producer and their consumer both run node_frags + the fused block kernel, which touch neither (15.3 KB per
// row against 9.2 KB of fragments per padded row: it fits from L = 32 on; frag2 says whether it does, and no workspace size grows)
struct GaScratch { float *proj, *feat, *u, *kvf[2], *qf[2], *split; size_t split_floats; float* xt[2]; bool frag2; };
static GaScratch carve_ga(Carver& cv, int64_t M, int N, int L) {
    GaScratch s;
    const size_t off0 = cv.off;
    s.proj = cv.f((size_t)M * NP);
    s.feat = cv.f((size_t)M * ABOPT_IPA_FEAT);
    {
        Carver alias(s.proj, cv.off - off0);                                // over proj | feat, with the same 256-byte carves (a size query: no base, no pointers)
        s.frag2 = plan_frag2_fits((size_t)M * NP, (size_t)M * ABOPT_IPA_FEAT, ipa_kvfrag_floats(N, L), ipa_qfrag_floats(N, L));
        s.kvf[1] = s.frag2 ? alias.f(ipa_kvfrag_floats(N, L)) : nullptr;
        s.qf[1] = s.frag2 ? alias.f(ipa_qfrag_floats(N, L)) : nullptr;
    }
    s.u = cv.f((size_t)M * F * OUT_KSPLIT);
    s.kvf[0] = cv.f(ipa_kvfrag_floats(N, L));
    s.qf[0] = cv.f(ipa_qfrag_floats(N, L));
    s.split_floats = ipa_split_ws_floats(N, L);
    s.split = s.split_floats ? cv.f(s.split_floats) : nullptr;
    s.xt[0] = cv.f((size_t)M * F);          // node features as two fp16 terms, ping-pong between blocks (written by the tail / mixer, read by node_frags)
    s.xt[1] = cv.f((size_t)M * F);
    return s;
}

// The nine environment switches of the forward path, read once per C-ABI call (never cached: callers flip them between the calls of one process)
static Switches read_switches() {
    const auto first = [](const char* name) { const char* e = getenv(name); return e ? e[0] : '\0'; };
    const char c32 = first("ABOPT_CORE32");
    return {c32 == '0' ? 0 : (c32 == '1' ? 1 : -1), getenv("ABOPT_CORE_NO_SPLIT") != nullptr, first("ABOPT_FUSE_TAIL") != '0', first("ABOPT_X_TERMS") != '0',
            first("ABOPT_FUSE_HEADS") != '0', first("ABOPT_FUSE_STEP") != '0', first("ABOPT_FUSE_NODE") != '0', first("ABOPT_STEP_ROWS") != '0', first("ABOPT_STEP_COMPACT") != '0'};
}

// What every forward entry knows of its ForwardQuery (forward_plan.h): geometry, the CU count (asked once per entry), operands and scratch held, which blocks are
// packed, the switches; dbg / dump / feat_out and the network's own operands are the entry's to add
static int forward_query(int N, int L, int z_shared, const GaScratch& s, const abopt_ga_weights* blocks, int num_blocks, const float* pbc, const float* pair_terms,
                         ForwardQuery* q) {
    ABOPT_CHECK_ARG(num_blocks <= kMaxBlocks, "an encoder of %d blocks (at most %d)", num_blocks, kMaxBlocks);
    *q = ForwardQuery{};
    q->N = N; q->L = L; q->z_shared = z_shared;
    q->cache = pbc != nullptr; q->terms = pbc && pair_terms;
    q->split_ws = s.split != nullptr; q->split_ws_floats = s.split_floats;
    q->frag2 = s.frag2;
    q->num_blocks = num_blocks;
    for (int i = 0; i < num_blocks; ++i) q->blocks[i] = {blocks[i].w_node_frag != nullptr, blocks[i].w_out_frag != nullptr, blocks[i].w_mlp_frag != nullptr, blocks[i].w_out_terms != nullptr};
    q->sw = read_switches();
    return device_cu_count(&q->cus);
}

// what one block runs on, besides its plan, its weights and the scratch
struct BlockArgs { const float *R, *t, *x, *z; const uint8_t* mask; float* x_out; const float *pbc = nullptr, *pair_terms = nullptr; const abopt_ga_debug* dbg = nullptr; float* feat_out = nullptr;
                   const uint8_t* query_rows = nullptr; /* [N L]: the rows on which the LAST block's output is read, for a plan with query_rows_masked */
                   const int32_t* query_row_list = nullptr; /* the same rows as abopt_query_row_list lists them, for a plan with query_rows_compact */ };

// wnext: the next block's weights where the plan has this block write that block's fragments (carry_next), into the other fragment pair
static int ga_block(const BlockPlan& p, const ForwardQuery& q, const abopt_ga_weights* w, const BlockArgs& a, const GaScratch& s, hipStream_t st,
                    const abopt_ga_weights* wnext = nullptr, int next_qk_terms = 0) {
    const int N = q.N, L = q.L;
    float *const qf = s.qf[p.frag_slot], *const kvf = s.kvf[p.frag_slot];
    ABOPT_CHECK_ARG(!p.query_rows_masked || (a.query_rows && p.tail == TailForm::InCore), "ga_block: the plan masks query rows the call does not name");
    ABOPT_CHECK_ARG(!p.query_rows_compact || (p.query_rows_masked && a.query_row_list), "ga_block: the plan gathers query rows the call does not list");
    ABOPT_CHECK_ARG(qf && kvf && (!p.carry_next || (wnext && s.qf[1 - p.frag_slot])), "ga_block: the plan carries fragments the workspace or the weight list cannot hold");
    const int64_t M = (int64_t)N * L;
    const float* pair_terms = p.qk_terms ? a.pair_terms : nullptr;          // the term forms go together: q / k term fragments only for the core that reads pair terms
    float* xt_out = p.xt_write >= 0 ? s.xt[p.xt_write] : nullptr;
    int rc;
    // node projections q|k|v|qp|kp|vp, points to the global frame, MFMA fragment layout: one fused kernel when the packed weights are given
    if (p.carried) {
        // the previous block's fused kernel wrote them as its last phase
    } else if (p.node == NodeForm::Kernel) {
        if ((rc = launch_node_frags(a.x, w->w_node_frag, a.R, a.t, w->spatial_coef, qf, kvf, N, L, st, q.cus, p.qk_terms, p.xt_read >= 0 ? s.xt[p.xt_read] : nullptr))) return rc;
    } else {
        if ((rc = launch_linear(a.x, F, w->w_node, F, nullptr, s.proj, NP, (int)M, ABOPT_NODE_PROJ, F, false, st))) return rc;
        if ((rc = launch_ipa_frags(s.proj, a.R, a.t, w->spatial_coef, qf, kvf, N, L, st))) return rc;
    }
    // core + tail as one kernel (feat stays on the chip); bit-identical to the two launches below
    if (p.tail == TailForm::InCore) {
        const NodeCarryArgs nc{wnext ? wnext->w_node_frag : nullptr, wnext ? wnext->spatial_coef : nullptr, s.qf[1 - p.frag_slot], s.kvf[1 - p.frag_slot], next_qk_terms};
        return launch_ipa_block_fused(p.core, qf, kvf, a.z, a.mask, a.R, a.t, a.pbc, N, L, st, q.z_shared, w->w_out_terms, w->w_mlp_frag, a.x, w->b_out, w->ln1_gamma,
                                      w->ln1_beta, w->b_mlp0, w->b_mlp1, w->b_mlp2, w->ln2_gamma, w->ln2_beta, a.x_out, pair_terms, xt_out, p.carry_next ? &nc : nullptr,
                                      p.query_rows_masked ? a.query_rows : nullptr, p.query_rows_compact ? a.query_row_list : nullptr, p.query_rows_compact);
    }
    float* feat = (a.dbg && a.dbg->feat) ? a.dbg->feat : (a.feat_out ? a.feat_out : s.feat);
    if ((rc = launch_ipa_core(p.core, qf, kvf, a.z, a.mask, a.R, a.t, w->w_pair_bias, feat, a.dbg ? a.dbg->logits : nullptr, a.dbg ? a.dbg->alpha : nullptr, a.pbc,
                              N, L, st, q.z_shared, s.split, pair_terms))) return rc;
    // out_transform -> mask -> +x -> LN1 -> MLP -> +res -> LN2
    if (p.tail == TailForm::OutLnMlp)
        return launch_out_ln_mlp(feat, w->w_out_frag, w->w_mlp_frag, a.x, w->b_out, a.mask, w->ln1_gamma, w->ln1_beta, w->b_mlp0, w->b_mlp1, w->b_mlp2,
                                 w->ln2_gamma, w->ln2_beta, a.x_out, nullptr, M, st, xt_out);
    if ((rc = launch_linear(feat, ABOPT_IPA_FEAT, w->w_out, ABOPT_IPA_FEAT, nullptr, s.u, F, (int)M, F, ABOPT_IPA_FEAT, false, st, OUT_KSPLIT, M * F))) return rc;
    return launch_fused_ln_mlp(a.x, s.u, OUT_KSPLIT, M * F, w->b_out, a.mask, w->ln1_gamma, w->ln1_beta, w->w_mlp0, w->b_mlp0, w->w_mlp1, w->b_mlp1,
                               w->w_mlp2, w->b_mlp2, w->ln2_gamma, w->ln2_beta, a.x_out, M, st);
}

static int check_ga_weights(const abopt_ga_weights* w) {
    ABOPT_CHECK_ARG(w && w->w_node && w->w_pair_bias && w->spatial_coef && w->w_out && w->b_out && w->ln1_gamma && w->ln1_beta &&
                    w->w_mlp0 && w->b_mlp0 && w->w_mlp1 && w->b_mlp1 && w->w_mlp2 && w->b_mlp2 && w->ln2_gamma && w->ln2_beta,
                    "GABlock weights: NULL pointer");
    return ABOPT_OK;
}

}  // namespace abopt

using namespace abopt;

extern "C" int abopt_abi_version(void) { return ABOPT_ABI_VERSION; }

extern "C" size_t abopt_node_frag_floats(void) { return node_wfrag_floats(); }
extern "C" int abopt_node_frag_source_row(int h, int T, int m) {
    if (h < 0 || h >= H || T < 0 || T >= 12 || m < 0 || m >= 16) return -1;
    static const int kSet[12] = {0, 0, 1, 1, 3, 3, 4, 4, 2, 2, 5, 5};   // tile -> projection: 0 q, 1 k, 2 v, 3 q_pts, 4 k_pts, 5 v_pts
    const int set = kSet[T], half = T % 2;
    if (set < 3) return set * (H * D) + h * D + half * 16 + m;
    const int p = half * 4 + m / 4, c = m % 4;
    if (c == 3) return -1;
    return 3 * H * D + (set - 3) * NPT + h * (P * 3) + p * 3 + c;
}
extern "C" const char* abopt_last_error(void) { return g_err; }

extern "C" size_t abopt_heads_frag_floats(void) { return heads_wfrag_floats(); }
extern "C" size_t abopt_mixer_frag_floats(void) { return mixer_wfrag_floats(); }
extern "C" size_t abopt_out_frag_floats(void) { return out_wfrag_floats(); }
extern "C" size_t abopt_mlp_frag_floats(void) { return mlp_wfrag_floats(); }
extern "C" size_t abopt_out_terms_floats(void) { return out_wterms_floats(); }
extern "C" int abopt_out_frag_terms(const float* w_out_frag, float* w_out_terms, abopt_stream stream) {
    ABOPT_CHECK_ARG(w_out_frag && w_out_terms, "out_frag_terms: NULL argument");
    return launch_out_frag_terms(w_out_frag, w_out_terms, (hipStream_t)stream);
}
extern "C" int abopt_pack_tail_weights(const float* w_out, const float* w_mlp0, const float* w_mlp1, const float* w_mlp2, float* w_out_frag,
                                       float* w_mlp_frag, float* w_mlpT_frag, abopt_stream stream) {
    ABOPT_CHECK_ARG(w_out && w_mlp0 && w_mlp1 && w_mlp2 && w_out_frag && w_mlp_frag, "pack_tail_weights: NULL argument");
    return launch_pack_tail_weights(w_out, w_mlp0, w_mlp1, w_mlp2, w_out_frag, w_mlp_frag, w_mlpT_frag, (hipStream_t)stream);
}
extern "C" int abopt_block_tail_forward(const float* feat, const float* w_out_frag, const float* w_mlp_frag, const float* x, const float* b_out,
                                        const uint8_t* mask, const float* ln1_gamma, const float* ln1_beta, const float* b_mlp0, const float* b_mlp1,
                                        const float* b_mlp2, const float* ln2_gamma, const float* ln2_beta, float* out, float* saved, int64_t rows,
                                        abopt_stream stream) {
    ABOPT_CHECK_ARG(rows >= 0, "block_tail_forward: negative row count");
    if (rows == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(feat && w_out_frag && w_mlp_frag && x && ln1_gamma && ln1_beta && b_mlp0 && b_mlp1 && b_mlp2 && ln2_gamma && ln2_beta && out,
                    "block_tail_forward: NULL argument");
    return launch_out_ln_mlp(feat, w_out_frag, w_mlp_frag, x, b_out, mask, ln1_gamma, ln1_beta, b_mlp0, b_mlp1, b_mlp2, ln2_gamma, ln2_beta, out, saved,
                             rows, (hipStream_t)stream);
}
extern "C" int abopt_block_tail_backward(const float* dout, const float* saved, const float* w_mlpT_frag, const uint8_t* mask, const float* ln1_gamma,
                                         const float* ln2_gamma, float* dpre, float* da1, float* du, float* colpart, int64_t rows, abopt_stream stream) {
    ABOPT_CHECK_ARG(rows >= 0, "block_tail_backward: negative row count");
    if (rows == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(dout && saved && w_mlpT_frag && ln1_gamma && ln2_gamma && dpre && da1 && du && colpart, "block_tail_backward: NULL argument");
    return launch_tail_backward(dout, saved, w_mlpT_frag, mask, ln1_gamma, ln2_gamma, dpre, da1, du, colpart, rows, (hipStream_t)stream);
}

extern "C" int abopt_device_info(int* cu_count, int* lds_bytes_per_cu, char* arch, int arch_len) {
    int dev = 0;
    ABOPT_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    ABOPT_HIP(hipGetDeviceProperties(&prop, dev));
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (lds_bytes_per_cu) *lds_bytes_per_cu = (int)prop.maxSharedMemoryPerMultiProcessor;
    if (arch && arch_len > 0) { strncpy(arch, prop.gcnArchName, arch_len - 1); arch[arch_len - 1] = 0; }
    return ABOPT_OK;
}

static int check_encode_inputs(const abopt_encode_inputs* in, const char* who) {
    ABOPT_CHECK_ARG(in, "%s: NULL inputs", who);
    ABOPT_CHECK_ARG(in->N >= 0 && in->L >= 0 && (int64_t)in->N * in->L < (1ll << 31) / 64, "%s: bad batch dims N=%d L=%d", who, in->N, in->L);
    if ((int64_t)in->N * in->L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(in->aa && in->res_nb && in->chain_nb && in->pos_atoms && in->mask_atoms, "%s: NULL input tensor", who);
    return ABOPT_OK;
}

extern "C" size_t abopt_residue_embed_workspace_bytes(int N, int L, int atoms, int hotspot) { return residue_embed_ws_bytes(N, L, atoms, hotspot); }
extern "C" size_t abopt_pair_embed_workspace_bytes(int N, int L, int atoms) { return pair_embed_ws_bytes(N, L, atoms); }

extern "C" int abopt_residue_embed_forward(const abopt_encode_inputs* in, const abopt_residue_embed_weights* w, float* res_feat, float* R, float* p,
                                           void* ws, size_t ws_bytes, abopt_stream stream) {
    int rc;
    if ((rc = check_encode_inputs(in, "residue_embed_forward"))) return rc;
    if ((int64_t)in->N * in->L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(in->fragment_type && w && w->aatype_embed && w->type_embed && w->freq_bands && w->w0 && w->b0 && w->w1 && w->b1 && w->w2 && w->b2 && w->w3 && w->b3 && ws,
                    "residue_embed_forward: NULL argument");
    return launch_residue_embed(in, w, res_feat, R, p, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" size_t abopt_residue_features_workspace_bytes(int N, int L) { return residue_features_ws_bytes(N, L); }

extern "C" int abopt_residue_features(const abopt_encode_inputs* in, const abopt_residue_embed_weights* w, float* features, float* R, float* p,
                                      void* ws, size_t ws_bytes, abopt_stream stream) {
    int rc;
    if ((rc = check_encode_inputs(in, "residue_features"))) return rc;
    if ((int64_t)in->N * in->L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(in->fragment_type && w && w->aatype_embed && w->type_embed && w->freq_bands && features && R && p && ws, "residue_features: NULL argument");
    return launch_residue_features(in, w, features, R, p, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int abopt_pair_embed_forward(const abopt_encode_inputs* in, const abopt_pair_embed_weights* w, float* pair_feat, float* activations,
                                        float* gauss, float* dgauss, void* ws, size_t ws_bytes, abopt_stream stream) {
    int rc;
    if ((rc = check_encode_inputs(in, "pair_embed_forward"))) return rc;
    if ((int64_t)in->N * in->L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(w && w->aa_pair_embed && w->relpos_embed && w->aapair_to_distcoef && w->freq_bands && w->wd0 && w->bd0 && w->wd1 && w->bd1 &&
                    w->wo0 && w->bo0 && w->wo1 && w->bo1 && w->wo2 && w->bo2 && pair_feat && ws, "pair_embed_forward: NULL argument");
    ABOPT_CHECK_ARG(gauss || !dgauss, "pair_embed_forward: dgauss needs gauss");
    return launch_pair_embed(in, w, pair_feat, activations, gauss, dgauss, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" size_t abopt_pair_embed_backward_workspace_bytes(int N, int L, int atoms) { return pair_embed_backward_ws_bytes(N, L, atoms); }

extern "C" int abopt_pair_embed_backward(const abopt_encode_inputs* in, const abopt_pair_embed_weights* w, const float* dpair_feat,
                                         const float* activations, const float* dgauss, float* dys, float* dsoftplus, float* dys_colsum,
                                         void* ws, size_t ws_bytes, abopt_stream stream) {
    int rc;
    if ((rc = check_encode_inputs(in, "pair_embed_backward"))) return rc;
    if ((int64_t)in->N * in->L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(w && w->wd0 && w->wd1 && w->wo0 && w->wo1 && w->wo2 && dpair_feat && activations && dys && dsoftplus && ws && w->aapair_to_distcoef && w->aa_pair_embed && w->relpos_embed,
                    "pair_embed_backward: NULL argument");
    return launch_pair_embed_backward(in, w, dpair_feat, activations, dgauss, dys, dsoftplus, dys_colsum, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int abopt_dpm_losses(const float* R_pred, const float* R_0, const float* p_pred, const float* p_target, const float* c_denoised, const int64_t* s_t,
                                const int64_t* s_0, const float* alpha_bar_t, const uint8_t* mask_generate, int N, int L, float* block_sums, float* dR_pred,
                                float* dp_pred, float* dc_denoised, abopt_stream stream) {
    ABOPT_CHECK_ARG(N >= 0 && L >= 0 && R_pred && R_0 && p_pred && p_target && c_denoised && s_t && s_0 && alpha_bar_t && mask_generate && block_sums && dR_pred &&
                    dp_pred && dc_denoised, "dpm_losses: NULL argument");
    return launch_dpm_losses(R_pred, R_0, p_pred, p_target, c_denoised, s_t, s_0, alpha_bar_t, mask_generate, N, L, block_sums, dR_pred, dp_pred, dc_denoised,
                             (hipStream_t)stream);
}

extern "C" int abopt_abdock_losses(const float* prmsd_logits, const float* p_pred, const float* p0_norm, const float* coef_a, const float* coef_b,
                                   const uint8_t* mask_generate, const uint8_t* mask_res, const float* bin_offsets, int num_bins, int N, int L, float position_scale,
                                   int pred_x0, float* sample_parts, float* dprmsd_logits, float* dp_pred, abopt_stream stream) {
    ABOPT_CHECK_ARG(N >= 0 && L >= 0 && prmsd_logits && p_pred && p0_norm && mask_generate && mask_res && bin_offsets && sample_parts && dprmsd_logits && dp_pred &&
                    (pred_x0 || (coef_a && coef_b)), "abdock_losses: NULL argument");
    return launch_abdock_losses(prmsd_logits, p_pred, p0_norm, coef_a, coef_b, mask_generate, mask_res, bin_offsets, num_bins, N, L, position_scale, pred_x0,
                                sample_parts, dprmsd_logits, dp_pred, (hipStream_t)stream);
}

extern "C" int abopt_layer_norm_forward(const float* x, const float* gamma, const float* beta, int cols, float eps, int64_t rows, float* y, float* xhat, float* rstd,
                                        abopt_stream stream) {
    ABOPT_CHECK_ARG(rows >= 0 && x && gamma && beta && y && (!xhat == !rstd), "layer_norm_forward: NULL argument (xhat and rstd come together)");
    return launch_row_layer_norm(x, gamma, beta, cols, eps, rows, y, xhat, rstd, (hipStream_t)stream);
}
extern "C" int abopt_layer_norm_backward(const float* dy, const float* xhat, const float* rstd, const float* gamma, int cols, int64_t rows, float* dx, float* dy_xhat,
                                         abopt_stream stream) {
    ABOPT_CHECK_ARG(rows >= 0 && dy && xhat && rstd && gamma && dx && dy_xhat, "layer_norm_backward: NULL argument");
    return launch_row_layer_norm_backward(dy, xhat, rstd, gamma, cols, rows, dx, dy_xhat, (hipStream_t)stream);
}

extern "C" int abopt_heads_epilogue_forward(const float* R, const float* v_t, const float* eps_crd, const float* eps_rot, const uint8_t* mask_generate,
                                            float* v_next, float* R_next, float* eps_pos, int64_t rows, int grad_mode, abopt_stream stream) {
    ABOPT_CHECK_ARG(rows >= 0 && R && eps_crd && eps_rot && mask_generate && R_next && eps_pos && (!v_next || v_t), "heads_epilogue_forward: NULL argument");
    return launch_heads_epilogue(R, v_t, eps_crd, eps_rot, nullptr, 3, 0, mask_generate, v_next, R_next, eps_pos, nullptr, rows, grad_mode, (hipStream_t)stream);
}

extern "C" int abopt_heads_epilogue_backward(const float* R, const float* eps_rot, const uint8_t* mask_generate, const float* dR_next, const float* deps_pos,
                                             float* deps_crd, float* deps_rot, int64_t rows, abopt_stream stream) {
    ABOPT_CHECK_ARG(rows >= 0 && R && eps_rot && mask_generate && deps_crd && deps_rot, "heads_epilogue_backward: NULL argument");
    return launch_heads_epilogue_backward(R, eps_rot, 3, mask_generate, dR_next, deps_pos, deps_crd, deps_rot, rows, (hipStream_t)stream);
}

extern "C" int abopt_reconstruct_backbone_partially(const float* pos_ctx, const float* R_new, const float* t_new, const int64_t* aa,
                                                    const int64_t* chain_nb, const int64_t* res_nb, const uint8_t* mask_atoms,
                                                    const uint8_t* mask_recons, const float* bb_table, const float* o_table,
                                                    float* pos_new, uint8_t* mask_new, int N, int L, int A, abopt_stream stream) {
    ABOPT_CHECK_ARG(N >= 0 && L >= 0 && A >= 4, "reconstruct_backbone_partially: bad dims N=%d L=%d A=%d (A >= 4)", N, L, A);
    if ((int64_t)N * L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(pos_ctx && R_new && t_new && aa && chain_nb && res_nb && mask_atoms && mask_recons && bb_table && o_table && pos_new && mask_new,
                    "reconstruct_backbone_partially: NULL argument");
    return launch_reconstruct_backbone(pos_ctx, R_new, t_new, aa, chain_nb, res_nb, mask_atoms, mask_recons, bb_table, o_table, pos_new, mask_new,
                                       N, L, A, (hipStream_t)stream);
}

extern "C" int abopt_so3_exp(const float* w, float* R, int64_t n, abopt_stream stream) {
    ABOPT_CHECK_ARG(w && R && n >= 0, "so3_exp: bad arguments");
    return launch_so3_exp(w, R, n, (hipStream_t)stream);
}
extern "C" int abopt_so3_log(const float* R, float* w, int64_t n, int grad_mode, abopt_stream stream) {
    ABOPT_CHECK_ARG(w && R && n >= 0, "so3_log: bad arguments");
    return launch_so3_log(R, w, n, grad_mode, (hipStream_t)stream);
}

extern "C" size_t abopt_ga_workspace_bytes(int N, int L, int Fd, int Cd) {
    (void)Fd; (void)Cd;
    Carver cv(nullptr, 0);
    const int64_t M = (int64_t)N * L;
    carve_ga(cv, M, N, L);
    cv.f((size_t)M * F);   // ping-pong buffer for the encoder
    return cv.off;
}

static int check_dims(int N, int L, int Fd, int Cd) {
    ABOPT_CHECK_ARG(N >= 0 && L >= 0, "negative batch dims N=%d L=%d", N, L);
    if (Fd != F || Cd != C) { set_error("this build supports res_feat_dim=128, pair_feat_dim=64 only (got %d, %d)", Fd, Cd); return ABOPT_EUNSUPPORTED; }
    ABOPT_CHECK_ARG((int64_t)N * L < (1ll << 31) / 64, "N*L too large");
    return ABOPT_OK;
}

extern "C" size_t abopt_ipa_train_workspace_bytes(int N, int L) { return ipa_train_ws_floats(N, L) * sizeof(float); }

extern "C" int abopt_ipa_core_train_forward(const float* proj_local, const float* R, const float* t, const float* pair_feat, const uint8_t* mask,
                                            const float* w_pair_bias, const float* spatial_coef, const float* pair_bias_cache, float* feat,
                                            float* alpha, int N, int L, int Cd, void* ws, size_t ws_bytes, abopt_stream stream) {
    int rc;
    if ((rc = check_dims(N, L, F, Cd))) return rc;
    if ((int64_t)N * L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(proj_local && R && t && pair_feat && mask && w_pair_bias && spatial_coef && feat && alpha && ws, "ipa_core_train_forward: NULL argument");
    if (pair_bias_cache && !bias_slab_fits_u32(N, L)) {                     // before anything is launched
        set_error("ipa_core_train_forward: the training core reads a pair-bias cache through 32-bit offsets and this one (%d x %d rows) is 4 GB or more per layer; pass none", N, L);
        return ABOPT_EUNSUPPORTED;
    }
    if (ws_bytes < ipa_train_ws_floats(N, L) * sizeof(float)) { set_error("ipa_core_train_forward: workspace too small (%zu bytes given)", ws_bytes); return ABOPT_EWORKSPACE; }
    return launch_ipa_train_forward(proj_local, R, t, pair_feat, mask, w_pair_bias, spatial_coef, pair_bias_cache, feat, alpha, N, L, (float*)ws,
                                    (hipStream_t)stream);
}

extern "C" int abopt_ipa_points_backward(const float* dfeat, int ld_dfeat, const float* feat, const float* R, const float* t,
                                         float* dout_cat, float* delta, int N, int L, abopt_stream stream) {
    ABOPT_CHECK_ARG(N >= 0 && L >= 0, "ipa_points_backward: negative dims");
    if ((int64_t)N * L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(dfeat && feat && R && t && dout_cat && delta && ld_dfeat >= ABOPT_IPA_FEAT, "ipa_points_backward: bad argument");
    return launch_ipa_points_backward(dfeat, ld_dfeat, feat, R, t, dout_cat, delta, N, L, (hipStream_t)stream);
}

extern "C" int abopt_ipa_backward_operands(const float* proj_local, const float* R, const float* t, float* Aq, float* Ak, float* Av,
                                           int N, int L, abopt_stream stream) {
    ABOPT_CHECK_ARG(N >= 0 && L >= 0, "ipa_backward_operands: negative dims");
    if ((int64_t)N * L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(proj_local && R && t && Aq && Ak && Av, "ipa_backward_operands: NULL argument");
    return launch_ipa_backward_operands(proj_local, R, t, Aq, Ak, Av, N, L, (hipStream_t)stream);
}

extern "C" int abopt_ipa_backward_assemble(const float* P1, const float* P2, const float* P3, const float* Aq, const float* Ak, const float* R,
                                           const float* spatial_coef, float* dproj, float* e, int N, int L, abopt_stream stream) {
    ABOPT_CHECK_ARG(N >= 0 && L >= 0, "ipa_backward_assemble: negative dims");
    if ((int64_t)N * L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(P1 && P2 && P3 && Aq && Ak && R && spatial_coef && dproj && e, "ipa_backward_assemble: NULL argument");
    return launch_ipa_backward_assemble(P1, P2, P3, Aq, Ak, R, spatial_coef, dproj, e, N, L, (hipStream_t)stream);
}

extern "C" int abopt_ipa_pair_backward(const float* pair_feat, const float* alpha, const float* dalpha_node, const float* delta,
                                       const float* dfeat, int ld_dfeat, const float* w_pair_bias, float* g, float* dpair_feat,
                                       float* dw_pair_bias_rows, int dpair_feat_accumulate, int N, int L, int Cd, abopt_stream stream) {
    int rc;
    if ((rc = check_dims(N, L, F, Cd))) return rc;
    if ((int64_t)N * L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(pair_feat && alpha && dalpha_node && delta && dfeat && w_pair_bias && g && dw_pair_bias_rows && ld_dfeat >= ABOPT_HEADS * 64 && (ld_dfeat % 4) == 0,
                    "ipa_pair_backward: bad argument");          // dpair_feat may be NULL: d pair_feat is then left to abopt_ipa_dz_assemble
    return launch_ipa_pair_backward(pair_feat, alpha, dalpha_node, delta, dfeat, ld_dfeat, w_pair_bias, g, dpair_feat, dw_pair_bias_rows, N, L, (hipStream_t)stream,
                                    dpair_feat_accumulate ? 1 : 0);
}

extern "C" int abopt_ipa_dz_assemble(int num_blocks, const float* const* alpha, const float* const* g, const float* const* dfeat, int ld_dfeat,
                                     const float* const* w_pair_bias, float* dpair_feat, int N, int L, int Cd, abopt_stream stream) {
    int rc;
    if ((rc = check_dims(N, L, F, Cd))) return rc;
    ABOPT_CHECK_ARG(alpha && g && dfeat && w_pair_bias && dpair_feat && ld_dfeat >= ABOPT_HEADS * 64 && (ld_dfeat % 4) == 0, "ipa_dz_assemble: bad argument");
    return launch_ipa_dz_assemble(num_blocks, alpha, g, dfeat, ld_dfeat, w_pair_bias, dpair_feat, N, L, (hipStream_t)stream);
}

extern "C" int abopt_ga_block_forward(const abopt_ga_weights* w, const float* R, const float* t, const float* x, const float* z,
                                      const uint8_t* mask, float* x_out, int N, int L, int Fd, int Cd, const abopt_ga_debug* dbg,
                                      void* ws, size_t ws_bytes, abopt_stream stream) {
    int rc;
    if ((rc = check_dims(N, L, Fd, Cd))) return rc;
    if ((rc = check_ga_weights(w))) return rc;
    if ((int64_t)N * L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(R && t && x && z && mask && x_out && ws, "ga_block_forward: NULL argument");
    Carver cv(ws, ws_bytes);
    GaScratch s = carve_ga(cv, (int64_t)N * L, N, L);
    if (!cv.ok) { set_error("ga_block_forward: workspace too small (%zu bytes given)", ws_bytes); return ABOPT_EWORKSPACE; }
    ForwardQuery q;
    if ((rc = forward_query(N, L, 0, s, w, 1, nullptr, nullptr, &q))) return rc;
    q.dbg = dbg != nullptr; q.dump = dbg && (dbg->logits || dbg->alpha);
    BlockArgs a{R, t, x, z, mask, x_out};
    a.dbg = dbg;
    return ga_block(plan_block(q, 0), q, w, a, s, (hipStream_t)stream);
}

extern "C" int abopt_ga_block_forward_cached(const abopt_ga_weights* w, const float* R, const float* t, const float* x, const float* z,
                                             const uint8_t* mask, float* x_out, int N, int L, int Fd, int Cd, const float* pair_bias_cache,
                                             const float* pair_terms, int pair_feat_shared, float* feat_out, void* ws, size_t ws_bytes, abopt_stream stream) {
    int rc;
    if ((rc = check_dims(N, L, Fd, Cd))) return rc;
    if ((rc = check_ga_weights(w))) return rc;
    if ((int64_t)N * L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(R && t && x && z && mask && x_out && ws && pair_bias_cache, "ga_block_forward_cached: NULL argument");
    ABOPT_CHECK_ARG(pair_feat_shared >= 0 && (pair_feat_shared <= 1 || N % pair_feat_shared == 0), "ga_block_forward_cached: pair_feat_shared=%d does not divide N=%d", pair_feat_shared, N);
    Carver cv(ws, ws_bytes);
    GaScratch s = carve_ga(cv, (int64_t)N * L, N, L);
    if (!cv.ok) { set_error("ga_block_forward_cached: workspace too small (%zu bytes given)", ws_bytes); return ABOPT_EWORKSPACE; }
    const int zg = pair_feat_shared == 1 ? N : pair_feat_shared;
    ForwardQuery q;
    if ((rc = forward_query(N, L, zg, s, w, 1, pair_bias_cache, pair_terms, &q))) return rc;
    q.feat_out = feat_out != nullptr;
    BlockArgs a{R, t, x, z, mask, x_out, pair_bias_cache, pair_terms};
    a.feat_out = feat_out;
    return ga_block(plan_block(q, 0), q, w, a, s, (hipStream_t)stream);
}

static int ga_encoder(const EncoderPlan& e, const ForwardQuery& q, const abopt_ga_weights* blocks, BlockArgs a, const GaScratch& s, float* pong, hipStream_t st) {
    // ga.py:190-193: the same R, t, z feed every block.  Ping-pong so the last block writes x_out.  (x as fp16 terms travels with x through the slots of the plan.)
    float* const x_out = a.x_out;
    const float* const pbc = a.pbc;
    for (int i = 0; i < e.num_blocks; ++i) {            // a plan that ends in an Unsupported core ends here with that core's error
        a.x_out = ((q.num_blocks - 1 - i) % 2 == 0) ? x_out : pong;
        a.pbc = pbc ? pbc + (size_t)i * pair_bias_layer_floats(q.z_shared ? q.N / q.z_shared : q.N, q.L) : nullptr;
        const bool carry = e.blocks[i].carry_next;                          // (then block i + 1 is planned: its fragments take the form its own plan asks for)
        if (int rc = ga_block(e.blocks[i], q, &blocks[i], a, s, st, carry ? &blocks[i + 1] : nullptr, carry ? (int)e.blocks[i + 1].qk_terms : 0)) return rc;
        a.x = a.x_out;
    }
    if (q.num_blocks == 0) ABOPT_HIP(hipMemcpyAsync(x_out, a.x, (size_t)q.N * q.L * F * sizeof(float), hipMemcpyDeviceToDevice, st));
    return ABOPT_OK;
}

extern "C" int abopt_ga_encoder_forward(const abopt_ga_weights* blocks, int num_layers, const float* R, const float* t, const float* x,
                                        const float* z, const uint8_t* mask, float* x_out, int N, int L, int Fd, int Cd,
                                        void* ws, size_t ws_bytes, abopt_stream stream) {
    int rc;
    if ((rc = check_dims(N, L, Fd, Cd))) return rc;
    ABOPT_CHECK_ARG(blocks && num_layers >= 0, "ga_encoder_forward: bad block list");
    for (int i = 0; i < num_layers; ++i) if ((rc = check_ga_weights(&blocks[i]))) return rc;
    if ((int64_t)N * L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(R && t && x && z && mask && x_out && ws, "ga_encoder_forward: NULL argument");
    ABOPT_CHECK_ARG(x != x_out, "ga_encoder_forward: x_out must not alias x");
    Carver cv(ws, ws_bytes);
    const int64_t M = (int64_t)N * L;
    GaScratch s = carve_ga(cv, M, N, L);
    float* pong = cv.f((size_t)M * F);
    if (!cv.ok) { set_error("ga_encoder_forward: workspace too small (%zu bytes given)", ws_bytes); return ABOPT_EWORKSPACE; }
    ForwardQuery q;
    if ((rc = forward_query(N, L, 0, s, blocks, num_layers, nullptr, nullptr, &q))) return rc;
    return ga_encoder(plan_encoder(q), q, blocks, BlockArgs{R, t, x, z, mask, x_out}, s, pong, (hipStream_t)stream);
}

extern "C" size_t abopt_pair_bias_cache_bytes(int N, int L, int num_layers) {
    return (size_t)num_layers * pair_bias_layer_floats(N, L) * sizeof(float);
}

extern "C" int abopt_nonfinite_flag(int reset, abopt_stream stream) {
    int flag = 0;
    const int rc = nonfinite_flag_read(reset, (hipStream_t)stream, &flag);
    return rc ? -1 : flag;
}

extern "C" int abopt_nonfinite_flag_reset(abopt_stream stream) { return nonfinite_flag_reset((hipStream_t)stream); }

extern "C" size_t abopt_pair_terms_bytes(int N, int L) { return pair_terms_blob_floats(N, L) * sizeof(float); }

extern "C" int abopt_pair_terms_used(int N, int L, int pair_feat_shared) {
    int cus = 0;
    if (N <= 0 || L <= 0 || device_cu_count(&cus)) return 0;
    return plan_pair_terms_used(N, L, pair_feat_shared, cus, read_switches()) ? 1 : 0;
}

extern "C" int abopt_pair_terms(const float* pair_feat, float* terms, int N, int L, int Cd, abopt_stream stream) {
    int rc;
    if ((rc = check_dims(N, L, 128, Cd))) return rc;
    ABOPT_CHECK_ARG(pair_feat && terms, "pair_terms: NULL argument");
    ABOPT_CHECK_ARG(L <= 2048, "pair_terms: L=%d (the kernels that read the terms address a sample's slab with 32-bit offsets: L <= 2048)", L);
    return launch_pair_terms(pair_feat, terms, N, L, (hipStream_t)stream);
}

extern "C" int abopt_pair_bias_cache(const abopt_ga_weights* blocks, int num_layers, const float* pair_feat, float* cache,
                                     int N, int L, int Cd, abopt_stream stream) {
    int rc;
    if ((rc = check_dims(N, L, 128, Cd))) return rc;
    ABOPT_CHECK_ARG(blocks && pair_feat && cache && num_layers >= 1 && num_layers <= 8, "pair_bias_cache: bad arguments");
    const float* wb[8];
    for (int l = 0; l < num_layers; ++l) { ABOPT_CHECK_ARG(blocks[l].w_pair_bias, "pair_bias_cache: NULL weight"); wb[l] = blocks[l].w_pair_bias; }
    return launch_pair_bias_cache(pair_feat, wb, num_layers, cache, N, L, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------- EpsilonNet
namespace {
struct EpsScratch { GaScratch ga; float *pong, *R, *cat, *x0, *xe, *infeat, *infeat_ln, *hh1, *hh2, *out3, *pr1, *pr2, *pr3; };
EpsScratch carve_eps(Carver& cv, int64_t M, int N, int L, int num_bins) {
    EpsScratch e;
    e.ga = carve_ga(cv, M, N, L);
    e.pong = cv.f((size_t)M * F);
    e.R = cv.f((size_t)M * 9);
    e.cat = cv.f((size_t)M * 2 * F);
    e.x0 = cv.f((size_t)M * F);
    e.xe = cv.f((size_t)M * F);
    e.infeat = cv.f((size_t)M * FI);
    e.infeat_ln = cv.f((size_t)M * FI);
    e.hh1 = cv.f((size_t)M * 3 * F);
    e.hh2 = cv.f((size_t)M * 3 * F);
    e.out3 = cv.f((size_t)M * 32);
    e.pr1 = cv.f((size_t)M * F);
    e.pr2 = cv.f((size_t)M * F);
    e.pr3 = cv.f((size_t)M * (size_t)(num_bins > 0 ? num_bins : 1));
    return e;
}
// what abopt_eps_net_step adds to a forward: the arguments of abopt_denoise_step that the forward does not have already, and the carry
struct StepCall {
    const abopt_step_params* sp; const abopt_step_noise* noise; uint64_t seed, offset; const float* p_angstrom; const float *igX, *igCdf; int bins, num_bins;
    float *v_next, *p_next; int64_t* s_next; float *prmsd, *ppl, *post_out, *p_next_norm; const uint64_t* seed_dev; const int32_t* aa_allowed; int carry_in, carry_out;
    int context_unused; const int32_t* query_row_list; int query_row_tiles;      // the loop's two optional facts; a row list implies context_unused
};
}  // namespace

extern "C" size_t abopt_eps_workspace_bytes(int N, int L, int Fd, int Cd) {
    (void)Fd; (void)Cd;
    Carver cv(nullptr, 0);
    carve_eps(cv, (int64_t)N * L, N, L, 64);
    return cv.off;
}

// EpsilonNet.forward and, sc given (abopt_eps_net_step), the step's transitions behind it -- as the plan says: the heads' launches + denoise_step, or the fused tail
static int eps_forward(const abopt_eps_weights* w, const float* v_t, const float* p_t, const int64_t* s_t,
                       const float* res_feat, const float* pair_feat, const float* beta,
                       const uint8_t* mask_generate, const uint8_t* mask_res,
                       float* v_next, float* R_next, float* eps_pos, float* c_denoised, float* prmsd_logits,
                       int N, int L, int Fd, int Cd, int grad_mode, const float* pair_bias_cache, int pair_feat_shared,
                       const float* pair_terms, void* ws, size_t ws_bytes, abopt_stream stream, const StepCall* sc) {
    int rc;
    if ((rc = check_dims(N, L, Fd, Cd))) return rc;
    ABOPT_CHECK_ARG(w && w->seq_embed && w->w_mix0 && w->b_mix0 && w->w_mix1 && w->b_mix1 && w->blocks && w->w_head1 && w->b_head1 &&
                    w->w_crd2 && w->b_crd2 && w->w_crd3 && w->b_crd3 && w->w_rot2 && w->b_rot2 && w->w_rot3 && w->b_rot3 &&
                    w->w_seq2 && w->b_seq2 && w->w_seq3 && w->b_seq3, "eps_net_forward: NULL weight pointer");
    for (int i = 0; i < w->num_layers; ++i) if ((rc = check_ga_weights(&w->blocks[i]))) return rc;
    if ((int64_t)N * L == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(v_t && p_t && s_t && res_feat && pair_feat && beta && mask_generate && mask_res && v_next && R_next && eps_pos && c_denoised && ws,
                    "eps_net_forward: NULL argument");
    const bool has_prmsd = w->w_prmsd1 != nullptr;
    ABOPT_CHECK_ARG(!has_prmsd || (prmsd_logits && w->prmsd_ln_gamma && w->prmsd_ln_beta && w->b_prmsd1 && w->w_prmsd2 && w->b_prmsd2 &&
                                   w->w_prmsd3 && w->b_prmsd3 && w->num_bins > 0 && w->num_bins <= 64), "eps_net_forward: incomplete prmsd head");
    hipStream_t st = (hipStream_t)stream;
    const int64_t M = (int64_t)N * L;
    if (M == 0) return ABOPT_OK;
    // pair_feat_shared: 0 distinct | 1 one entry for the whole batch | g > 1 consecutive groups of g samples share an entry
    ABOPT_CHECK_ARG(pair_feat_shared >= 0 && (pair_feat_shared <= 1 || N % pair_feat_shared == 0), "eps_net_forward: pair_feat_shared=%d does not divide N=%d", pair_feat_shared, N);
    ABOPT_CHECK_ARG(!pair_feat_shared || pair_bias_cache, "eps_net_forward: a shared pair_feat comes with its pair-bias cache");
    ABOPT_CHECK_ARG(!pair_terms || pair_bias_cache, "eps_net_forward: pair_terms come with the pair-bias cache of the same pair_feat");
    const int zg = pair_feat_shared == 1 ? N : pair_feat_shared;
    Carver cv(ws, ws_bytes);
    EpsScratch e = carve_eps(cv, M, N, L, 64);
    if (!cv.ok) { set_error("eps_net_forward: workspace too small (%zu bytes given, %zu needed)", ws_bytes, abopt_eps_workspace_bytes(N, L, Fd, Cd)); return ABOPT_EWORKSPACE; }

    ForwardQuery q;
    if ((rc = forward_query(N, L, zg, e.ga, w->blocks, w->num_layers, pair_bias_cache, pair_terms, &q))) return rc;
    q.mix_frag = w->w_mix_frag && w->mix_table; q.heads_frag = w->w_heads_frag != nullptr; q.prmsd = has_prmsd;
    abopt_step_noise nz{};
    if (sc) {
        ABOPT_CHECK_ARG(sc->p_angstrom && sc->v_next && sc->p_next && sc->s_next, "eps_net_step: NULL argument");
        if ((rc = check_step_args(sc->sp, sc->noise, sc->igX, sc->igCdf, sc->bins, &nz))) return rc;
        q.step = true; q.ppl = sc->ppl != nullptr; q.carry_in = sc->carry_in != 0; q.carry_out = sc->carry_out != 0;
        q.context_unused = sc->context_unused != 0;
        q.query_row_tiles = sc->context_unused ? sc->query_row_tiles : 0;
    }
    const NetPlan plan = plan_network(q);

    // dpm_full.py:86  R = exp(v_t)   and   dpm_full.py:89  res_feat_mixer([res_feat | Embedding(s_t)])
    if (!plan.mixer_launch) {
        // carried in: the fused tail of the previous step wrote x, its terms and R for exactly this state into this workspace
    } else if (plan.mixer_kernel) {
        if ((rc = launch_mixer(res_feat, s_t, w->w_mix_frag, w->mix_table, w->b_mix1, e.cat, M, st, v_t, e.R, plan.mixer_xt >= 0 ? e.ga.xt[plan.mixer_xt] : nullptr))) return rc;       // one launch for both
    } else {
        if ((rc = launch_so3_exp(v_t, e.R, M, st))) return rc;
        if ((rc = launch_embed_concat(res_feat, s_t, w->seq_embed, e.cat, M, st))) return rc;
        if ((rc = launch_linear(e.cat, 2 * F, w->w_mix0, 2 * F, w->b_mix0, e.x0, F, (int)M, F, 2 * F, true, st))) return rc;
        if ((rc = launch_linear(e.x0, F, w->w_mix1, F, w->b_mix1, e.cat, F, (int)M, F, F, false, st))) return rc;   // reuse cat[:, :F] as x (ld = F)
    }
    // dpm_full.py:90  encoder
    BlockArgs ba{e.R, p_t, e.cat, pair_feat, mask_res, e.xe, pair_bias_cache, pair_terms};
    ba.query_rows = mask_generate;                                          // read where the plan masks the last block's query rows (a step that says context_unused)
    ba.query_row_list = sc ? sc->query_row_list : nullptr;                  // ... and where it gathers them
    if ((rc = ga_encoder(plan.enc, q, w->blocks, ba, e.ga, e.pong, st))) return rc;
    // dpm_full.py:92-93 time features (the heads kernel takes them as an affine term: then only the prmsd head's LayerNorm'd copy is needed)
    if (plan.build_infeat && (rc = launch_build_infeat(e.xe, beta, e.infeat, w->prmsd_ln_gamma, w->prmsd_ln_beta, plan.prmsd ? e.infeat_ln : nullptr, N, L, st))) return rc;
    if (plan.step_fused) {
        // the heads, their epilogue, the step's transitions and (carry) the next evaluation's mixer in one launch (heads.hip: step_tail_kernel)
        const HeadsEpilogue hep{e.R, v_t, mask_generate, v_next, R_next, eps_pos, c_denoised, grad_mode, nonfinite_flag_ptr()};
        StepTail tl{*sc->sp, nz, sc->seed, sc->offset, sc->seed_dev, sc->p_angstrom, s_t, sc->aa_allowed, sc->igX, sc->igCdf, sc->bins,
                    sc->v_next, sc->p_next, sc->s_next, sc->post_out, sc->p_next_norm, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        if (plan.step_carry) {
            tl.res_feat = res_feat; tl.mix_wfrag = w->w_mix_frag; tl.mix_table = w->mix_table; tl.mix_b1 = w->b_mix1;
            tl.x_out = e.cat; tl.R_out = e.R; tl.xt_out = plan.mixer_xt >= 0 ? e.ga.xt[plan.mixer_xt] : nullptr;
        }
        return launch_step_tail(e.xe, beta, w->w_heads_frag, w->w_head1, FI, w->b_head1, w->b_crd2, w->b_rot2, w->b_seq2, w->b_crd3, w->b_rot3, w->b_seq3, e.out3, M, L,
                                st, hep, tl);
    }
    if (plan.heads_kernel) {
        // dpm_full.py:92-101: time features + the three heads in one launch (heads.hip) and, unless ABOPT_FUSE_HEADS=0 (A/B, tests), their geometric epilogue as its tail
        const HeadsEpilogue hep{e.R, v_t, mask_generate, v_next, R_next, eps_pos, c_denoised, grad_mode, nonfinite_flag_ptr()};
        if ((rc = launch_heads_mlp(e.xe, beta, w->w_heads_frag, w->w_head1, FI, w->b_head1, w->b_crd2, w->b_rot2, w->b_seq2, w->b_crd3, w->b_rot3,
                                   w->b_seq3, e.out3, M, L, st, plan.heads_epilogue ? &hep : nullptr))) return rc;
    } else {
    // three heads, first layers fused (shared input): [M,132] x [384,132]^T
    if ((rc = launch_linear(e.infeat, FI, w->w_head1, FI, w->b_head1, e.hh1, 3 * F, (int)M, 3 * F, FI, true, st))) return rc;
    if ((rc = launch_linear(e.hh1 + 0 * F, 3 * F, w->w_crd2, F, w->b_crd2, e.hh2 + 0 * F, 3 * F, (int)M, F, F, true, st))) return rc;
    if ((rc = launch_linear(e.hh1 + 1 * F, 3 * F, w->w_rot2, F, w->b_rot2, e.hh2 + 1 * F, 3 * F, (int)M, F, F, true, st))) return rc;
    if ((rc = launch_linear(e.hh1 + 2 * F, 3 * F, w->w_seq2, F, w->b_seq2, e.hh2 + 2 * F, 3 * F, (int)M, F, F, true, st))) return rc;
    // third layers into out3 [M,32]: cols 0..2 crd, 4..6 rot, 8..27 seq logits
    if ((rc = launch_linear(e.hh2 + 0 * F, 3 * F, w->w_crd3, F, w->b_crd3, e.out3 + 0, 32, (int)M, 3, F, false, st))) return rc;
    if ((rc = launch_linear(e.hh2 + 1 * F, 3 * F, w->w_rot3, F, w->b_rot3, e.out3 + 4, 32, (int)M, 3, F, false, st))) return rc;
    if ((rc = launch_linear(e.hh2 + 2 * F, 3 * F, w->w_seq3, F, w->b_seq3, e.out3 + 8, 32, (int)M, ABOPT_AA, F, false, st))) return rc;
    }
    if (!plan.heads_epilogue && (rc = launch_heads_epilogue(e.R, v_t, e.out3 + 0, e.out3 + 4, e.out3 + 8, 32, 32, mask_generate, v_next, R_next, eps_pos, c_denoised,
                                                            M, grad_mode, st))) return rc;
    if (plan.prmsd) {
        // PerResiduePredictor (nn.py:179-188) then mean over L (dpm_full.py:109-110)
        if ((rc = launch_linear(e.infeat_ln, FI, w->w_prmsd1, FI, w->b_prmsd1, e.pr1, F, (int)M, F, FI, true, st))) return rc;
        if ((rc = launch_linear(e.pr1, F, w->w_prmsd2, F, w->b_prmsd2, e.pr2, F, (int)M, F, F, true, st))) return rc;
        if ((rc = launch_linear(e.pr2, F, w->w_prmsd3, F, w->b_prmsd3, e.pr3, w->num_bins, (int)M, w->num_bins, F, false, st))) return rc;
        if ((rc = launch_mean_over_L(e.pr3, prmsd_logits, N, L, w->num_bins, st))) return rc;
    }
    if (!sc) return ABOPT_OK;
    return abopt_denoise_step(sc->sp, sc->noise, sc->seed, sc->offset, v_t, sc->p_angstrom, s_t, v_next, eps_pos, c_denoised, prmsd_logits, mask_generate, sc->igX, sc->igCdf,
                              sc->bins, sc->num_bins, sc->v_next, sc->p_next, sc->s_next, sc->prmsd, sc->ppl, sc->post_out, sc->p_next_norm, sc->seed_dev, sc->aa_allowed,
                              N, L, stream);
}

extern "C" int abopt_eps_net_forward(const abopt_eps_weights* w, const float* v_t, const float* p_t, const int64_t* s_t,
                                     const float* res_feat, const float* pair_feat, const float* beta,
                                     const uint8_t* mask_generate, const uint8_t* mask_res,
                                     float* v_next, float* R_next, float* eps_pos, float* c_denoised, float* prmsd_logits,
                                     int N, int L, int Fd, int Cd, int grad_mode, const float* pair_bias_cache, int pair_feat_shared,
                                     const float* pair_terms, void* ws, size_t ws_bytes, abopt_stream stream) {
    return eps_forward(w, v_t, p_t, s_t, res_feat, pair_feat, beta, mask_generate, mask_res, v_next, R_next, eps_pos, c_denoised, prmsd_logits, N, L, Fd, Cd, grad_mode,
                       pair_bias_cache, pair_feat_shared, pair_terms, ws, ws_bytes, stream, nullptr);
}

extern "C" int abopt_query_row_list(const uint8_t* mask_generate, int N, int L, void* rows, void* count, abopt_stream stream) {
    ABOPT_CHECK_ARG(N >= 0 && L >= 0 && (int64_t)N * (L + 15) < (1ll << 31), "query_row_list: bad dims N=%d L=%d", N, L);
    if (N == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(mask_generate && rows && count, "query_row_list: NULL argument");
    return launch_query_row_list(mask_generate, N, L, (int32_t*)rows, (int32_t*)count, (hipStream_t)stream);
}

extern "C" int abopt_eps_net_step(const abopt_eps_weights* w, const float* v_t, const float* p_t, const int64_t* s_t,
                                  const float* res_feat, const float* pair_feat, const float* beta,
                                  const uint8_t* mask_generate, const uint8_t* mask_res,
                                  float* v_net, float* R_net, float* eps_pos, float* c_denoised, float* prmsd_logits,
                                  int N, int L, int Fd, int Cd, const float* pair_bias_cache, int pair_feat_shared,
                                  const float* pair_terms, void* ws, size_t ws_bytes,
                                  const abopt_step_params* sp, const abopt_step_noise* noise, uint64_t seed, uint64_t offset, const float* p_angstrom,
                                  const float* igso3_X, const float* igso3_cdf, int igso3_bins, int num_bins,
                                  float* v_next, float* p_next, int64_t* s_next, float* prmsd, float* perplexity, float* post_out, float* p_next_norm,
                                  const uint64_t* seed_offset_dev, const int32_t* aa_allowed, int carry_in, int carry_out,
                                  int context_outputs_unused, const int32_t* query_rows, const int32_t* query_row_count, int query_row_tiles,
                                  abopt_stream stream) {
    ABOPT_CHECK_ARG(query_row_tiles >= 0 && (query_row_tiles == 0 || (query_rows && query_row_count)), "eps_net_step: %d tiles of a row list that is not given", query_row_tiles);
    const StepCall sc{sp, noise, seed, offset, p_angstrom, igso3_X, igso3_cdf, igso3_bins, num_bins, v_next, p_next, s_next, prmsd, perplexity, post_out, p_next_norm,
                      seed_offset_dev, aa_allowed, carry_in, carry_out, context_outputs_unused || query_row_tiles > 0, query_rows, query_row_tiles};
    return eps_forward(w, v_t, p_t, s_t, res_feat, pair_feat, beta, mask_generate, mask_res, v_net, R_net, eps_pos, c_denoised, prmsd_logits, N, L, Fd, Cd, 0,
                       pair_bias_cache, pair_feat_shared, pair_terms, ws, ws_bytes, stream, &sc);
}

// ---- lDDT-CA (kernels: lddt.hip).  Every check precedes the first launch.
extern "C" size_t abopt_lddt_ws_bytes(int G, int S, int L) { return lddt_ws_bytes(G, S, L); }

static int lddt_check(const char* name, bool ensemble, const void* pos, const void* mask, int G, int S, int L, int A, float cutoff, const void* num, const void* den,
                      const void* ws, size_t ws_bytes) {
    ABOPT_CHECK_ARG(G >= 0 && S >= 0 && L >= 1 && A >= 2 && (int64_t)G * S <= 0x7fffffff, "%s: bad dims G=%d S=%d L=%d A=%d (atom slot 1 is the CA: A >= 2)", name, G, S, L, A);
    ABOPT_CHECK_ARG(A <= 15, "%s: A=%d atoms per residue exceed the maximum of 15", name, A);
    ABOPT_CHECK_ARG(std::isfinite(cutoff) && cutoff > 0.f, "%s: the cutoff must be finite and > 0 (got %g)", name, (double)cutoff);
    if (L > 16384) { set_error("%s: L=%d residues exceed the maximum of 16384 (4 L^2 has to fit an int32)", name, L); return ABOPT_EUNSUPPORTED; }
    if (ensemble && S > 16384) { set_error("%s: S=%d candidates per group exceed the maximum of 16384", name, S); return ABOPT_EUNSUPPORTED; }
    ABOPT_CHECK_ARG(!ensemble || (int64_t)G * S * S <= 0x7fffffff, "%s: G S S = %lld entries exceed 2^31 - 1", name, (long long)G * S * S);
    if (G == 0 || S == 0) return ABOPT_OK;
    ABOPT_CHECK_ARG(G <= 65535, "%s: G=%d groups exceed one launch (max 65535)", name, G);
    ABOPT_CHECK_ARG(pos && mask && num && den && ws, "%s: NULL argument", name);
    ABOPT_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)num & 3) == 0 && ((uintptr_t)den & 3) == 0, "%s: the workspace must be 16-byte aligned, num and den 4-byte aligned", name);
    const size_t need = lddt_ws_bytes(G, S, L);
    if (ws_bytes < need) { set_error("%s: workspace too small (%zu bytes given, %zu needed)", name, ws_bytes, need); return ABOPT_EWORKSPACE; }
    return ABOPT_OK;
}

extern "C" int abopt_lddt_ca_grouped(const float* pos, const uint8_t* mask, int mask_shared, const float* ref_pos, const uint8_t* ref_mask, const uint8_t* rows,
                                     const int32_t* group, int G, int S, int L, int A, float cutoff, void* num, void* den, void* ws, size_t ws_bytes,
                                     abopt_stream stream) {
    const int rc = lddt_check("lddt_ca_grouped", false, pos, mask, G, S, L, A, cutoff, num, den, ws, ws_bytes);
    if (rc != ABOPT_OK || G == 0 || S == 0) return rc;
    ABOPT_CHECK_ARG(ref_pos && ref_mask, "lddt_ca_grouped: NULL argument");
    return launch_lddt(pos, mask, mask_shared, ref_pos, ref_mask, rows, group, G, S, L, A, cutoff, (int32_t*)num, (int32_t*)den, ws, (hipStream_t)stream);
}

extern "C" int abopt_lddt_ca_ensemble(const float* pos, const uint8_t* mask, int mask_shared, const uint8_t* rows, const int32_t* group, int G, int S, int L, int A,
                                      float cutoff, void* num, void* den, void* ws, size_t ws_bytes, abopt_stream stream) {
    const int rc = lddt_check("lddt_ca_ensemble", true, pos, mask, G, S, L, A, cutoff, num, den, ws, ws_bytes);
    if (rc != ABOPT_OK || G == 0 || S == 0) return rc;
    return launch_lddt(pos, mask, mask_shared, nullptr, nullptr, rows, group, G, S, L, A, cutoff, (int32_t*)num, (int32_t*)den, ws, (hipStream_t)stream);
}
