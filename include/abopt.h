/* abopt.h -- C ABI of libabopt_hip.so: the MI355X (gfx950) denoising hot path of
 * pengzhangzhi/ab_opt (AbDock / AbDesign).
 *
 * The reference is pure Python/PyTorch: it has no FFI of its own, so this is the boundary a
 * maintainer binds with ctypes under the reference's nn.Module methods (INTEGRATION.md shows the
 * stub).  Every entry point names the reference function(s) it replaces
 * (D/ = AbDock/src/, A/ = AbDesign/diffab/ in the reference tree).
 *
 * Conventions
 *   - plain C: device pointers + sizes, no torch types; all floating point is fp32, row-major,
 *     contiguous; masks are 1 byte per element (torch.bool storage); s_t / aa are int64.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); buffers are owned by
 *     the caller; `ws` is caller-owned scratch of at least the matching *_workspace_bytes().
 *   - no global mutable state: re-entrant across streams (one workspace per stream).
 *   - return 0 on success, else an ABOPT_E* code; abopt_last_error() gives the thread-local text.
 */
#ifndef ABOPT_H
#define ABOPT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ABOPT_ABI_VERSION 59

enum { ABOPT_OK = 0, ABOPT_EINVAL = 1, ABOPT_EHIP = 2, ABOPT_EUNSUPPORTED = 3, ABOPT_EWORKSPACE = 4 };

/* Fixed architecture of the IPA block (D/modules/encoders/ga.py:42-43 defaults, used by every shipped config). */
enum { ABOPT_HEADS = 12, ABOPT_QK_DIM = 32, ABOPT_POINTS = 8, ABOPT_AA = 20,
       ABOPT_NODE_PROJ = 2016,   /* 3*H*D + 3*H*P*3: query|key|value|query_pt|key_pt|value_pt */
       ABOPT_IPA_FEAT = 1824 };  /* H*C + H*D + H*P*(3+1+3) at C = 64 */

typedef void* abopt_stream;

int abopt_abi_version(void);
const char* abopt_last_error(void);
/* name/CU count/LDS bytes of the current HIP device; arch receives e.g. "gfx950". */
int abopt_device_info(int* cu_count, int* lds_bytes_per_cu, char* arch, int arch_len);

/* ---- SO(3) maps: D/modules/common/so3.py:33-57 (so3vec_to_rotation), :10-30,60-63 (rotation_to_so3vec).
 * w (n,3) <-> R (n,3,3).  grad_mode!=0 selects the reference's autograd-on cosine clamp (-0.999). */
int abopt_so3_exp(const float* w, float* R, int64_t n, abopt_stream stream);
int abopt_so3_log(const float* R, float* w, int64_t n, int grad_mode, abopt_stream stream);

/* ---- One GABlock: D/modules/encoders/ga.py:40-178.  Weight layouts are torch's ([out,in]). */
typedef struct {
    const float* w_node;        /* [2016, F]  rows: proj_query|proj_key|proj_value|proj_query_point|proj_key_point|proj_value_point (ga.py:54-66) */
    const float* w_pair_bias;   /* [12, C]    proj_pair_bias.weight (ga.py:59) */
    const float* spatial_coef;  /* [12]       raw parameter; softplus applied on device (ga.py:62-63,108) */
    const float* w_out;         /* [F, 1824]  out_transform.weight (ga.py:69-73) */
    const float* b_out;         /* [F] */
    const float* ln1_gamma; const float* ln1_beta;   /* layer_norm_1 (D/modules/common/layers.py:109-155) */
    const float* w_mlp0; const float* b_mlp0;        /* mlp_transition.0/.2/.4, each [F,F] + [F] (ga.py:76-78) */
    const float* w_mlp1; const float* b_mlp1;
    const float* w_mlp2; const float* b_mlp2;
    const float* ln2_gamma; const float* ln2_beta;
    const float* w_node_frag;   /* optional, abopt_node_frag_floats() floats = [12, 12, 4, 2, 64, 4] + {S, 1 / S, 0, 0}: w_node re-laid out per head in MFMA
                                   operand order, every weight as the two fp16 terms of S w (layout below); when given, the fused projection kernel
                                   replaces the GEMM + fragment pass (same results up to fp32 summation order) */
    const float* w_out_frag;    /* optional, 128 * 1824 4-byte words = [4 cb][114 s][2 terms][64 lanes] x 8 fp16: w_out in MFMA operand order as the two
                                   fp16 terms h = fp16(S w), l = fp16(S w - h) of [cb][s][lane = 32 kh + c][i] = w_out[32 cb + c][col(16 s + 8 kh + i)],
                                   S = the power of two with max |w_out| S in [2^14, 2^15) (stored in w_mlp_frag, below; the kernels multiply the
                                   sums by 1 / S; activations are split the same way in the kernels, three products per k-step: csrc/ipa_common.h,
                                   split_pair2).  col(k) = k for k >= 768; the 768 pair-feature columns
                                   (head h, channel ch) enter the K index at k = 192 ((ch % 16) / 4) + 16 h + 4 (ch / 16) + ch % 4 -- the order in
                                   which the fused core + tail kernel's lanes hold them (csrc/tail_common.h: ot_feat_col; abopt_pack_tail_weights
                                   produces this layout);
                                   when given together with w_mlp_frag, out_transform runs inside the LayerNorm/MLP kernel (no split-K partial slabs) */
    const float* w_mlp_frag;    /* optional, abopt_mlp_frag_floats() floats: w_mlp0, w_mlp1, w_mlp2 in 16x16x32 MFMA operand order as two fp16 terms of
                                   S_layer w: [layer][ct][s][term][lane = 16 kq + m] x 8 fp16, entry i = term(S w[16 ct + m][32 s + 8 kq + i])
                                   (3 * 128 * 128 words), then 8 floats {S_out, S_0, S_1, S_2, 1 / S_out, 1 / S_0, 1 / S_1, 1 / S_2}, then 256 floats of
                                   packer scratch; the rest of the buffer is zero */
    const float* w_out_terms;   /* optional, abopt_out_terms_floats() floats: a copy of w_out_frag (abopt_out_frag_terms; until ABI 38 the fused kernel
                                   streamed a different layout).  When given (with w_mlp_frag and a pair-bias cache), the IPA core and the tail of the
                                   block run as ONE kernel wherever the 32-row core applies: feat never leaves the chip (bit-identical results) */
} abopt_ga_weights;

/* Host-side description of the w_node_frag layout (used by the binding to pack weights once): for head h, tile T (0,1 q | 2,3 k |
 * 4,5 q_pts | 6,7 k_pts | 8,9 v | 10,11 v_pts), tile row m (0..15) -> source row of w_node, or -1 for a zero row.  Point tiles hold 4
 * points as (x, y, z, pad): m = 4 p + c.  A weight w is stored as two fp16 numbers h = fp16(S w), l = fp16(S w - h) (round to nearest), S the power
 * of two with max |w_node| S in [2^14, 2^15).  Element [h][T][s][term][lane = 16 kq + m] is a 16-byte vector of 8 fp16:
 * entry i = term(S w_node[row][32 s + 8 kq + i]), term 0 = h, 1 = l; the four floats behind the last element are {S, 1 / S, 0, 0}.
 * abopt_node_frag_floats() = size in 4-byte units. */
int abopt_node_frag_source_row(int h, int T, int m);
size_t abopt_node_frag_floats(void);

/* The tail of a GABlock on its own -- out_transform, mask, residual, LayerNorm, mlp_transition, LayerNorm
 * (AbDock/src/modules/encoders/ga.py:174-177; LayerNorm: AbDock/src/modules/common/layers.py:146-155) -- for hosts that drive the
 * block piecewise (the training path: forward with an activation dump, then the row-local part of its backward).
 *   abopt_pack_tail_weights  : w_out [128,1824], w_mlp0..2 [128,128] -> w_out_frag (abopt_out_frag_floats() floats), w_mlp_frag and
 *                              (optional) w_mlpT_frag = the three transposed layers (abopt_mlp_frag_floats() floats each), on the device.
 *   abopt_block_tail_forward : out [rows,128] = LN2(y + MLP(y)), y = LN1(x + mask * (feat W_out^T + b_out)).  saved (optional) receives
 *                              five [rows,128] slabs: x + mask*u | y | h0 = relu(W0 y + b0) | h1 = relu(W1 h0 + b1) | y + W2 h1 + b2.
 *   abopt_block_tail_backward: from d out and `saved`: dpre [3,rows,128] = d loss / d (pre-activation) of the three MLP layers (so
 *                              d W_l = dpre[l]^T . input_l), da1 [rows,128] = gradient reaching x through the residual,
 *                              du = mask * da1 (so d feat = du . W_out, d W_out = du^T . feat), and colpart [ceil(rows/32), 8, 128] =
 *                              per-tile column sums: 0 d ln2.beta | 1 d ln2.gamma | 2 d b_mlp2 | 3 d b_mlp1 | 4 d b_mlp0 | 5 d ln1.beta |
 *                              6 d ln1.gamma | 7 d b_out; the caller sums over tiles (deterministic). */
size_t abopt_out_frag_floats(void);
size_t abopt_heads_frag_floats(void);
size_t abopt_mixer_frag_floats(void);
size_t abopt_mlp_frag_floats(void);
size_t abopt_out_terms_floats(void);
/* w_out_frag (abopt_pack_tail_weights) -> w_out_terms: a copy since ABI 39 (both kernels stream the same pre-split layout). */
int abopt_out_frag_terms(const float* w_out_frag, float* w_out_terms, abopt_stream stream);
int abopt_pack_tail_weights(const float* w_out, const float* w_mlp0, const float* w_mlp1, const float* w_mlp2, float* w_out_frag,
                            float* w_mlp_frag, float* w_mlpT_frag, abopt_stream stream);
int abopt_block_tail_forward(const float* feat, const float* w_out_frag, const float* w_mlp_frag, const float* x, const float* b_out,
                             const uint8_t* mask, const float* ln1_gamma, const float* ln1_beta, const float* b_mlp0, const float* b_mlp1,
                             const float* b_mlp2, const float* ln2_gamma, const float* ln2_beta, float* out, float* saved, int64_t rows,
                             abopt_stream stream);
int abopt_block_tail_backward(const float* dout, const float* saved, const float* w_mlpT_frag, const uint8_t* mask, const float* ln1_gamma,
                              const float* ln2_gamma, float* dpre, float* da1, float* du, float* colpart, int64_t rows, abopt_stream stream);

/* Optional intermediates of one block for parity tests (any pointer may be NULL):
 * logits = (node+pair+spatial)*sqrt(1/3) before masking, alpha after softmax/masking: [N,L,L,12]; feat [N,L,1824]. */
typedef struct { float* logits; float* alpha; float* feat; } abopt_ga_debug;

size_t abopt_ga_workspace_bytes(int N, int L, int F, int C);

/* GABlock.forward (ga.py:149-178): R [N,L,3,3], t [N,L,3] (normalised coords), x [N,L,F], z [N,L,L,C],
 * mask [N,L] -> x_out [N,L,F].  F must be 128 and C 64 in this build (the only shipped shapes). */
int abopt_ga_block_forward(const abopt_ga_weights* w, const float* R, const float* t, const float* x,
                           const float* z, const uint8_t* mask, float* x_out, int N, int L, int F, int C,
                           const abopt_ga_debug* dbg, void* ws, size_t ws_bytes, abopt_stream stream);

/* The same block with what a sampling loop carries from call to call (ABI 41): this block's slice of abopt_pair_bias_cache and, optionally, the
 * abopt_pair_terms of the same z (pair_feat_shared as in abopt_eps_net_forward).  feat_out (optional, [N,L,1824]): the IPA features feeding
 * out_transform (ga.py:141-145) -- asking for them keeps the core and the tail as two launches (same results bit for bit). */
int abopt_ga_block_forward_cached(const abopt_ga_weights* w, const float* R, const float* t, const float* x,
                                  const float* z, const uint8_t* mask, float* x_out, int N, int L, int F, int C,
                                  const float* pair_bias_cache, const float* pair_terms, int pair_feat_shared, float* feat_out,
                                  void* ws, size_t ws_bytes, abopt_stream stream);

/* GAEncoder.forward (ga.py:181-193): num_layers blocks over the same R, t, z. */
int abopt_ga_encoder_forward(const abopt_ga_weights* blocks, int num_layers, const float* R, const float* t,
                             const float* x, const float* z, const uint8_t* mask, float* x_out,
                             int N, int L, int F, int C, void* ws, size_t ws_bytes, abopt_stream stream);

/* ---- EpsilonNet: D/modules/diffusion/dpm_full.py:35-112 (A/...:33-102 without the prmsd head).
 * Head weights are passed packed (see ab_opt_amd/hip.py: pack_eps_weights):
 *   w_head1 [384,132]: rows eps_crd_net.0 | eps_rot_net.0 | eps_seq_net.0, K padded 131->132 with a zero column
 *   w_head3_* keep torch shapes.  prmsd_* may be NULL (AbDesign). */
typedef struct {
    const float* seq_embed;                 /* [25, F]  current_sequence_embedding.weight */
    const float* w_mix0; const float* b_mix0;   /* [F, 2F], [F]   res_feat_mixer.0 */
    const float* w_mix1; const float* b_mix1;   /* [F, F],  [F]   res_feat_mixer.2 */
    const abopt_ga_weights* blocks; int num_layers;
    const float* w_head1; const float* b_head1;     /* [3F, F+4], [3F] */
    const float* w_crd2; const float* b_crd2; const float* w_crd3; const float* b_crd3;   /* [F,F],[F],[3,F],[3] */
    const float* w_rot2; const float* b_rot2; const float* w_rot3; const float* b_rot3;   /* [F,F],[F],[3,F],[3] */
    const float* w_seq2; const float* b_seq2; const float* w_seq3; const float* b_seq3;   /* [F,F],[F],[20,F],[20] */
    const float* prmsd_ln_gamma; const float* prmsd_ln_beta;      /* [F+3] */
    const float* w_prmsd1; const float* b_prmsd1;                 /* [F, F+4] (K padded), [F] */
    const float* w_prmsd2; const float* b_prmsd2;                 /* [F, F], [F] */
    const float* w_prmsd3; const float* b_prmsd3; int num_bins;   /* [num_bins, F], [num_bins] */
    const float* w_heads_frag;  /* optional, abopt_heads_frag_floats() floats = [27, 8, 2, 64, 4] + {S, 1 / S, 0, 0}: the heads' weights as two fp16 terms of S w in
                                   MFMA operand order (block layout of w_out_frag with one column block per entry: [block][s][term][lane = 32 kh + c] -> 8 fp16,
                                   entry i = term(S W[32 blk + c][16 s + 8 kh + i]), S one power of two for the whole buffer): blocks 0..11 = w_head1[:, :F]
                                   (crd | rot | seq first layers), 12..15 w_crd2, 16..19 w_rot2, 20..23 w_seq2, 24 w_crd3, 25 w_rot3, 26 w_seq3 (rows zero-padded to 32).
                                   When given, the three heads run as one kernel (time features enter as an affine term from w_head1[:, F:F+3]). */
    const float* w_mix_frag;    /* optional, abopt_mixer_frag_floats() floats = [8, 8, 2, 64, 4] + {S, 1 / S, 0, 0}: blocks 0..3 = w_mix0[:, :F], 4..7 = w_mix1, same
                                   layout; with mix_table the mixer is one kernel */
    const float* mix_table;     /* optional [25, F]: row s = w_mix0[:, F:] . seq_embed[s] + b_mix0 (the embedding half of the mixer's first layer) */
} abopt_eps_weights;

size_t abopt_eps_workspace_bytes(int N, int L, int F, int C);

/* Per-call pair-bias cache: proj_pair_bias(z) of EVERY block (ga.py:88-90) in one pass over pair_feat.  pair_feat and
 * the weights are constant over the steps of FullDPM.sample / optimize (dpm_full.py:274-283), so the sampler builds the
 * cache once per call and passes it to every abopt_eps_net_forward; the per-step kernel then skips that contraction
 * (bit-identical results).  cache: abopt_pair_bias_cache_bytes(N, L, num_layers) bytes, caller-owned.  The cache is an opaque operand of this library for exactly the
 * (N, L) batch it was built from (per block: chunk of 16 keys outermost, then the rows of the whole batch): it cannot be sliced per sample. */
size_t abopt_pair_bias_cache_bytes(int N, int L, int num_layers);
int abopt_pair_bias_cache(const abopt_ga_weights* blocks, int num_layers, const float* pair_feat, float* cache,
                          int N, int L, int C, abopt_stream stream);

/* Range guard (ABI 41).  The dense layers of abopt_eps_net_forward (node projections, out_transform + MLP, heads, mixer) multiply fp32 operands as two fp16
 * terms when the packed weights (w_node_frag, w_out_frag / w_out_terms, w_mlp_frag, w_heads_frag, w_mix_frag) are given: an activation beyond 65504 -- which
 * the fp32 reference handles -- becomes inf there and reaches the outputs as inf / NaN.  Every abopt_eps_net_forward raises a device flag when a head output
 * of any row is not finite; abopt_nonfinite_flag synchronises `stream`, returns the flag (1 / 0; -1 on error) and clears it if `reset`.  A caller that
 * sees 1 repeats the work with the packed-weight pointers set to NULL: the same layers then run as fp32 GEMMs with fp32's range (ab_opt_amd/dpm.py does,
 * once per sample() / optimize() call; tests/test_hip_parity.py::test_fp16_range_guard_falls_back_to_fp32_layers). */
int abopt_nonfinite_flag(int reset, abopt_stream stream);
/* The same flag cleared in stream order (ABI 43): a memset enqueued on `stream`, no copy to the host and no synchronisation.  A guarded call is
 *   abopt_nonfinite_flag_reset -> abopt_eps_net_forward ... -> abopt_nonfinite_flag(reset = 1)        (one synchronisation, after the work)
 * so a flag left up by earlier work on the stream is not taken for this call's.  abopt_nonfinite_flag itself synchronises and therefore must not be called while
 * `stream` is capturing: a caller that captures abopt_eps_net_forward in a graph of its own gets no fallback inside the graph (ab_opt_amd.modules.EpsilonNet.forward
 * then touches the flag neither before nor after) and reads abopt_nonfinite_flag after a replay -- a replay that produced a non-finite head output leaves it up
 * (tests/test_large_and_guard.py::test_eps_net_captured_in_a_user_graph_leaves_the_flag_to_the_caller). */
int abopt_nonfinite_flag_reset(abopt_stream stream);

/* Per-call pair terms (ABI 41): pair_feat re-laid as the fp16 operands of the pair aggregation sum_j alpha[i,j,h] z[i,j,:] (ga.py:114-118), built once per
 * FullDPM.sample / optimize call next to the bias cache (same constancy argument).  Every value becomes two fp16 terms h = fp16(S_i z), l = fp16(S_i z - h)
 * with one power of two S_ic per (query row, channel) (max_j |z[n,i,j,c]| S_ic in [2^13, 2^14)): 22 significant bits for every value within 2^-17 of the
 * largest of its (row, channel) column over the keys, the same 4 bytes per value; terms are packed along the contraction (key) index in the operand order of
 * v_mfma_f32_16x16x32_f16, the factors 2^-14 / S_ic follow them (the consuming kernel multiplies its probabilities by 2^14 before their split).
 * With the terms the 32-row block kernels run that aggregation on the fp16 matrix instructions (products exact, fp32 accumulation; error against the fp32
 * statement: that of fp32 accumulation itself, tests/test_hip_parity.py::test_pair_aggregation_on_fp16_terms_vs_fp64); without them (NULL) on the fp32 ones.
 * terms: abopt_pair_terms_bytes(N, L) bytes (< 4 GB), caller-owned; N = number of DISTINCT pair_feat entries (as for the bias cache); L <= 2048.  Opaque like the cache and
 * laid out over the whole batch ([chunk of 16 keys][row of the batch][4 KB]): not sliceable per sample. */
size_t abopt_pair_terms_bytes(int N, int L);
int abopt_pair_terms(const float* pair_feat, float* terms, int N, int L, int C, abopt_stream stream);
/* 1 if abopt_eps_net_forward(N samples, L residues, a bias cache, pair_feat_shared) would launch the kernels that read the terms on the current device
 * (the 32-row block kernels: shapes that fill the chip in whole rounds), 0 otherwise -- a caller need not build terms nobody reads. */
int abopt_pair_terms_used(int N, int L, int pair_feat_shared);

/* EpsilonNet.forward (dpm_full.py:70-112).  beta [N].  Outputs: v_next [N,L,3], R_next [N,L,3,3],
 * eps_pos [N,L,3], c_denoised [N,L,20], prmsd_logits [N,num_bins] (NULL when the head is absent). */
int abopt_eps_net_forward(const abopt_eps_weights* w, const float* v_t, const float* p_t, const int64_t* s_t,
                          const float* res_feat, const float* pair_feat, const float* beta,
                          const uint8_t* mask_generate, const uint8_t* mask_res,
                          float* v_next, float* R_next, float* eps_pos, float* c_denoised, float* prmsd_logits,
                          int N, int L, int F, int C, int grad_mode,
                          const float* pair_bias_cache /* NULL: compute the pair bias inside the step */,
                          int pair_feat_shared /* 0: pair_feat is [N,L,L,C].  1: pair_feat is [1,L,L,C] (and the cache was built with N = 1) and is
                                                  shared by all N samples -- the replicated-complex batches of the reference's runners,
                                                  D/tools/runner/design_for_pdb.py:141-147.  g > 1 (g divides N): pair_feat is [N/g,L,L,C] and
                                                  samples g c .. g c + g - 1 share entry c -- a test set of complexes x g samples in ONE launch
                                                  (D/tools/runner/design_for_testset.py:556-589; BASELINE config 4) */,
                          const float* pair_terms /* optional (needs pair_bias_cache): abopt_pair_terms of the same pair_feat */,
                          void* ws, size_t ws_bytes, abopt_stream stream);

/* ---- Per-step transitions: D/modules/diffusion/transition.py:42-50,80-101 (position), :146-160
 * (rotation), :202-245 (amino acid), D/modules/common/so3.py:111-146 (IGSO(3) draw),
 * dpm_full.py:284-300 (loop body after eps_net), :380-399 (perplexity), prmsd.py:31-47.
 * Schedule scalars of the step t -> t_prev.  For t_prev = t - 1 the host reads them from the var_sched buffers; for a longer stride of a respaced loop
 * (ABI 45) alpha_clamped, sigma, igso3_std and igso3_gaussian are those of the stride, the rest stay those of t: */
typedef struct {
    int   t;                 /* current step, T..1: the Philox tag of the step's draws */
    float alpha_clamped;     /* max(alphas[t], alphas[T-1])          transition.py:84-86 */
    float alpha_bar;         /* alpha_bars[t] */
    float sigma;             /* sigmas[t] */
    float sqrt_recip_abar;   /* sqrt_recip_alphas_cumprod[t]          transition.py:45 */
    float sqrt_recipm1_abar; /* sqrt_recipm1_alphas_cumprod[t]        transition.py:46 */
    float igso3_std;         /* angular_distrib_inv.stddevs[t] */
    int   igso3_gaussian;    /* angular_distrib_inv.approx_flag[t] */
    float position_scale;    /* FullDPM.position_scale (10.0) */
    float position_mean[3];
    int   pred_x0;           /* 1: eps_net output is x0 (AbDock obj=pred_x0), 0: it is the noise */
    int   sample_structure;  /* dpm_full.py:294-295 */
    int   sample_sequence;   /* dpm_full.py:296-297 */
    float dist_min, dist_max;/* prmsd bounds (prmsd.py:41) */
    int   ppl_masked;        /* 1: perplexity averaged over generated residues (sample, dpm_full.py:293); 0: over all L (optimize, :358) */
    int   t_prev;            /* the step this one lands on, t - 1 in the full loop: no noise is added when it is 0 (the reference's t > 1, transition.py:94-98,155) */
    int   tempered;          /* 0: the two fields below are not read; the step is that of every earlier ABI (so a zero-initialised tail keeps it).  ABI 55, see below */
    float seq_temperature;   /* tau >= 0: the temperature of the predicted residue-type distribution; 1 takes the untempered path, 0 is greedy */
    float noise_scale;       /* lambda >= 0: scales the structure noise of the step; 1 multiplies by 1 (exact), 0 makes the structure update deterministic */
} abopt_step_params;

/* Sampling at a temperature (ABI 55; no reference counterpart).  With tempered != 0:
 *   Residue types.  Where a row draws its type (mask_generate set, a non-empty allowed set A -- all 20 classes without aa_allowed) and tau != 1, the network's
 *     prediction c_net[0..19] of the row is replaced, BEFORE the posterior is formed, by its tempered form over A.  With m = max_{k in A} max(c_k, 0):
 *       e_k = exp2((log2(max(c_k, 0)) - log2(m)) / tau) for k in A, e_k = 0 outside A, c'_k = e_k / sum_j e_j;
 *       tau = 0: c' is one-hot at the lowest-index class of A with max(c_k, 0) == m;   m == 0 or not finite: c' = c (nothing to sharpen).
 *     Everything downstream is the untempered code on c': the products ((ab ct) + unif) ((ab c'_k) + unif), the aa_allowed zeroing, the normalisation, post_out,
 *     the perplexity term and the inverse-CDF walk -- so post_out and the perplexity describe the distribution that is sampled (a perplexity at tau != 1 is not
 *     comparable with one at tau = 1).  The temperature acts on the predicted x0 distribution, not on the posterior: the forward-noise term the network is
 *     conditioned on stays.  Context rows and frozen rows (an empty set) never read c_net for their posterior and still do not; an injected s_next is taken as
 *     it is, post_out is still the tempered posterior.  tau = 1 takes the untempered path verbatim.
 *   Structure.  The position update adds sigma_eff z with sigma_eff = the rounded fp32 product sigma * lambda; the rotation noise angle (either IGSO(3) branch,
 *     after the select) is multiplied by lambda before it scales the axis.  Injected structure noise is scaled likewise; the step that lands on 0 still adds
 *     nothing.  No random number is added or dropped: the Philox counter layout is that of every earlier ABI.
 * tau and lambda must be finite and >= 0, and a non-zero tau below 1e-3 is refused (1 / tau has to stay a sane fp32; 0 is the greedy limit): ABOPT_EINVAL. */

/* Explicit draws for teacher-forced replay, reference draw order; all NULL => the
 * device Philox stream (seed, offset) is used instead. */
typedef struct {
    const float*   axis;    /* [N,L,3]  randn  -> rotation axis before normalisation  (so3.py:143) */
    const int64_t* bin;     /* [N,L]    multinomial bin of the IGSO(3) histogram      (so3.py:122) */
    const float*   ubin;    /* [N,L]    rand   in-bin position                        (so3.py:125) */
    const float*   gauss;   /* [N,L]    randn  Gaussian branch                        (so3.py:130) */
    const float*   z;       /* [N,L,3]  randn  position noise                         (transition.py:94-98) */
    const int64_t* s_next;  /* [N,L]    the multinomial sample itself                 (transition.py:176-177) */
} abopt_step_noise;

/* Allowed residue types (ABI 44): the optional last data argument `aa_allowed` [N,L] of the three functions that draw a residue type
 * (abopt_denoise_step, abopt_sample_init, abopt_add_noise).  One int32 word per residue; bit k (0..19, the order ACDEFGHIKLMNPQRSTVWY of the
 * reference's AA enum, utils/protein/constants.py) set = type k may be drawn there; bits 20.. are ignored, so -1 means "all".  The word is read on
 * residues with mask_generate set and nowhere else: context residues behave as without the argument.  NULL = no constraint; a word with all of bits
 * 0..19 set is the same arithmetic in the same order, so NULL, 0xFFFFF and -1 give bit-identical outputs.
 *   abopt_denoise_step: a disallowed class leaves the posterior BEFORE it is normalised -- its unnormalised product
 *     ((ab ct) + unif) ((ab c_net) + unif) (transition.py:166-174) is replaced by 0, then post[k] = raw[k] / (sum + 1e-8) as ever -- so post_out and the
 *     perplexity term are those of the distribution that is sampled; the inverse-CDF walk over post[k] + 1e-8 skips disallowed classes and ends, when
 *     rounding leaves it short, on the last allowed one (class 19 without a constraint).
 *   abopt_sample_init: the initial type is uniform over the allowed types among 0..18 -- the (r % count)-th set bit for the random word r that
 *     is r % 19 without a constraint (randint_like(high=19) never draws TYR) -- and 19 where bit 19 alone is set.
 *   abopt_add_noise: the walk over c_t + 1e-8 skips disallowed classes and ends on the last allowed one; c_noisy stays the unconstrained c_t.
 * An injected draw (noise->s_next, sr, noise->s_noisy) is taken as it is.
 * A word with NONE of bits 0..19 set on a generated residue is defined: the residue's type is frozen -- s_next = s_t, s_init = s, s_noisy = s_0,
 * injected draws included -- its posterior is reported as onehot(s_t) like a context residue's (and enters the perplexity so), and its structure
 * still moves.  (The Python layer refuses such a word before any launch.) */

/* One loop iteration after eps_net: state (v_t, p_t in Angstrom, s_t) -> (v_next, p_next in Angstrom, s_next),
 * plus per-sample prmsd [N] and perplexity [N] (either may be NULL).
 * igso3_X / igso3_cdf: row t of the inverse-process histogram, [bins] bin starts and [bins-1] normalised CDF
 * (cdf only used without injected noise). post_out [N,L,20] optional (posterior, for tests).  p_next_norm [N,L,3] optional:
 * (p_next - position_mean) / position_scale, the normalised positions the next step's network call takes (dpm_full.py:276). */
int abopt_denoise_step(const abopt_step_params* sp, const abopt_step_noise* noise,
                       uint64_t seed, uint64_t offset,
                       const float* v_t, const float* p_t, const int64_t* s_t,
                       const float* v_net, const float* p_net, const float* c_net, const float* prmsd_logits,
                       const uint8_t* mask_generate,
                       const float* igso3_X, const float* igso3_cdf, int igso3_bins, int num_bins,
                       float* v_next, float* p_next, int64_t* s_next, float* prmsd, float* perplexity,
                       float* post_out, float* p_next_norm,
                       const uint64_t* seed_offset_dev /* optional DEVICE pointer to {seed, offset}: read by the kernel instead of the
                                                          two by-value arguments, so a captured hipGraph of the loop can be replayed
                                                          with a fresh stream position (the values are read at execution time) */,
                       const int32_t* aa_allowed /* optional [N,L]: allowed residue types, see above */,
                       int N, int L, abopt_stream stream);

/* The generated rows of every sample as a list (ABI 52): rows [N][ceil(L / 16) * 16] int32 takes, per sample, the ascending indices of the residues with
 * mask_generate != 0 and -1 in every entry behind them; count [N] int32 takes their number.  One launch; the host learns nothing. */
int abopt_query_row_list(const uint8_t* mask_generate, int N, int L, void* rows, void* count, abopt_stream stream);

/* One whole loop iteration (ABI 46; one entry for all its forms since ABI 53): abopt_eps_net_forward (grad_mode 0) followed by abopt_denoise_step on its outputs, as
 * one call.  The arguments are those of the two functions, once each: v_t / s_t / mask_generate / N / L / stream are shared, p_t is the normalised position the
 * network takes and p_angstrom the state the step moves, v_net / R_net / eps_pos / c_denoised / prmsd_logits are the network's outputs (written as by
 * abopt_eps_net_forward, read as the step's v_net / p_net / c_net / prmsd_logits).  p_next_norm may be p_t itself.
 * The plain call -- context_outputs_unused = 0, query_row_tiles = 0; query_rows and query_row_count may be NULL: every output is bit-identical to the two calls in a row.
 * Where the packed mixer and heads operands are given, neither prmsd nor perplexity is asked for (no prmsd head in w, perplexity NULL) and ABOPT_FUSE_STEP is not 0,
 * the heads, the step's transitions and -- carry_out -- the mixer step of the NEXT evaluation on the state just sampled run as ONE launch behind the encoder;
 * otherwise the call makes the launches of the two functions, in their order, and ignores the carry.
 *   carry_out != 0: also leave the next evaluation's mixer output (for v_next / s_next and the same res_feat) in ws.
 *   carry_in  != 0: ws already holds this evaluation's mixer output -- the previous call of this function, with carry_out set, on the same ws, N, L, w and res_feat,
 *                   produced exactly this v_t / s_t, and nothing wrote ws in between.  The mixer launch is skipped.
 * Two optional facts a loop may add; neither changes what the step hands on:
 *   context_outputs_unused != 0 (ABI 50): the caller reads the network's outputs on generated residues only.  v_next, p_next, s_next, post_out and p_next_norm are
 *     still bit-identical to the plain call's -- the transitions keep the old state wherever mask_generate is 0, whatever the network says there -- and so are v_net,
 *     R_net, eps_pos and c_denoised on residues with mask_generate set; on the other residues those four are finite but unspecified, and abopt_nonfinite_flag does not
 *     rise because of them.  What the library does with the freedom: where the step's tail is fused (see above: packed operands, no prmsd head, perplexity NULL) and
 *     the last block of the encoder is the fused 32-row kernel on a pair-bias cache, that block streams pair features and pair bias for generated query rows only.
 *     Every other call runs exactly as the plain call does; ABOPT_STEP_ROWS=0 makes all do.
 *   query_row_tiles > 0 (ABI 52): the caller also holds the row list of its mask_generate.  query_rows and query_row_count, both required then, are what
 *     abopt_query_row_list wrote for THIS mask_generate, N and L, and query_row_tiles >= ceil(max_n count[n] / 16) is the number of 16-row tiles of the list the longest
 *     sample fills (the caller reads the counts once per loop; masks do not change over its steps).  A row list implies the caller's word: context outputs are unused
 *     whatever context_outputs_unused says, and the contract is that of the flag -- v_next, p_next, s_next, post_out and p_next_norm bit-identical everywhere, v_net,
 *     R_net, eps_pos and c_denoised bit-identical on generated residues, finite but unspecified on the others.  What the library does with the list: where the flag
 *     alone would mask the last block's query rows, the net has three blocks or more, N * query_row_tiles workgroups fit the device's CUs in one round and
 *     query_row_tiles <= ceil(L / 32), that block runs one workgroup per 16 LISTED rows instead of one per 32 rows of the sample.  Every other call makes the launches
 *     of the flag alone; ABOPT_STEP_COMPACT=0 makes all do.  A list that does not belong to mask_generate, or fewer tiles than the longest sample fills, leaves
 *     generated rows of the network's outputs unspecified.  query_row_tiles = 0: no list, the pointers are not read. */
int abopt_eps_net_step(const abopt_eps_weights* w, const float* v_t, const float* p_t, const int64_t* s_t,
                       const float* res_feat, const float* pair_feat, const float* beta,
                       const uint8_t* mask_generate, const uint8_t* mask_res,
                       float* v_net, float* R_net, float* eps_pos, float* c_denoised, float* prmsd_logits,
                       int N, int L, int F, int C,
                       const float* pair_bias_cache, int pair_feat_shared, const float* pair_terms, void* ws, size_t ws_bytes,
                       const abopt_step_params* sp, const abopt_step_noise* noise, uint64_t seed, uint64_t offset, const float* p_angstrom,
                       const float* igso3_X, const float* igso3_cdf, int igso3_bins, int num_bins,
                       float* v_next, float* p_next, int64_t* s_next, float* prmsd, float* perplexity, float* post_out, float* p_next_norm,
                       const uint64_t* seed_offset_dev, const int32_t* aa_allowed, int carry_in, int carry_out,
                       int context_outputs_unused, const int32_t* query_rows, const int32_t* query_row_count, int query_row_tiles,
                       abopt_stream stream);

/* ---- IGSO(3) angle histograms for arbitrary standard deviations (ABI 45): the tables ApproxAngularDistribution builds on the host at construction
 * (D/modules/common/so3.py:82-109), for the strides of a respaced loop, whose sigmas are chosen per call.  Row r, bin b at x_b = linspace(0, pi, bins)[b]:
 *   Y[r,b] = max(0, nan_to_num(sum_{l < iters} c a_l b_l)),  c = (1 - cos x) / pi,  a_l = (2 l + 1) exp(-l (l + 1) std_r^2),
 *   b_l = (sin((l + 1/2) x) + 1e-6) / (sin(x / 2) + 1e-6)
 * with every factor evaluated in fp32 as the host builder does and the products summed over l in fp64 (one rounding to fp32 at the end);
 * cdf[r,:] = cumsum(Y[r,:bins-1]) / sum(Y[r,:bins-1]) in fp64, rounded to fp32 (an all-zero row is divided by 1): what multinomial(Y[:, :-1]) samples.
 * stddevs [rows] (device), X [rows,bins] (every row linspace(0, pi, bins); may be NULL), Y [rows,bins], cdf [rows,bins-1].  bins >= 2, iters >= 1. */
int abopt_igso3_tables(const float* stddevs, int rows, int bins, int iters, float* X, float* Y, float* cdf, abopt_stream stream);

/* Initial state of FullDPM.sample (dpm_full.py:255-269): q4 [N,L,4], pn [N,L,3], sr [N,L] are the
 * reference's three draws (NULL => Philox).  p in/out in Angstrom.  position_mean is a HOST pointer to 3 floats. */
int abopt_sample_init(const float* v, const float* p, const int64_t* s, const uint8_t* mask_generate,
                      const float* q4, const float* pn, const int64_t* sr, uint64_t seed, uint64_t offset,
                      float position_scale, const float* position_mean, int sample_structure, int sample_sequence,
                      float* v_init, float* p_init, int64_t* s_init,
                      const int32_t* aa_allowed /* optional [N,L]: allowed residue types, see above abopt_denoise_step */,
                      int N, int L, abopt_stream stream);

/* ---- Forward noising: RotationTransition.add_noise (D/modules/diffusion/transition.py:120-144), PositionTransition.add_noise
 * (:62-78), AminoacidCategoricalTransition.add_noise (:179-200); used by FullDPM.optimize (dpm_full.py:320-339) and by the
 * training loss (dpm_full.py:162-178).  t [N] is per sample; alpha_bars/fwd_* are the schedule buffers ([T+1], [T+1,bins]);
 * fwd_cdf [T+1,bins-1] only for the device-RNG path.  p_0 / p_noisy in Angstrom.  noise: reference draw order
 * randn(N,L,3) axis, multinomial bin, rand ubin, randn gauss | randn(N,L,3) pos | multinomial s_noisy; all NULL => Philox.
 * With noise_structure = 0 (train_structure / sample_structure = False: dpm_full.py:169-173 draws nothing for the structure)
 * s_noisy alone may be injected.
 * c_noisy (optional, [N,L,20]): the categorical c_t the sequence sample is drawn from (transition.py:196-198), whether or not
 * the sample itself is injected; with noise_sequence = 0 it is onehot(s_0), the reference's c_0 (all-zero rows for s_0 outside 0..19). */
typedef struct {
    const float* axis; const int64_t* bin; const float* ubin; const float* gauss;   /* rotation (so3.py:141-146) */
    const float* pos;                                                               /* e_rand (transition.py:75) */
    const int64_t* s_noisy;                                                         /* the categorical sample itself */
} abopt_addnoise_noise;

int abopt_add_noise(const int64_t* t, const float* alpha_bars, const float* fwd_stddevs, const uint8_t* fwd_approx,
                    const float* fwd_X, const float* fwd_cdf, int bins, int num_sched,
                    const abopt_addnoise_noise* noise, uint64_t seed, uint64_t offset,
                    const float* v_0, const float* p_0, const int64_t* s_0, const uint8_t* mask_generate,
                    float position_scale, const float* position_mean, int noise_structure, int noise_sequence, int grad_mode,
                    float* v_noisy, float* p_noisy, int64_t* s_noisy, float* eps_p, float* c_noisy,
                    const uint64_t* seed_offset_dev /* optional device {seed, offset}, as in abopt_denoise_step */,
                    const int32_t* aa_allowed /* optional [N,L]: allowed residue types, see above abopt_denoise_step; the training loss passes NULL */,
                    int N, int L, abopt_stream stream);

/* ---- DockQ scoring of docked candidates: D/tools/runner/design_for_pdb.py:316-321 calls calc_DockQ(model, native, use_CA_only=True)
 * (AbDock/DockQ/DockQ.py:98-385) per candidate, which runs the `fnat` program twice (DockQ/src/fnat.c:100-252: residue contacts over
 * all heavy atoms, 5 A for Fnat, 10 A for the interface) and superimposes CA atoms twice (interface -> iRMS; receptor -> LRMS).
 * Structures are tensors with the batch's residue indexing: pos [L,A,3] Angstrom, mask [L,A], group [L] (0 = not in the file,
 * 1 / 2 = the two chains); atom slot 1 = CA.  model_pos [S,L,A,3]; model_mask [S,L,A], or [L,A] with model_mask_shared = 1.
 * out [S,4] = (fnat, irms, Lrms, DockQ).  ws: abopt_dockq_workspace_bytes(L).  S >= 0, L >= 1 with L * L <= INT_MAX (the contact table is
 * indexed with an int; L = 46341 is refused with ABOPT_EINVAL, as by the grouped entry), A >= 2.
 * A candidate whose interface, receptor or ligand has NO CA atom present in both model and native has no superposition: its irms /
 * Lrms (and DockQ) come back as -1 (the reference asserts on such inputs); with 1 or 2 common atoms the fit is degenerate but defined. */
size_t abopt_dockq_workspace_bytes(int L);
int abopt_dockq_lite(const float* model_pos, const uint8_t* model_mask, int model_mask_shared, const float* native_pos,
                     const uint8_t* native_mask, const int32_t* group, int S, int L, int A, float* out,
                     void* ws, size_t ws_bytes, abopt_stream stream);

/* The same scoring for G natives at once (ABI 42): the re-dock screen of AbDock/optimize_ab.py:73-98 (dock_seqs) scores the D re-docks of
 * EVERY design against that design's own complex (design_for_pdb.py:311-321), one calc_DockQ per candidate.  native_pos [G,L,A,3],
 * native_mask [G,L,A], group [G,L]; model_pos [G*S,L,A,3], candidate c scored against native c / S; model_mask [G*S,L,A], or [G,L,A]
 * (one mask per native) with model_mask_shared = 1.  out [G*S,4] as abopt_dockq_lite, -1 markers included; every row is bit-identical
 * to abopt_dockq_lite called on its group alone.  ws: abopt_dockq_grouped_workspace_bytes(G, L). */
size_t abopt_dockq_grouped_workspace_bytes(int G, int L);
int abopt_dockq_lite_grouped(const float* model_pos, const uint8_t* model_mask, int model_mask_shared, const float* native_pos,
                             const uint8_t* native_mask, const int32_t* group, int G, int S, int L, int A, float* out,
                             void* ws, size_t ws_bytes, abopt_stream stream);

/* ---- Batched-sampling reduction: D/tools/runner/design_for_testset.py:556-589 (calc_per_rmsd +
 * rank_commoness score).  structs [B,n,3] -> score [B] = mean_{b'} RMSD(b,b') * B/(B-1). */
/* ---- Training side of the IPA core (FullDPM.forward, D/modules/diffusion/dpm_full.py:156-234; the autograd of
 * GABlock.forward, ga.py:81-147).  The host keeps the dense projections, LayerNorm/MLP and losses in its autograd graph
 * (library GEMMs) and calls these two for the part that streams pair_feat:
 *   forward : proj_local [N,L,2016] = x . [Wq|Wk|Wv|Wqp|Wkp|Wvp]^T (points still in the residue frames)
 *             -> feat [N,L,1824] (the input of out_transform, ga.py:174) and alpha (ga.py:166) HEAD-MAJOR [N,12,L,L]
 *   backward: g [N,12,L,L] = d loss / d logits (after the sqrt(1/3) scale) and dpair_feat [N,L,L,C] of this block, from
 *             alpha, dalpha_node[n,h,i,j] = <dfeat_node_ih, v_jh> + <dagg_pts_ih, v_pts_jh>, delta[n,i,h] = sum_j alpha dalpha,
 *             dfeat (its first 12*C columns are d feat_p2n, row stride ld_dfeat) and proj_pair_bias.weight. */
size_t abopt_ipa_train_workspace_bytes(int N, int L);
int abopt_ipa_core_train_forward(const float* proj_local, const float* R, const float* t, const float* pair_feat, const uint8_t* mask,
                                 const float* w_pair_bias, const float* spatial_coef,
                                 const float* pair_bias_cache /* optional: this block's slice of abopt_pair_bias_cache built from the same pair_feat and weights */,
                                 float* feat, float* alpha, int N, int L, int C, void* ws, size_t ws_bytes, abopt_stream stream);
/* prologue of the backward: the points epilogue (ga.py:133-139) differentiated, d feat_node re-laid out head-major next to
 * it (dout_cat [N,12,L,32+24]) and delta [N,L,12] = sum_j alpha dalpha (see above). */
int abopt_ipa_points_backward(const float* dfeat, int ld_dfeat, const float* feat, const float* R, const float* t,
                              float* dout_cat, float* delta, int N, int L, abopt_stream stream);
/* head-major operands of the backward's batched GEMMs: Aq/Ak [N,12,L,57] = [q|k (32) | points in the global frame (24) | 1],
 * Av [N,12,L,56] = [v | v points]; and the final assembly of d proj_local [N,L,2016] (+ e [N,L,12], whose sum over (N, L) is
 * d loss / d spatial_coef: the chain through -softplus(.) sqrt(2/(9P))/2 is applied in the kernel) from P1 = g Ak, P2 = g^T Aq, P3 = alpha^T dout_cat. */
int abopt_ipa_backward_operands(const float* proj_local, const float* R, const float* t, float* Aq, float* Ak, float* Av,
                                int N, int L, abopt_stream stream);
int abopt_ipa_backward_assemble(const float* P1, const float* P2, const float* P3, const float* Aq, const float* Ak, const float* R,
                                const float* spatial_coef, float* dproj, float* e, int N, int L, abopt_stream stream);
int abopt_ipa_pair_backward(const float* pair_feat, const float* alpha, const float* dalpha_node, const float* delta,
                            const float* dfeat, int ld_dfeat, const float* w_pair_bias, float* g, float* dpair_feat /* may be NULL: see abopt_ipa_dz_assemble */,
                            float* dw_pair_bias_rows /* [N*L, 12*C]: per-query-row partials of d proj_pair_bias.weight (sum over rows) */,
                            int dpair_feat_accumulate /* 1: dpair_feat += this block's gradient (the six blocks of the encoder share one
                                                         buffer instead of six 268 MB tensors that autograd adds up); 0: overwrite */,
                            int N, int L, int C, abopt_stream stream);

/* d pair_feat of ALL blocks of an encoder in one pass: dpair_feat[n,i,j,c] = sum over blocks l and heads h of
 * alpha_l[n,h,i,j] dfeat_l[n,i,h*C+c] + g_l[n,h,i,j] w_pair_bias_l[h,c] (the pair-aggregation and proj_pair_bias terms of ga.py:88-90,114-118
 * differentiated), from what abopt_ipa_pair_backward(..., dpair_feat = NULL, ...) of every block left behind.  No z read and ONE write of
 * d pair_feat instead of a read-modify-write per block.  alpha / g / dfeat / w_pair_bias: HOST arrays of num_blocks (<= 6) device pointers. */
int abopt_ipa_dz_assemble(int num_blocks, const float* const* alpha, const float* const* g, const float* const* dfeat, int ld_dfeat,
                          const float* const* w_pair_bias, float* dpair_feat, int N, int L, int C, abopt_stream stream);

/* ---- encode(): D/models/diffab.py:39-83.  ResidueEmbedding.forward (D/modules/encoders/residue.py:26-92; the AbDesign
 * variant adds hotspot_embed, A/modules/encoders/residue.py:19-21), PairEmbedding.forward (D/modules/encoders/pair.py:37-101),
 * construct_3d_basis (D/modules/common/geometry.py:47-69).  Feature widths are fixed: res_feat_dim 128, pair_feat_dim 64,
 * max_aa_types 22, max_relpos 32. */
typedef struct {
    int N, L;
    int atoms_in;                    /* atoms per residue in pos_atoms / mask_atoms (15) */
    int atoms;                       /* atoms the embeddings use: 15 ('full') or 5 ('backbone+CB'), D/models/diffab.py:13-16 */
    const int64_t* aa;               /* [N,L] */
    const int64_t* res_nb;           /* [N,L] */
    const int64_t* chain_nb;         /* [N,L] */
    const int64_t* fragment_type;    /* [N,L]  (residue embedding only) */
    const int64_t* hotspot;          /* [N,L] or NULL -> zeros (AbDesign residue embedding only) */
    const float*   pos_atoms;        /* [N,L,atoms_in,3] Angstrom */
    const uint8_t* mask_atoms;       /* [N,L,atoms_in] */
    const uint8_t* structure_mask;   /* [N,L] or NULL (diffab.py:47-55) */
    const uint8_t* sequence_mask;    /* [N,L] or NULL */
} abopt_encode_inputs;

typedef struct {
    const float* aatype_embed;       /* [22, 128] */
    const float* type_embed;         /* [10, 128] */
    const float* hotspot_embed;      /* [10, 128] or NULL (AbDock) */
    const float* freq_bands;         /* [6] dihed_embed.freq_bands */
    const float* w0; const float* b0;/* mlp.0 [256, in], in = 128 + 22*atoms*3 + 39 + 128 (+128 with hotspot) */
    const float* w1; const float* b1;/* mlp.2 [128, 256] */
    const float* w2; const float* b2;/* mlp.4 [128, 128] */
    const float* w3; const float* b3;/* mlp.6 [128, 128] */
} abopt_residue_embed_weights;

typedef struct {
    const float* aa_pair_embed;      /* [484, 64] */
    const float* relpos_embed;       /* [65, 64] */
    const float* aapair_to_distcoef; /* [484, atoms*atoms] */
    const float* freq_bands;         /* [6] dihedral_embed.freq_bands */
    const float* wd0; const float* bd0;   /* distance_embed.0 [64, atoms*atoms] */
    const float* wd1; const float* bd1;   /* distance_embed.2 [64, 64] */
    const float* wo0; const float* bo0;   /* out_mlp.0 [64, 218] */
    const float* wo1; const float* bo1;   /* out_mlp.2 [64, 64] */
    const float* wo2; const float* bo2;   /* out_mlp.4 [64, 64] */
} abopt_pair_embed_weights;

size_t abopt_residue_embed_workspace_bytes(int N, int L, int atoms, int hotspot);
/* -> res_feat [N,L,128]; R [N,L,3,3] = construct_3d_basis(CA, C, N); p [N,L,3] = CA (diffab.py:76-83) */
int abopt_residue_embed_forward(const abopt_encode_inputs* in, const abopt_residue_embed_weights* w, float* res_feat, float* R, float* p,
                                void* ws, size_t ws_bytes, abopt_stream stream);
/* Training path: the input features of the residue MLP on their own (residue.py:33-88: aa embedding | per-type local coordinates | dihedral
 * encoding | fragment-type embedding [| hotspot embedding]) -> features [N*L, ld], ld = in_dim rounded up to a multiple of 4
 * (in_dim = 128 + 22*atoms*3 + 39 + 128 [+ 128]); only the embedding tables and freq_bands of `w` are read.  R, p as in the fused forward. */
size_t abopt_residue_features_workspace_bytes(int N, int L);
int abopt_residue_features(const abopt_encode_inputs* in, const abopt_residue_embed_weights* w, float* features, float* R, float* p,
                           void* ws, size_t ws_bytes, abopt_stream stream);
size_t abopt_pair_embed_workspace_bytes(int N, int L, int atoms);
/* -> pair_feat [N,L,L,64].  activations: NULL for inference; for training a [N,L,L,ABOPT_PAIR_ACT] buffer that receives, per
 * pair, relu(distance_embed.0) (64) | f_dist = relu(distance_embed.2) x structure mask (64) | f_dih (26, padded to 32) |
 * relu(out_mlp.0) (64) | relu(out_mlp.2) (64): what the backward of the five linears needs (pair.py:74-99). */
enum { ABOPT_PAIR_ACT = 288 };
/* gauss / dgauss (training): [N,L,L,atoms,16] -- the Gaussian atom-pair features g (pair.py:62-73, atom b of residue j padded to 16)
 * and T = dg / d softplus(coef) = -d^2 g.  dgauss may be NULL with gauss given: the backward then recomputes T from the atoms (1 GB
 * less to write and to read back at N = 16, L = 256). */
int abopt_pair_embed_forward(const abopt_encode_inputs* in, const abopt_pair_embed_weights* w, float* pair_feat, float* activations,
                             float* gauss, float* dgauss, void* ws, size_t ws_bytes, abopt_stream stream);
/* Backward chain of the five linears for the training path: from dpair_feat [N,L,L,64] and the saved activations writes, per pair,
 * dys [N,L,L,ABOPT_PAIR_DY] = d loss / d pre-activation of out_mlp.4 | out_mlp.2 | out_mlp.0 | distance_embed.2 |
 * distance_embed.0 (64 each), and dsoftplus [N,L,L,atoms,16] = d loss / d softplus(aapair_to_distcoef) per atom pair.  The
 * weight gradients are tall GEMMs of dys against the activations (host side).  dgauss NULL: T is recomputed in the kernel with the
 * forward's arithmetic (same bits).  dys_colsum (optional, [ABOPT_PAIR_DY]): the column sums of dys = the five bias gradients, formed from
 * per-wave partial sums inside the kernel instead of a second pass over the 1.3 GB of dys. */
enum { ABOPT_PAIR_DY = 320 };
size_t abopt_pair_embed_backward_workspace_bytes(int N, int L, int atoms);
int abopt_pair_embed_backward(const abopt_encode_inputs* in, const abopt_pair_embed_weights* w, const float* dpair_feat,
                              const float* activations, const float* dgauss, float* dys, float* dsoftplus, float* dys_colsum,
                              void* ws, size_t ws_bytes, abopt_stream stream);

/* ---- Training path: the geometric epilogue of the heads on its own, D/modules/diffusion/dpm_full.py:95-101 (A: 86-92), and its backward.
 *   eps_pos = gen ? R eps_crd : 0;   R_next = R U(eps_rot) with U the rotation of the quaternion 1 + b i + c j + d k (geometry.py:215-233);
 *   v_next = gen ? log(R_next) : v_t  (optional: v_t / v_next may both be NULL -- the training losses do not use it).
 * eps_crd / eps_rot [rows,3] are the outputs of eps_crd_net / eps_rot_net; the backward takes d R_next [rows,3,3] and d eps_pos [rows,3]
 * (either may be NULL = zero) and writes d eps_crd, d eps_rot [rows,3].  In the reference these are ~45 elementwise ATen kernels forward
 * and ~90 backward per step. */
/* The three per-residue losses of FullDPM.forward and their gradients in one pass (D/modules/diffusion/dpm_full.py:199-231, A: 156-190):
 *   rot = sum_k 1 - cos(R_pred[:, k], R_0[:, k])  (rotation_matrix_cosine_loss, dpm_full.py:15-32);  pos = |p_pred - p_target|^2;
 *   seq = KL(posterior(s_t, s_0) || posterior(s_t, c_denoised))  (transition.py:217-229),  each summed over the generated residues.
 * block_sums [ceil(N L / 256)][3]: per-workgroup sums of (rot, pos, seq), to be added in order and divided by sum(mask_generate) + 1e-8;
 * dR_pred [N,L,3,3], dp_pred [N,L,3], dc_denoised [N,L,20]: d(sum)/d(input) per residue, zero outside mask_generate. */
int abopt_dpm_losses(const float* R_pred, const float* R_0, const float* p_pred, const float* p_target, const float* c_denoised, const int64_t* s_t,
                     const int64_t* s_0, const float* alpha_bar_t, const uint8_t* mask_generate, int N, int L, float* block_sums, float* dR_pred,
                     float* dp_pred, float* dc_denoised, abopt_stream stream);
/* The two losses only the AbDock flavour has, with their gradients, one workgroup per sample (D/modules/diffusion/dpm_full.py:180-198,
 * D/modules/common/prmsd.py:49-70 pRMSDCa, dpm_full.py:369-378 calc_dist_loss):
 *   prmsd = sum_n CE(prmsd_logits[n], bin of rmsd_n) m0_n / (sum_n m0_n + 1e-10), rmsd_n over the generated residues of position_scale (pred_p0 - p0),
 *           m0_n = mask_generate[n, 0]; pred_p0 = p_pred (pred_x0 = 1) or gen ? coef_a[n] p0 - coef_b[n] p_pred : p0 (pred_x0 = 0, transition.py:52-60);
 *   dist  = mean smooth_l1(cdist(p_pred) - cdist(p0)) over the pairs mask_generate_i & mask_res_i & mask_res_j (pred_x0 = 1 only).
 * sample_parts [N,4] = {CE_n, m0_n, sum of the sample's smooth-l1 terms, their count}; dprmsd_logits [N,num_bins] = softmax - onehot (scale by
 * m0_n / (sum m0 + 1e-10)); dp_pred [N,L,3] = d(sum of smooth-l1 terms)/d p_pred (scale by 1 / total count; zeros when pred_x0 = 0).  A sample without a
 * generated residue has rmsd = 0 / 0 = NaN and takes bin 0, as torch.argmin does.  1 <= num_bins <= 64.  A sample's positions live in the workgroup's LDS, 32 bytes
 * per residue beside the kernel's 48 bytes of static LDS: L <= abopt_abdock_losses_max_length() = 5118 = (163840 - 48) / 32; a longer L is refused
 * (ABOPT_EINVAL) before any HIP call, the outputs untouched.  (The entry is an addition: ABOPT_ABI_VERSION stays 59.) */
int abopt_abdock_losses_max_length(void);
int abopt_abdock_losses(const float* prmsd_logits, const float* p_pred, const float* p0_norm, const float* coef_a, const float* coef_b,
                        const uint8_t* mask_generate, const uint8_t* mask_res, const float* bin_offsets, int num_bins, int N, int L, float position_scale,
                        int pred_x0, float* sample_parts, float* dprmsd_logits, float* dp_pred, abopt_stream stream);
/* LayerNorm with the reference's definition (D/modules/common/layers.py:146-155: biased variance, sqrt(var + eps)) over rows of cols <= 256 values --
 * the prmsd head's layer_norm under autograd (D/modules/common/nn.py:179-188).  forward keeps xhat [rows,cols] and rstd [rows] (both or neither);
 * backward writes dx and dy_xhat = dy * xhat (d gamma = column sums of dy_xhat, d beta = column sums of dy: abopt_colsum). */
int abopt_layer_norm_forward(const float* x, const float* gamma, const float* beta, int cols, float eps, int64_t rows, float* y, float* xhat, float* rstd,
                             abopt_stream stream);
int abopt_layer_norm_backward(const float* dy, const float* xhat, const float* rstd, const float* gamma, int cols, int64_t rows, float* dx, float* dy_xhat,
                              abopt_stream stream);
int abopt_heads_epilogue_forward(const float* R, const float* v_t, const float* eps_crd, const float* eps_rot, const uint8_t* mask_generate,
                                 float* v_next, float* R_next, float* eps_pos, int64_t rows, int grad_mode, abopt_stream stream);
int abopt_heads_epilogue_backward(const float* R, const float* eps_rot, const uint8_t* mask_generate, const float* dR_next, const float* deps_pos,
                                  float* deps_crd, float* deps_rot, int64_t rows, abopt_stream stream);

/* ---- reconstruct_backbone_partially: D/modules/common/geometry.py:404-480 (called on every saved frame right after the
 * sampler, D/tools/runner/design_for_pdb.py:166-223).  pos_ctx/pos_new [N,L,A,3], mask_atoms/mask_new [N,L,A], R_new [N,L,3,3],
 * t_new [N,L,3] in Angstrom, mask_recons [N,L]; bb_table [21,3,3] / o_table [21,3] are the ideal local backbone coordinates
 * per residue type (D/utils/protein/constants.py:310-320; shipped as ab_opt_amd/data/backbone_ideal.npz). */
int abopt_reconstruct_backbone_partially(const float* pos_ctx, const float* R_new, const float* t_new, const int64_t* aa,
                                         const int64_t* chain_nb, const int64_t* res_nb, const uint8_t* mask_atoms,
                                         const uint8_t* mask_recons, const float* bb_table, const float* o_table,
                                         float* pos_new, uint8_t* mask_new, int N, int L, int A, abopt_stream stream);

/* ---- Training path: general strided-batched fp32 GEMM, C[b] = alpha * A[b] . B[b]^T (exact fp32 FMA chains on the matrix cores).
 *   A(m,k) = a_transposed ? A[k*lda + m] : A[m*lda + k]     B(n,k) = b_transposed ? B[k*ldb + n] : B[n*ldb + k]     C(m,n) = C[m*ldc + n]
 * It stands where the reference's autograd calls ATen GEMMs in the backward of the denoiser (D/modules/encoders/ga.py:54-66,81-147,
 * 174-177 and D/modules/diffusion/dpm_full.py:39-59 under torch.autograd).  ws (optional): scratch for split-K partial tiles, used when
 * the output has too few tiles to fill the chip and K >= 1024 (weight gradients); partials are summed in a fixed order.
 * bias (optional, [N]) is added to every row and relu != 0 clamps at zero in the product's epilogue: y = relu(x W^T + b), the nn.Linear +
 * nn.ReLU pairs of the heads / mixer / residue MLPs as one launch (no split-K then). */
int abopt_gemm(const float* A, int lda, int64_t stride_a, int a_transposed, const float* B, int ldb, int64_t stride_b, int b_transposed,
               float* C, int ldc, int64_t stride_c, int M, int N, int K, int batch, float alpha, const float* bias, int relu,
               void* ws, size_t ws_bytes, abopt_stream stream);

/* The weight-gradient products of one backward pass as a group: C_p = A_p^T . B_p for count <= 24 tall operand pairs, i.e.
 *   C_p[m*n_p + n] = sum over k < k_p of a_p[k*lda_p + m] * b_p[k*ldb_p + n]      (C_p dense [m_p, n_p]; a_p, b_p read in place)
 * -- d W = d y^T x of every nn.Linear the backward of the denoiser walks (D/modules/encoders/ga.py:54-79, D/modules/diffusion/dpm_full.py:39-65
 * under `loss.backward()`, D/train.py:101-114) -- in ONE launch plus one for the split-K slab sums of all of them, instead of two launches per
 * product.  Exact fp32 FMA chains on the matrix cores; the K split is chosen for the group's tile count; partial slabs are summed in a fixed order
 * (deterministic; the order differs from abopt_gemm's for the same product).  ws: scratch for the slabs, up to
 * sum_p min(1024 / total 64x64 tiles, k_p / 256) * m_p * n_p floats are used (less workspace: fewer slabs, never an error). */
typedef struct { const float* a; const float* b; float* c; int lda, ldb, m, n, k; } abopt_gemm_tn_problem;
int abopt_gemm_tn_grouped(const abopt_gemm_tn_problem* problems, int count, void* ws, size_t ws_bytes, abopt_stream stream);

/* out[c] = sum over rows of x[r*ld + c] (bias gradients and per-row partials of weight gradients on the training path); deterministic:
 * row slices are summed in a fixed order.  ws (optional): slices * cols floats of scratch. */
int abopt_colsum(const float* x, int ld, int64_t rows, int cols, float* out, void* ws, size_t ws_bytes, abopt_stream stream);

/* out[b*cols + c] = sum over the rows r with idx[r] == b of x[r*ld + c] (rows with idx outside [0, buckets) are skipped; buckets <= 96):
 * the gradient of an embedding table looked up once per row of a tall activation matrix -- the relative-position table of
 * D/modules/encoders/pair.py:46-53 over its N L^2 pair rows -- without the [rows, buckets] one-hot matrix autograd builds.  Deterministic. */
int abopt_bucket_colsum(const float* x, int ld, int64_t rows, int cols, const int32_t* idx, int buckets, float* out, void* ws, size_t ws_bytes,
                        abopt_stream stream);

/* The same sum per SEGMENT of rows_per_segment consecutive rows: out[(s*buckets + b)*cols + c] = sum over the rows j of segment s with bucket b of
 * x[(s*rows_per_segment + j)*ld + c], where the bucket of row j of segment s is idx[(s / idx_div)*rows_per_segment + j] (idx_div consecutive
 * segments share one index row).  With segment = (sample, query residue i), rows = key residues j and idx = the residue types of the sample this
 * is the first half of the gradient of the amino-acid-pair tables of D/modules/encoders/pair.py:46-53,66 (aa_pair_embed, aapair_to_distcoef),
 * summed over j by type(j); abopt_bucket_colsum over the (sample, i) rows by type(i) finishes it -- in place of the two one-hot batched products
 * (and a 268 MB contiguous copy of the strided operand) autograd would run.  Deterministic.  buckets <= 96, segments <= 65535. */
int abopt_segment_bucket_colsum(const float* x, int ld, int segments, int rows_per_segment, int cols, const int32_t* idx, int idx_div, int buckets,
                                float* out, abopt_stream stream);

/* ---- Training path: gradient clipping + Adam for a whole parameter list in a handful of launches.  Replaces, with the same arithmetic,
 *   orig_grad_norm = clip_grad_norm_(model.parameters(), config.train.max_grad_norm); optimizer.step()
 * of A/train.py:116-117 / D/train.py:112-113 with torch.optim.Adam(lr, betas, weight_decay) (A/diffab/utils/train.py:28-36; eps as given,
 * no amsgrad, no maximize), which torch runs as ~1000 small launches for the model's 207 tensors.
 *   params / grads / exp_avg / exp_avg_sq / numel : HOST arrays of `count` device pointers / element counts (fp32, contiguous)
 *   step  : device int64, the number of steps taken so far; incremented by the call (bias corrections use the incremented value)
 *   max_grad_norm > 0 : gradients are scaled by min(1, max_grad_norm / (||g||_2 + 1e-6)) inside the update (the gradient tensors themselves
 *                       are NOT rewritten) and the unclipped norm is stored in grad_norm_out[0] (device, may be NULL); <= 0: no clipping
 *   ws    : device scratch of abopt_adam_ws_floats(count, numel) floats.
 * Hyper-parameters are doubles, as Python holds them: 1 - beta and the bias corrections are formed in double and rounded once, as torch does.
 *   hyper_dev (optional, DEVICE, 6 doubles {lr, beta1, beta2, eps, weight_decay, max_grad_norm}): read by the kernels at execution time
 *   INSTEAD of the by-value arguments, so a captured hipGraph of the step follows a learning-rate scheduler (the reference's loops use
 *   ReduceLROnPlateau / MultiStepLR, A/diffab/utils/train.py:39-60): the host rewrites the buffer before a replay.  Whether clipping
 *   happens at all is still decided by the by-value max_grad_norm > 0 (it changes the launch list).
 * Deterministic (block partials of the norm are summed in a fixed order); capturable into a hipGraph (pointers travel as kernel arguments). */
size_t abopt_adam_ws_floats(int count, const int64_t* numel);
int abopt_adam_step(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                    const int64_t* numel, double lr, double beta1, double beta2, double eps, double weight_decay, double max_grad_norm,
                    int64_t* step, float* ws, size_t ws_floats, float* grad_norm_out, const double* hyper_dev, abopt_stream stream);

int abopt_commonness_score(const float* structs, float* score, int B, int n, abopt_stream stream);
/* G groups of S structures in one launch (ABI 42; the re-docks of every design of AbDock/optimize_ab.py:73-98, ranked like
 * design_for_pdb.py:326-345 ranks one run's candidates): structs [G*S,n,3] -> score [G*S], each score the commonness within its own group
 * of S, bit-identical to abopt_commonness_score called on that group.  S >= 2. */
int abopt_commonness_score_grouped(const float* structs, float* score, int G, int S, int n, abopt_stream stream);

/* ---- Pose clustering (ABI 47): the step a docking workflow puts between its sampler and everything expensive.  A docking sampler returns a few binding
 * modes many times over; this merges the near-duplicates so that the redesign and re-dock stages of the screen (AbDock/optimize_ab.py:12-98) run on ONE
 * representative per mode, and reports every mode's population -- for the D re-docks of a design, the share of the largest mode is the convergence
 * measure.  Nothing in the reference is matched; the definition is this library's own, per group of S structures [n,3]:
 *   distance    ssd(a, b) = sum_k |a_k - b_k|^2 over the n points WITHOUT superposition (abopt_commonness_score's distance), accumulated in fp32 as one
 *               fma chain over the 3 n coordinates in index order -- the same for (a, b) and (b, a), so the relation below is symmetric bit for bit
 *   neighbours  a ~ b iff ssd(a, b) <= cutoff^2 n, and a ~ a always (a structure holding a NaN is a neighbour of itself alone)
 *   greedy      all structures start alive; repeat: the alive structure with the most alive neighbours (ties: the lowest index) is the centre of the
 *               next cluster, its alive neighbours (itself included) are the members, which get the cluster's number as label and die; stop when nobody
 *               is alive or max_clusters clusters exist (0: no cap).  Structures still alive at the cap keep label -1.  Clusters are numbered in order
 *               of discovery and are NOT sorted.
 *   structs [G*S,n,3] -> label [G*S] (cluster of every structure, within its group), centre [G*S] (per group: the centres' indices WITHIN the group,
 *   -1 padded to S), size [G*S] (per group: members per cluster, 0 padded), count [G] (clusters per group); all four are DEVICE int32 arrays (spelled
 *   void* here: this header names no mutable int32 pointer type).  rmsd (optional, [G,S,S] fp32): sqrt(ssd / n) of every pair, symmetric bit for bit.
 *   ws: abopt_cluster_ws_bytes(G, S) bytes, 8-byte aligned (a bit matrix of S x ceil(S / 64) 8-byte words per group + one int32 per structure;
 *   0 for G = 0 and for an S the call refuses).
 * Two stream-ordered launches, nothing allocated, no host synchronisation.  1 <= S <= 16384 (beyond: ABOPT_EUNSUPPORTED), n >= 1, G S <= 2^31 - 1,
 * G <= 65535, G = 0 is a no-op, cutoff finite and >= 0; every check precedes the first launch.  A group's result is bit-identical to a call on that
 * group alone. */
size_t abopt_cluster_ws_bytes(int G, int S);
int abopt_cluster_poses_grouped(const float* structs, int G, int S, int n, float cutoff, int max_clusters, void* ws, size_t ws_bytes,
                                void* label, void* centre, void* size, void* count, float* rmsd, abopt_stream stream);

/* ---- Sequence clustering and composition (ABI 49): the sequence side of the same question.  A sequence-design model sampling S times on one backbone
 * returns near-identical designs many times over; this groups them so that the screen re-docks one design per family (and identical designs once), and
 * counts what every position holds.  Nothing in the reference is matched (its notebooks summarise designs on the host); the definition is this library's
 * own, per group of S sequences [n] of one byte per residue type (any byte value; bytes are compared for equality only):
 *   distance    d(a, b) = the number of positions k with a_k != b_k: an integer, exact, d(a, b) == d(b, a)
 *   neighbours  a ~ b iff d(a, b) <= max_mismatch, and a ~ a always; max_mismatch >= n puts every sequence of a group into one cluster
 *   greedy      exactly as abopt_cluster_poses_grouped above (the same kernel walks the relation): most alive neighbours first, ties to the lowest index,
 *               clusters numbered in order of discovery, max_clusters 0 = no cap, sequences still alive at the cap keep label -1
 *   seqs [G*S,n] uint8 -> label [G*S], centre [G*S], size [G*S], count [G]: DEVICE int32 arrays laid out as above.  dist (optional, [G,S,S] DEVICE
 *   int32): d of every pair, symmetric.  ws: abopt_cluster_ws_bytes(G, S) bytes, 8-byte aligned.
 * Two stream-ordered launches, nothing allocated, no host synchronisation, no floating point.  1 <= S <= 16384 (beyond: ABOPT_EUNSUPPORTED), n >= 1,
 * G S <= 2^31 - 1, G <= 65535, G = 0 is a no-op, max_mismatch >= 0; every check precedes the first launch.  A group's result is identical to a call on
 * that group alone.
 * abopt_sequence_profile_grouped: counts [G,n,21] DEVICE int32, counts[g][k][t] = how many of group g's S sequences hold type t < 20 at position k;
 * bin 20 counts every other byte (UNK, padding), so every position sums to S.  One launch; S >= 1, n >= 1, G n 21 <= 2^31 - 1, G <= 65535, G = 0 is a
 * no-op. */
int abopt_cluster_sequences_grouped(const uint8_t* seqs, int G, int S, int n, int max_mismatch, int max_clusters, void* ws, size_t ws_bytes,
                                    void* label, void* centre, void* size, void* count, void* dist, abopt_stream stream);
int abopt_sequence_profile_grouped(const uint8_t* seqs, int G, int S, int n, void* counts, abopt_stream stream);

/* ---- Shape clustering (ABI 59, an addition): abopt_cluster_poses_grouped with the structures SUPERPOSED before the distance is taken --
 * designed loops that live in different docked frames, pooled and grouped by conformation rather than by where the docking put them.  Nothing in the reference
 * is matched; per group of S structures [n,3], all n points being fitted and measured:
 *   distance    ss(a, b) = sum_k |R (x_k - cx) - (y_k - cy)|^2 with x = the structure of the LOWER index of the two, y = the other, cx, cy their centroids and R
 *               the best proper rotation of x onto y (Horn's quaternion form, a cyclic Jacobi solve, all in double: the pair function of
 *               abopt_superposed_rmsd below, one lane per pair).  Evaluating (a, b) and (b, a) as the same ordered pair makes the relation symmetric bit for bit.
 *   neighbours  a ~ b iff ss(a, b) <= (double) cutoff^2 n, and a ~ a always (a structure holding a NaN is a neighbour of itself alone)
 *   greedy      exactly as abopt_cluster_poses_grouped (the same kernel walks the relation)
 *   structs, label, centre, size, count, ws: as for abopt_cluster_poses_grouped.  rmsd (optional, [G,S,S] fp32): (float) sqrt(ss / n) of every pair, 0 on the
 *   diagonal, symmetric bit for bit, and equal bit for bit to abopt_superposed_rmsd on rows (min(a, b), max(a, b)) of the same structures with NULL masks.
 * Two stream-ordered launches, nothing allocated, no host synchronisation.  1 <= S <= 16384 (beyond: ABOPT_EUNSUPPORTED), G S <= 2^31 - 1, G <= 65535, G = 0
 * is a no-op, cutoff finite and >= 0.  3 <= n <= 256: below 3 points no rotation is determined and the call REFUSES (ABOPT_EINVAL) rather than report the
 * distance of an arbitrary optimal one; beyond 256: ABOPT_EUNSUPPORTED.  Every check precedes the first launch.  Collinear structures are compared as
 * abopt_superposed_rmsd compares them (score == fit: the distance is unique).  A group's result is bit-identical to a call on that group alone. */
int abopt_cluster_shapes_grouped(const float* structs, int G, int S, int n, float cutoff, int max_clusters, void* ws, size_t ws_bytes,
                                 void* label, void* centre, void* size, void* count, float* rmsd, abopt_stream stream);

/* ---- Interface geometry (ABI 48): the physical sanity check of a docked pose that every structure-generation pipeline reports -- steric clashes across the
 * interface, the size of the interface in contacts, broken peptide bonds -- and, per group, how often each residue is contacted across the group's candidates
 * (for the D re-docks of a design: the consensus epitope).  Nothing in the reference is matched (its relax stage is its only physical check); the definition is
 * this library's own.  G groups of S candidates, conventions of abopt_dockq_lite_grouped:
 *   pos [G*S,L,A,3] fp32; mask [G*S,L,A], or [G,L,A] shared by the S candidates of a group (mask_shared != 0); group [G,L] int32: 1 and 2 name the two sides,
 *   any other value takes no part; link (optional) [G,L]: link[r] != 0 = residue r is peptide-bonded to r + 1 (the last entry is ignored);
 *   clash_d, contact_d, bond_max in Angstrom: finite, clash_d and contact_d >= 0, a negative bond_max = breaks are not counted.
 *   distance    atoms p, q in fp32: dx = x_p - x_q (dy, dz likewise), d2(p, q) = fmaf(dz, dz, fmaf(dy, dy, dx dx)), every step rounded once: symmetric bit for
 *               bit.  The thresholds are clash_d clash_d, contact_d contact_d and bond_max bond_max, each rounded once in fp32.
 *   pairs       a residue pair (a, b) takes part iff group[a] == 1 and group[b] == 2 and, with link, the two are not bonded neighbours (b == a + 1 with link[a],
 *               or a == b + 1 with link[b]: a caller may put the generated residues on side 1 and the rest of their own chain on side 2 without counting every
 *               peptide bond as a clash).  An atom takes part iff its mask byte is set.
 *   out [G*S,5] int32 (DEVICE, spelled void*: this header names no mutable int32 pointer type), per candidate:
 *     0 clash     atom pairs of participating residue pairs with d2 < clash_d^2 (strict)
 *     1 contacts  participating residue pairs whose minimum d2 over their masked atom pairs is <= contact_d^2 (the <= of fnat.c); a residue without atoms
 *                 contacts nobody
 *     2 iface1    side-1 residues in at least one contact          3 iface2    the same for side 2
 *     4 breaks    r < L - 1 with link[r], atom 2 (C) of r and atom 0 (N) of r + 1 both masked, and NOT d2(C_r, N_r+1) <= bond_max^2: a NaN coordinate counts as a
 *                 break, a link with a missing atom does not; 0 without link or with bond_max < 0
 *     A NaN coordinate never clashes and never contacts: every comparison is false.
 *   freq (optional, [G,L] int32, DEVICE): freq[g,r] = the number of the group's S candidates in which residue r, of either side, is in at least one contact;
 *     cleared by the call in stream order, accumulated with integer atomics (deterministic).
 *   ws: abopt_interface_geometry_ws_bytes(G, S, L) bytes, 4-byte aligned (per candidate one bit per residue + four int32; 0 for an empty call).
 * Stream-ordered (three launches in one chain, no memset node: capturable into a hipGraph), nothing allocated, no host synchronisation.  L >= 1, 1 <= A <= 15, link needs
 * A >= 3, G S <= 2^31 - 1, G <= 65535, G = 0 or S = 0 is a no-op; every check precedes the first launch (ABOPT_EINVAL).  Residue pairs are pruned by bounding
 * spheres before their atoms are compared; the prune is conservative in fp32 and never changes a count.  A group's result is that of a call on the group alone. */
size_t abopt_interface_geometry_ws_bytes(int G, int S, int L);
int abopt_interface_geometry_grouped(const float* pos, const uint8_t* mask, int mask_shared, const int32_t* group, const uint8_t* link,
                                     int G, int S, int L, int A, float clash_d, float contact_d, float bond_max, void* out, void* freq,
                                     void* ws, size_t ws_bytes, abopt_stream stream);

/* ---- lDDT-CA (ABI 51): the superposition-free, bounded agreement score of two structures of one chain set, per residue -- where do a design's re-docks
 * disagree with the design, and with each other.  The reference carries the score as lddt() of D/modules/common/plddt.py:41-94 (CA, cutoff 15, the four
 * thresholds 0.5 / 1 / 2 / 4); this is that function as integer counts, with two deliberate differences: no eps inside the root, and a residue or pair set
 * without any scored pair is reported by den = 0 (Python: -1) where the reference returns eps / eps = 1.0.  G groups of S
 * candidates, conventions of abopt_dockq_lite_grouped and abopt_interface_geometry_grouped:
 *   pos [G*S,L,A,3] fp32; mask [G*S,L,A], or [G,L,A] shared by the S candidates of a group (mask_shared != 0); atom slot 1 is the CA, so A >= 2;
 *   rows (optional) [G,L] uint8: the residues i that are scored (NULL: all); group (optional) [G,L] int32, the interface form: a pair (i, j) takes part only
 *   if {group[i], group[j]} == {1, 2}; cutoff in Angstrom, finite and > 0 (15.0 in the reference).
 *   distance    d2(p, q) = fmaf(dz, dz, fmaf(dy, dy, dx dx)) with dx = __fsub_rn(x_p, x_q) and dx dx = __fmul_rn: the spelling of
 *               abopt_interface_geometry_grouped, every step rounded once; d = __fsqrt_rn(d2).  No eps inside the root.
 *   abopt_lddt_ca_grouped: candidate c of group g against ref_pos [G,L,A,3] / ref_mask [G,L,A].  Residue i is valid iff its CA byte is set in both the
 *     candidate's mask and the reference's.  For a valid i selected by rows, every valid j != i that passes the group test is a pair; dt is the CA-CA distance in
 *     the reference, dp in the candidate.  The pair is scored iff dt < cutoff (strict; a NaN dt is never scored).  A scored pair adds 1 to den[c,i] and
 *     [e < 0.5] + [e < 1] + [e < 2] + [e < 4] to num[c,i], e = |__fsub_rn(dt, dp)|: a NaN dp scores no hit, and the pair still counts in den.
 *     num, den [G*S,L] int32 (DEVICE, spelled void*: this header names no mutable int32 pointer type); every row that is not scored holds 0.
 *   abopt_lddt_ca_ensemble: no separate reference.  Entry (g, a, b) of num, den [G,S,S] int32 is the sum over i of the counts above with candidate a of the
 *     group as the reference and candidate b as the model, validity from both candidates' masks; the diagonal is computed like any other entry (num = 4 den).
 *     It equals, bit for bit, the sum over L of an abopt_lddt_ca_grouped call that is handed candidate a as ref_pos.
 *   The scores a caller derives: lddt_res = num / (4 den) per residue, lddt = sum_i num / (4 sum_i den) pooled (the reference's per_residue=False).
 *   ws: abopt_lddt_ws_bytes(G, S, L) bytes, 16-byte aligned (the CA of every structure as float4, the compacted rows; 0 for an empty call).
 * Stream-ordered (two launches in one chain, outputs and workspace cleared by a kernel: capturable into a hipGraph), nothing allocated, no host
 * synchronisation, no LDS.  1 <= L <= 16384 (4 L^2 fits an int32; beyond: ABOPT_EUNSUPPORTED), 2 <= A <= 15, G <= 65535, G S <= 2^31 - 1; the ensemble form:
 * S <= 16384 (beyond: ABOPT_EUNSUPPORTED) and G S S <= 2^31 - 1; G = 0 or S = 0 is a no-op; every check precedes the first launch.  The results are
 * integers: no order of the additions changes them, and a group's result is that of a call on the group alone. */
size_t abopt_lddt_ws_bytes(int G, int S, int L);
int abopt_lddt_ca_grouped(const float* pos, const uint8_t* mask, int mask_shared, const float* ref_pos, const uint8_t* ref_mask, const uint8_t* rows,
                          const int32_t* group, int G, int S, int L, int A, float cutoff, void* num, void* den, void* ws, size_t ws_bytes,
                          abopt_stream stream);
int abopt_lddt_ca_ensemble(const float* pos, const uint8_t* mask, int mask_shared, const uint8_t* rows, const int32_t* group, int G, int S, int L, int A,
                           float cutoff, void* num, void* den, void* ws, size_t ws_bytes, abopt_stream stream);

/* ---- Buried surface area (ABI 54): the solvent-accessible surface of each side of a docked candidate, alone and in the complex (Shrake-Rupley), per residue:
 * how much surface a pose buries, and on which residues -- the paratope and the epitope in A^2, where the contacts above count touches.  Nothing in the
 * reference is matched (its interface energy and dSASA came from its relax stage); the definition is this library's own.  G groups of S
 * candidates, conventions of abopt_interface_geometry_grouped:
 *   pos [G*S,L,A,3] fp32; mask [G*S,L,A], or [G,L,A] shared by the S candidates of a group (mask_shared != 0); group [G,L] int32: 1 and 2 name the two sides,
 *   any other value takes no part -- it is neither scored nor an occluder; radius [G,L,A] fp32, the van der Waals radius per atom slot in Angstrom;
 *   dirs [n_points,3] fp32 unit vectors, supplied by the caller, 1 <= n_points <= 1024; probe fp32, finite and >= 0; k fp32, the caller's rounding of 4 pi / n_points.
 *   taking part an atom takes part iff its mask byte is set, its residue's group is 1 or 2, its three coordinates are finite, and 0 < r <= 16 (a NaN radius takes no
 *               part).  An atom that takes no part has count 0 and occludes nothing.
 *   arithmetic  every step is rounded once, in fp32: __fadd_rn / __fsub_rn / __fmul_rn only, no fmaf, so that numpy float32 reproduces it bit for bit.
 *               For atom i with centre c and radius r:  R_i = r_i + probe;  T_i = R_i R_i;  test point p of atom i: q = c_i + R_i u_p per coordinate (one multiply,
 *               one add);  for an occluder j != i of the same candidate, in the same residue or any other: dx = q_x - c_jx (dy, dz likewise),
 *               d2 = (dx dx + dy dy) + dz dz in exactly this association;  point p is HIDDEN BY j iff d2 < T_j (strict).
 *   verdicts    own: the point is hidden by some participating atom of i's own side; other: by some participating atom of the other side.  The point is
 *               free-exposed iff not own, complex-exposed iff neither own nor other.  Every comparison is a pure function of the inputs: no pruning, tile order or
 *               early exit changes a verdict.
 *   pts [G*S,4] int32 (DEVICE, spelled void*): free-exposed points of side 1, of side 2, complex-exposed points of side 1, of side 2.
 *   area [G*S,L,2] fp32 (DEVICE, spelled void*): the free and the complex exposed area of each residue.  acc starts at 0.0f; for the participating atoms
 *               a = 0 .. A - 1 in ascending order acc = acc + float(count_a) (k T_a): the inner product is rounded first, then the product with the count, then the
 *               sum (an atom that takes no part is passed over: it would add 0).  A residue that takes no part gets 0, 0.  Free >= complex per atom by construction.
 *   ws: abopt_sasa_ws_bytes(G, S, L, A) bytes, 16-byte aligned (one bounding sphere per residue of every candidate; 0 for an empty call).
 * Stream-ordered (two launches in one chain, outputs cleared by a kernel, no memset node: capturable into a hipGraph), nothing allocated, no host synchronisation.
 * L >= 1, 1 <= A <= 15, G S <= 2^31 - 1, G <= 65535, G = 0 or S = 0 is a no-op; every check precedes the first launch (ABOPT_EINVAL; a workspace that is too
 * small: ABOPT_EWORKSPACE).  Occluder residues are pruned by bounding spheres; the prune is conservative in fp32 (it measures the caller's directions itself)
 * and never changes a verdict.  Only the four integer counters of pts are accumulated with atomics; a group's result is that of a call on the group alone. */
size_t abopt_sasa_ws_bytes(int G, int S, int L, int A);
int abopt_sasa_grouped(const float* pos, const uint8_t* mask, int mask_shared, const int32_t* group, const float* radius, const float* dirs, int n_points,
                       int G, int S, int L, int A, float probe, float k, void* pts, void* area, void* ws, size_t ws_bytes, abopt_stream stream);

/* ---- Guided sampling (ABI 56; no reference counterpart): after a reverse step t -> u, a geometric potential nudges the generated
 * residues of every sample -- towards an epitope, away from clashes.  In place on the step's stored state:
 *   p [N,L,3] fp32, Angstrom (the step's p_next); p_norm (optional, may be NULL) [N,L,3], its normalised copy (p_next_norm); mask_generate, mask_res [N,L];
 *   role [N,L] int32: bit 0 marks a hotspot, bit 1 a repeller, other bits are ignored.  role_shared = S > 0: role is [N/S,L] and sample n reads row n / S
 *   (the convention of pair_feat_shared); 0: one row per sample.
 *   row sets    per sample: the moved rows M = gen & res; the context rows ctx = res & ~gen; H = ctx & bit 0; R = ctx & bit 1.  Role bits on generated or
 *               masked-out rows mean nothing.
 *   scalars     fp32, finite and >= 0: w_att <= 1, r_att, w_rep, r_rep, max_shift > 0; position_scale > 0 and position_mean[3] (HOST) as abopt_step_params
 *               carries them.
 *   attraction  a rigid pull of the generated set towards the hotspots: with M and H both non-empty, d = mean_H p - mean_M p, D = |d|,
 *               a = w_att max(D - r_att, 0) / D d; a = 0 if D = 0 or either set is empty.  The same a applies to every moved row; with w_att <= 1 the pull
 *               never overshoots.
 *   repulsion   per moved row i: f_i = w_rep sum_{j in R} max(r_rep - d_ij, 0) / d_ij (p_i - p_j); a pair with d_ij^2 < 1e-12 contributes 0.  Moved rows do
 *               not repel one another: the network owns the loop's internal geometry.
 *   shift       D_i = a + f_i; if |D_i| > max_shift then D_i <- D_i max_shift / |D_i|.
 *   write-back  for the moved rows whose D_i has a non-zero component: p_i <- p_i + D_i and p_norm_i <- (p_i - position_mean) / position_scale per component,
 *               the formula of the step itself.  Every other element of p and p_norm keeps its bits.
 * All forces are formed from the positions BEFORE the update: only M changes, and the forces read context rows and the old centroid of M.  The potential is
 * continuous everywhere (its branch points are the two max(., 0) and the cap, and the shift is continuous at each), so the device is held to a float64 statement
 * of the above by a tolerance, not bit for bit; the sums are taken in fp32 in a fixed order (coordinates relative to position_mean), so repeated calls agree bit
 * for bit.  One launch, one workgroup per sample; no float atomic, no workspace, no memset, no host synchronisation: capturable into a hipGraph.
 * N = 0 or L = 0 is a no-op, and so is w_att = w_rep = 0.  A NULL pointer (p_norm apart), N % S != 0, a negative or non-finite scalar, w_att > 1, max_shift = 0 or
 * position_scale = 0: ABOPT_EINVAL with a message, before any launch.  The caller scales w_att and w_rep per step (Python: guide_decay). */
int abopt_guide_positions(float* p, float* p_norm, const uint8_t* mask_generate, const uint8_t* mask_res, const int32_t* role, int role_shared, int N, int L,
                          float w_att, float r_att, float w_rep, float r_rep, float max_shift, float position_scale, const float* position_mean,
                          abopt_stream stream);

/* ---- Relax of docked candidates (ABI 57; no reference counterpart: the reference relaxes with OpenMM / Rosetta): a deterministic,
 * training-free descent with a fixed number of iterations that moves every movable residue as a rigid body, down atom-level clashes and peptide-bond / CA-CA
 * violations, tethered to where the residue started.  The smallest honest relax, no force field.  G groups of S candidates, conventions of
 * abopt_interface_geometry_grouped:
 *   pos_in [G*S,L,A,3] fp32, read only; pos_out [G*S,L,A,3] fp32, may be the same pointer as pos_in; mask [G*S,L,A], or [G,L,A] shared by the S candidates of a
 *   group (mask_shared != 0); move [G,L]: the residues that may move; link (optional) [G,L] as for abopt_interface_geometry_grouped: without it there is no bond
 *   term, no CA term and no neighbour exclusion.  Atom slots 0, 1, 2 are N, CA, C, so 3 <= A <= 15.
 *   scalars     fp32, each finite and >= 0: w_bond, w_ca, w_clash, w_tether, clash_d (Angstrom), step; max_shift > 0 (Angstrom), max_angle > 0 (rad);
 *               iters 0 .. 1024.  max_moved: the caller's bound on the moved residues of any one candidate, 1 .. 256 after min(max_moved, L) -- it sizes the
 *               workgroup's LDS; a larger one: ABOPT_EUNSUPPORTED, before the launch.  (abopt_relax_max_moved() returns the 256.)
 *   taking part an atom takes part iff its mask byte is set and its three input coordinates are finite.  A residue is MOVED iff its byte of move is set and it has
 *               at least one participating atom.  An atom that takes no part is copied to pos_out bit for bit; it exerts nothing and feels nothing.
 *   energy      of a candidate at the positions x (x0: the input), d the Euclidean distance, b0 = 1.329 A and a0 = 3.80 A the conventional trans-peptide values:
 *     bond      r < L - 1 with link[r], C_r and N_r+1 participating, r or r + 1 moved:   w_bond (d(C_r, N_r+1) - b0)^2
 *     ca        the same r (link[r], r or r + 1 moved) with the CA of both participating:  w_ca (d(CA_r, CA_r+1) - a0)^2
 *     clash     unordered atom pairs (p of residue a, q of residue b), a != b, at least one of a, b moved, a and b not bonded neighbours by link (b == a + 1 with
 *               link[a] or a == b + 1 with link[b]), both atoms participating:          w_clash max(clash_d - d, 0)^2
 *     tether    participating atoms of moved residues:                                  w_tether |x - x0|^2
 *               A pair with d^2 < 1e-12 contributes no force (the rule of abopt_guide_positions); its energy is counted.
 *   iteration   a Jacobi update: every force is formed from the positions before the iteration.  For a moved residue a with its participating atoms P_a (n_a):
 *               f_p = -dE/dx_p;  c = mean of x_p;  F = sum f_p;  tau = sum (x_p - c) x f_p;  I = sum |x_p - c|^2;
 *               D = step F / n_a, scaled down to length max_shift if longer;  w = step tau / I (0 if I < 1e-12), scaled down to length max_angle if longer;
 *               x_p <- c + Rot(w)(x_p - c) + D,  Rot(w) v = v + (sin t / t) w x v + ((1 - cos t) / t^2) w x (w x v), t = |w| (the limits 1 and 1/2 for t^2 < 1e-12).
 *               Residues that are not moved never change.  iters = 0 copies the input.
 *   energy [G*S,2,4] fp32: bond, ca, clash, tether on the input and on the output positions.
 *   refusal on the device: a candidate with more moved residues than min(max_moved, L) is copied unchanged and its eight energies are NaN.
 * Every branch point (the max(., 0), the two caps) is continuous, so the device is held to a float64 statement of the above by a tolerance, not bit for bit, as
 * abopt_guide_positions is.  All sums are fp32 in a fixed order on coordinates relative to the candidate's first participating atom (lowest residue, then
 * slot), so an input far from the origin loses nothing; a moved residue is kept as its centre and its atoms' offsets from it -- a rotation acts on the offsets,
 * a shift on the centre (the mean of c + Rot(w)(x_p - c) + D is c + D).  Repeated calls agree bit for bit, and a group's result is that of a call on the group
 * alone.  Residue pairs are pruned by bounding spheres; the prune is conservative in fp32 and a pruned pair would have added exactly +0.
 * One stream-ordered launch, one workgroup per candidate, all iterations inside it; no float atomic, no memset node, no workspace, nothing allocated, no host
 * synchronisation: capturable into a hipGraph.  L >= 1, G S <= 2^31 - 1, G <= 65535, G = 0 or S = 0 is a no-op; every value or pointer check precedes the
 * launch (ABOPT_EINVAL). */
int abopt_relax_max_moved(void);
int abopt_relax_grouped(const float* pos_in, float* pos_out, const uint8_t* mask, int mask_shared, const uint8_t* move, const uint8_t* link,
                        int G, int S, int L, int A, int max_moved, float w_bond, float w_ca, float w_clash, float w_tether, float clash_d, float step,
                        float max_shift, float max_angle, int iters, float* energy, abopt_stream stream);

/* ---- Developability (ABI 58; no reference counterpart): what a designed sequence is, chemically, and where it lies on the surface --
 * the filters every antibody pipeline applies before synthesis.  Residue types are the library's: type k = 'ACDEFGHIKLMNPQRSTVWY'[k]; a byte >= 20 is "no type"
 * (UNK, padding), as in abopt_sequence_profile_grouped.
 *
 * abopt_sequence_liabilities_grouped -- integers only, one launch.  G groups of S designs of n positions:
 *   seqs [G*S,n] uint8; rows (optional, may be NULL) [G,n] uint8: the scored positions, e.g. the designed ones, NULL = all; link (optional, may be NULL) [G,n]
 *   uint8: link[k] != 0 means residue k is peptide-bonded to k + 1 (the last entry is ignored), NULL = every consecutive pair is bonded; run_min: 0 = class 6
 *   off, else 2 .. 16.
 *   window      the positions k .. k + w - 1 (anchor k, width w).  It EXISTS iff k + w - 1 < n, every step inside it is linked and every byte in it is < 20.
 *               It COUNTS iff it exists and at least one of its positions is a scored row: a sequon completed by designing its third residue beside a
 *               framework Asn is a liability of the design.
 *   classes     bit b of the flag byte at the anchor:  0 n_glyc: w = 3, N, not P, S or T;  1 deamidation: w = 2, N then G or S;  2 isomerisation: w = 2, D
 *               then G or S;  3 cleavage: w = 2, D then P;  4 cys: w = 1, C;  5 met: w = 1, M;  6 hydrophobic_run: w = run_min, every residue one of
 *               F, I, L, M, V, W, Y -- EVERY anchor of such a window is flagged, not only the first of a maximal run.
 *   flags [G*S,n] uint8 (DEVICE, spelled void*): the classes whose window at this anchor counts.
 *   counts [G*S,13] int32 (DEVICE, spelled void*), per design: 0-6 the windows counted per class; 7 the positions with a non-zero flag; 8 K + R, 9 D + E,
 *               10 H among the scored rows; 11 the scored rows whose byte is < 20; 12 hyd10: the sum over the scored rows of ten times the Kyte-Doolittle
 *               hydropathy, an exact integer -- in type order 18, 25, -35, -35, 28, -4, -32, 45, -39, 38, 19, -35, -16, -35, -45, -8, -7, 42, -9, -13; a byte
 *               >= 20 gives 0.  (hyd10 is column 12 of counts, not an output of its own.)
 *   freq (optional, may be NULL) [G,n] int32 (DEVICE, spelled void*): how many of the group's S designs carry any flag at position k.
 * Every output is written whole by plain stores: no atomic, no memset node, nothing to clear (with freq the flags are computed a second time, per group, by
 * further workgroups of the same launch).  Stream-ordered, capturable into a hipGraph, nothing allocated, no host synchronisation.  S >= 1, n >= 1,
 * G S n <= 2^31 - 1, G <= 65535, G = 0 is a no-op; a bad value or a NULL seqs / flags / counts: ABOPT_EINVAL with a message, before the launch.
 *
 * abopt_surface_patches_grouped -- fp32 in a fixed order, one launch.  G groups of S candidates, conventions of abopt_sasa_grouped:
 *   pos [G*S,L,A,3] fp32; mask [G*S,L,A], or [G,L,A] shared by the S candidates of a group (mask_shared != 0); group [G,L] int32: only side 1 is scored and only
 *   side 1 contributes (a caller scoring the antigen swaps the sides); area [G*S,L] fp32: the exposed area per residue, contiguous -- a column of
 *   abopt_sasa_grouped's area; seqs [G*S,L] uint8, or [G,L] shared by the group (seq_shared != 0: the re-docks of one design share their sequence);
 *   weight [21] fp32 (DEVICE): the hydrophobicity per type, entry 20 serves every byte >= 20; radius fp32 in Angstrom, finite and >= 0.
 *   centre      of a residue: its atom slot 4 (CB) if A >= 5 and that slot is masked in, else slot 1 (CA); so 2 <= A <= 15.
 *   taking part a residue takes part iff its group is 1, its centre's mask byte is set, its centre's three coordinates are finite, its area is finite and >= 0
 *               and its weight is finite.
 *   arithmetic  h_j = weight[t_j] area_j: one fp32 multiply, rounded once, fused into nothing.  d2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)) on the differences
 *               dx = c_ix - c_jx (dy, dz likewise), every step rounded once.  T = radius radius, rounded once.  j is a NEIGHBOUR of i iff both take part and
 *               d2 <= T; a residue is its own neighbour.
 *   patch [G*S,L] fp32 (DEVICE, spelled void*): for a residue that takes part acc = 0.0f, then acc = acc + h_j over its neighbours j in ascending j; 0 for
 *               any other residue.
 *   nbr [G*S,L] int32 (DEVICE, spelled void*): the number of neighbours; 0 for a residue that takes no part.
 * Every verdict is a pure function of the inputs; there is no prune.  A lane owns a target residue and adds by itself: no reduction, no atomic, so no order but
 * the definition's exists and a group's result is that of a call on the group alone.  Stream-ordered, capturable into a hipGraph, nothing allocated, no
 * workspace, no host synchronisation; the outputs are written whole.  L >= 1, 2 <= A <= 15, G S <= 2^31 - 1, G <= 65535, G = 0 or S = 0 is a no-op; every
 * value or pointer check precedes the launch (ABOPT_EINVAL). */
int abopt_sequence_liabilities_grouped(const uint8_t* seqs, const uint8_t* rows, const uint8_t* link, int run_min, int G, int S, int n, void* flags,
                                       void* counts, void* freq, abopt_stream stream);
int abopt_surface_patches_grouped(const float* pos, const uint8_t* mask, int mask_shared, const int32_t* group, const float* area, const uint8_t* seqs,
                                  int seq_shared, const float* weight, float radius, int G, int S, int L, int A, void* patch, void* nbr, abopt_stream stream);

/* ---- Interface energetics (ABI 59; no reference counterpart: the reference ranks its relaxed poses by Rosetta's dG_separated): what
 * the contacts across an interface are, chemically -- backbone hydrogen bonds, charge pairs and a caller's residue-pair table --, per residue.  A small
 * energy-LIKE score on the five backbone + CB slots, comparable between candidates of one complex and nothing more; every constant is a conventional value,
 * not a tuned one.  G groups of S candidates, conventions of abopt_interface_geometry_grouped and abopt_surface_patches_grouped:
 *   pos [G*S,L,A,3] fp32, 4 <= A <= 15, atom slots 0 .. 4 = N, CA, C, O, CB; mask [G*S,L,A], or [G,L,A] shared by the S candidates of a group (mask_shared != 0);
 *   group [G,L] int32: 1 and 2 name the two sides, any other value is on no side; seqs [G*S,L] uint8, or [G,L] shared by the group (seq_shared != 0), type k =
 *   'ACDEFGHIKLMNPQRSTVWY'[k], a byte >= 20 reads entry 20 of every table; link (optional, may be NULL) [G,L] uint8: link[r] != 0 means residue r is
 *   peptide-bonded to r + 1 (the last entry is ignored), NULL = every consecutive pair is bonded; charge [21] fp32 (DEVICE); pair_table (optional, may be NULL)
 *   [21,21] fp32 (DEVICE), NULL = the pair term is off.
 *   scalars     fp32: hb_cutoff finite and <= 0 (kcal/mol; conventionally -0.5); elec_cutoff, salt_cutoff, pair_cutoff finite and >= 0 (Angstrom;
 *               conventionally 15, 7, 8); eps and d_min finite and > 0 (conventionally 4 and 3 A).  Each cutoff and d_min is squared once in fp32.
 *   taking part an atom takes part iff its mask byte is set and its three coordinates are finite.  A term that needs an atom that takes no part is SKIPPED for
 *               that pair; it never becomes NaN.  This is the one rule; everything below builds on it.
 *   centre      of a residue: its CB (slot 4) if A >= 5 and that atom takes part, else its CA if that takes part; otherwise the residue has no centre.
 *   pairs       ordered pairs (owner i, partner j) with group[i] + group[j] == 3, both in {1, 2}.  A pair of bonded neighbours (j == i + 1 with link[i], or
 *               j == i - 1 with link[j]) is skipped for every term.
 *   arithmetic  fp32, every step rounded once, nothing fused: d2(a, b) = (dx dx + dy dy) + dz dz on dx = a_x - b_x (dy, dz likewise), in this association;
 *               distances are sqrt(d2); divisions and square roots are correctly rounded.
 *   amide H     residue r has one iff r >= 1, step r - 1 is linked, the type of r is not P (12), N of r and C, O of r - 1 take part (r - 1 need not be on a
 *               side) and len = sqrt(ux ux + uy uy + uz uz) > 0 for u = C_{r-1} - O_{r-1} (same association).  Then H = N_r + u / len per coordinate.
 *   1. hbond    (Kabsch & Sander 1983, the DSSP rule) donor d with an H and acceptor a with C and O taking part, both CA taking part and
 *               d2(CA_d, CA_a) < 81 (DSSP's 9 A pre-filter is part of the definition):
 *               E = 27.888 (((1 / r_ON + 1 / r_CH) - 1 / r_OH) - 1 / r_CN), r_XY = |X_a - Y_d|; if any of the four distances is < 0.5 A, E = -9.9; otherwise
 *               E = -9.9 where E < -9.9.  A bond EXISTS iff E < hb_cutoff.  For each partner j the owner is examined as donor to j, then as acceptor from j;
 *               each existing bond adds E to the owner's hb energy and 1 to its donor / acceptor count.
 *   2. charges  q = charge[type]; a NaN entry reads as 0.  With both centres, q_i != 0, q_j != 0 and d2 <= elec_cutoff^2 (d2 between the centres):
 *               E = (332.0637 (q_i q_j)) / (eps max(d2, d_min^2)) -- Coulomb with the dielectric eps r, no exponential screening -- is added to the owner's
 *               elec energy.  Such a pair with d2 <= salt_cutoff^2 is a SALT BRIDGE if q_i q_j < 0 and a LIKE-CHARGE PAIR if q_i q_j > 0.
 *   3. pairs    with both centres and d2 <= pair_cutoff^2 the partner is counted (column 4, with or without a table) and, with pair_table given,
 *               pair_table[t_i][t_j] -- the row is the owner's, the table need not be symmetric -- is added to the owner's pair energy; a NaN entry adds nothing.
 *   energy [G*S,L,3] fp32 (DEVICE, spelled void*): hb, elec, pair.  Each starts at 0.0f and takes its terms over the partners j in ascending j, within a j the
 *               donor term before the acceptor term: acc = acc + E, rounded once.  Every pair's energy is attributed in full to BOTH of its residues, so a
 *               per-candidate total sums one side only.
 *   count [G*S,L,5] int32 (DEVICE, spelled void*): bonds as donor, bonds as acceptor, salt bridges, like-charge pairs, partners within pair_cutoff.
 *   A residue on no side gets zeros in both.
 * Every verdict is a pure function of the inputs; there is no prune beyond the definition's own tests.  A lane owns a residue and adds by itself: no reduction,
 * no atomic, so no order but the definition's exists and a group's result is that of a call on the group alone.  One stream-ordered launch, capturable into a
 * hipGraph, nothing allocated, no workspace, no host synchronisation; the outputs are written whole by plain stores.  L >= 1, G S <= 2^31 - 1, G <= 65535,
 * G = 0 or S = 0 is a no-op; every value or pointer check precedes the launch (ABOPT_EINVAL). */
int abopt_interface_energy_grouped(const float* pos, const uint8_t* mask, int mask_shared, const int32_t* group, const uint8_t* seqs, int seq_shared,
                                   const uint8_t* link, const float* charge, const float* pair_table, int G, int S, int L, int A, float hb_cutoff,
                                   float elec_cutoff, float salt_cutoff, float pair_cutoff, float eps, float d_min, void* energy, void* count,
                                   abopt_stream stream);

/* ---- Backbone conformation (ABI 59, an addition: no existing signature moves): whether a candidate's backbone is a plausible
 * polypeptide BETWEEN its residues -- torsions, the peptide bond's geometry, a Ramachandran class, cis / twisted peptides and DSSP-LIKE states from
 * Kabsch & Sander's hydrogen-bond patterns within the candidate.  This is NOT DSSP: there are no ladders or sheets, no B / E distinction, no bends and no helix
 * trimming.  Nothing in the reference is matched; the definition is this library's own.  G groups of S candidates, conventions of
 * abopt_interface_energy_grouped:
 *   pos [G*S,L,A,3] fp32, 4 <= A <= 15, atom slots 0 .. 3 = N, CA, C, O; mask [G*S,L,A], or [G,L,A] shared by the S candidates of a group (mask_shared != 0);
 *   rows [G,L] uint8 flags: the SCORED residues; seqs (optional, may be NULL) [G*S,L] uint8, or [G,L] shared by the group (seq_shared != 0), type k =
 *   'ACDEFGHIKLMNPQRSTVWY'[k]: Pro = 12, Gly = 5, a byte >= 20 is no type, NULL = no residue is Pro or Gly; link (optional, may be NULL) [G,L] uint8:
 *   link[r] != 0 means STEP r -- residue r is peptide-bonded to r + 1 -- is linked (the last entry is ignored: there is no step L - 1, nor a step -1),
 *   NULL = every step 0 .. L - 2 is linked; regions [K,8] fp32 (DEVICE; may be NULL with K = 0), 0 <= K <= 8; hb_cutoff fp32, finite and <= 0
 *   (kcal/mol; conventionally -0.5).
 *   taking part an atom takes part iff its mask byte is set and its three coordinates are finite (the one rule of abopt_interface_energy_grouped).  A RESIDUE
 *               takes part iff one of its slots 0 .. 3 does.  A quantity that needs an atom that takes no part is UNDEFINED for that residue; nothing becomes
 *               NaN.  Every residue that takes part is a neighbour and a hydrogen-bond partner whether or not it is a scored row; only scored rows are
 *               counted, and a row that is not scored gets torsion = bond = 0, have = ss = 0, rama = state = 255, partner = -1.
 *   arithmetic  fp32, every step rounded once, nothing fused; divisions and square roots correctly rounded.  a - b per coordinate;
 *               a . b = (ax bx + ay by) + az bz; a x b = (ay bz - az by, az bx - ax bz, ax by - ay bx); d2(a, b) = (a - b) . (a - b), which is the d2 of
 *               abopt_interface_energy_grouped.
 *   torsion     of four points p0 .. p3: b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2; n1 = b1 x b2, n2 = b2 x b3; x = n1 . n2; y = sqrt(b2 . b2) (b1 . n2);
 *               rho = sqrt(x x + y y); cos = x / rho, sin = y / rho (IUPAC sign: a trans peptide has cos = -1).  Undefined unless 0 < rho < inf.
 *               phi_r = (C_{r-1}, N, CA, C) needs step r - 1 linked; psi_r = (N, CA, C, N_{r+1}) and omega_r = (CA, C, N_{r+1}, CA_{r+1}) need step r linked;
 *               omega belongs to r.
 *   torsion [G*S,L,6] fp32 (DEVICE, spelled void*): cos phi, sin phi, cos psi, sin psi, cos omega, sin omega; an undefined pair is 0.0f, 0.0f.
 *   have [G*S,L] uint8: bit 0 phi, 1 psi, 2 omega, 3 .. 5 the three entries of bond, set where defined.
 *   bond [G*S,L,3] fp32 (DEVICE, spelled void*) of a linked step r: |C - N_{r+1}| = sqrt(d2(C, N_{r+1})), defined iff it is < inf;
 *               cos(CA-C-N_{r+1}) and cos(C-N_{r+1}-CA_{r+1}), the cosine at vertex v of a, b being ((a - v) . (b - v)) / (sqrt((a - v) . (a - v))
 *               sqrt((b - v) . (b - v))), defined iff 0 < that denominator < inf.  Undefined entries are 0.0f.
 *   rama [G*S,L] uint8: a region is cos, sin of phi_lo, of phi_hi, of psi_lo, of psi_hi (8 floats): a box of two counter-clockwise arcs, each strictly
 *               narrower than 180 degrees.  theta lies in [lo, hi] iff sin theta cos lo - cos theta sin lo >= 0 and cos theta sin hi - sin theta cos hi >= 0
 *               (two products and a difference each, on the cos and sin of `torsion`).  A scored row with phi and psi gets the lowest k whose two arcs hold
 *               them, K if none does (an outlier); 255 otherwise.
 *   peptide     of a scored row with omega: cis iff cos omega > 0; twisted iff |sin omega| > 0.5; cis is counted once more where r + 1 is not Pro.
 *   hbond       amide H and E exactly as in abopt_interface_energy_grouped (H = N_r + u / |u|, u = C_{r-1} - O_{r-1}; none for Pro, r = 0, an unlinked
 *               step r - 1, a missing N, C_{r-1}, O_{r-1} or |u| = 0; E = 27.888 (((1 / r_ON + 1 / r_CH) - 1 / r_OH) - 1 / r_CN), -9.9 if a distance is
 *               below 0.5 A, else max(E, -9.9)).  hb(a -> d), acceptor a and donor d of ONE candidate, exists iff a != d, they are not linked neighbours
 *               (d == a + 1 with step a linked, or a == d + 1 with step d linked), d has an H, C and O of a and both CA take part,
 *               d2(CA_d, CA_a) < 81 (part of the definition) and E < hb_cutoff.  Hbond(i, j) = hb(acceptor i -> donor j); false outside 0 .. L - 1.
 *   patterns    n-turn at i, n in {3, 4, 5}: Hbond(i, i + n) with every step i .. i + n - 1 linked.  helix_n on the residues i .. i + n - 1 iff there are
 *               n-turns at i - 1 and at i.  r is INSIDE a turn iff there is an n-turn at some i with i < r < i + n.  bridge(i, j) needs |i - j| >= 3 and the
 *               steps i - 1, i, j - 1, j linked; parallel: [Hbond(i-1, j) and Hbond(j, i+1)] or [Hbond(j-1, i) and Hbond(i, j+1)]; antiparallel:
 *               [Hbond(i, j) and Hbond(j, i)] or [Hbond(i-1, j+1) and Hbond(j-1, i+1)].  j need not be a scored row.
 *   ss [G*S,L] uint8 of a scored row that takes part: bit 0 helix_4, 1 helix_3, 2 helix_5, 3 a parallel bridge, 4 an antiparallel bridge, 5 inside a turn.
 *   state [G*S,L] uint8 of such a row: 0 H (helix_4), else 1 E (a bridge), else 2 G (helix_3), else 3 I (helix_5), else 4 T (inside a turn), else 5 C;
 *               255 for any other row.
 *   partner [G*S,L,2] int32 (DEVICE, spelled void*): the lowest j with a parallel, with an antiparallel bridge(r, j); -1 if none.
 *   count [G*S,24] int32 (DEVICE, spelled void*), over the scored rows: 0 rows that take part; 1 rows with phi and psi; 2 .. 9 rows of region 0 .. 7;
 *               10 outliers; 11 outliers that are Gly; 12 rows with omega; 13 cis; 14 cis with r + 1 not Pro; 15 twisted; 16 .. 21 rows of state H, E, G,
 *               I, T, C; 22 hydrogen bonds whose donor is a scored row; 23 those whose acceptor is one.
 * Every output is a pure function of the candidate; the counts are integers, so no order of summation exists, and a group's result is that of a call on the
 * group alone.  One stream-ordered launch, a workgroup per candidate, capturable into a hipGraph, nothing allocated, no workspace, no global atomic, no host
 * synchronisation; the outputs are written whole by plain stores.  L >= 1, G S <= 2^31 - 1, G <= 65535, G = 0 or S = 0 is a no-op; every value or pointer
 * check precedes the launch (ABOPT_EINVAL).  The relation hb lives in the workgroup's LDS: L <= abopt_backbone_max_rows() = 512, beyond that
 * ABOPT_EUNSUPPORTED and nothing is launched. */
int abopt_backbone_max_rows(void);
int abopt_backbone_conformation_grouped(const float* pos, const uint8_t* mask, int mask_shared, const uint8_t* rows, const uint8_t* seqs, int seq_shared,
                                        const uint8_t* link, const float* regions, int K, int G, int S, int L, int A, float hb_cutoff, void* torsion,
                                        void* have, void* bond, void* rama, void* ss, void* state, void* partner, void* count, abopt_stream stream);

/* ---- Similarity to reference sequences and loops: the `seqid` and `rmsd` of the reference's eval stage (tools/eval/similarity.py)
 * for sequences and residue lists of DIFFERENT lengths.  Both entries compare every one of Q query rows with every one of R reference rows.
 * ABOPT_ABI_VERSION stays 59: the two entries are additions, no existing signature moves, and a library built before them is still caught, because binding
 * the signature table fails on the missing symbol.
 *   rows        a row has na (query) or nb (reference) elements and a mask of one byte per element, NULL = all true; a row's SEQUENCE is its mask-true
 *               elements in order -- masks need not be prefixes, and a row may be empty.
 *
 * abopt_align_sequences -- integers only.  Global alignment with a substitution table and affine gaps, end gaps free.
 *   q [Q,na] uint8, qmask (may be NULL) [Q,na] uint8; r [R,nb] uint8, rmask (may be NULL) [R,nb] uint8; table [T,T] int32 (DEVICE), 1 <= T <= 32, row = the
 *   query's byte, column = the reference's, a byte >= T reads row or column T - 1; an entry beyond +-32767 is read as +-32767; gap_open and gap_extend with
 *   -32767 <= gap_open <= gap_extend <= 0.
 *   alignment   a sequence of columns, each a pair (a_i, b_j), a gap against b_j or a_i against a gap, that spells a (the query's sequence) and b in order.
 *   gap run     a maximal run of consecutive columns with the gap on the SAME side.  A run that touches either end of the alignment costs nothing; any
 *               other run of k columns costs gap_open + (k - 1) gap_extend.  (A run of one side directly after a run of the other is a run of its own: behind
 *               a leading run it does not touch the end, so it is paid.)
 *   pair        scores table[a_i][b_j] and is a MATCH iff the two raw bytes are equal (also when both are >= T).
 *   score, matches, columns [Q,R] int32 (DEVICE, spelled void*): score is the maximum over all alignments; matches the largest number of matches among the
 *               alignments of that score; columns the smallest number of columns among those.  All three are additive along an alignment, so a three-state
 *               Gotoh recurrence that carries (score, matches, -columns) and takes the lexicographic maximum computes them; the result depends on no
 *               traceback order.  With gap_open <= gap_extend it equals the enumeration of every alignment
 *               (tests/test_similarity.py::test_alignment_statement_equals_brute_force).  If either sequence is empty: 0, 0, max(len a, len b).
 *   seqid       100 matches / columns is the identity over the alignment's columns that the reference reports.  UNVERIFIED against it: Biopython's first
 *               alignment may be another co-optimal one, so the identity can differ on ties (Biopython is not a dependency and nothing here was compared
 *               with it).  The score has no such ambiguity.
 *
 * abopt_gapped_rmsd -- fp32 in a fixed order.  The reference's reslist_rmsd as written: CA deviations minimised over gapped placements, no superposition.
 *   qca [Q,na,3] fp32, qmask (may be NULL) [Q,na]; rca [R,nb,3] fp32, rmask (may be NULL) [R,nb].
 *   lists       s is the shorter sequence (M residues) and l the longer (N); with equal lengths the query is s.  d(i, j) = fmaf(dz, dz, fmaf(dy, dy, dx dx))
 *               on dx = s_ix - l_jx (dy, dz likewise), every step rounded once.
 *   recurrence  SD[M-1][j] = d(M-1, j);  for i < M - 1 and j <= N - M + i:  SD[i][j] = min(d(i, j) + SD[i+1][j+1], SD[i][j+1]), where SD[i][N-M+i+1] reads
 *               +inf -- so the boundary diagonal is built by the same addition, d + SD[i+1][j+1], and the order of additions is fixed.  One fp32 add and one
 *               min per cell.
 *   sd [Q,R] fp32 (DEVICE, spelled void*): min over j <= N - M of SD[0][j];  m [Q,R] int32 (DEVICE, spelled void*): M.  If either sequence is empty: sd = -1
 *               and m = 0.  The caller's rmsd is sqrt(sd / m).
 *   ADJACENT LAST PAIR  the last row is d itself, not its running minimum, so the result is the minimum over the order-preserving placements of s in l in
 *               which the LAST TWO residues of s are adjacent in l (for M >= 2), not over all of them.  That is the reference's number and is kept on
 *               purpose (tests/test_similarity.py::test_rmsd_statement_is_the_adjacent_last_minimum).
 *   Coordinates are expected to be finite; a NaN is dropped or kept by a min as fminf does.
 * Both: one launch, a wave per pair, four pairs per workgroup; no atomic, no workspace, nothing allocated, no host synchronisation, capturable into a hipGraph;
 * the outputs are written whole by plain stores and a pair's result is that of a call on the pair alone.  Q, R >= 0, na, nb >= 1, Q R <= 2^31 - 1
 * (ABOPT_EINVAL); na, nb <= 256 (beyond: ABOPT_EUNSUPPORTED); Q = 0 or R = 0 is a no-op; every check precedes the launch. */
int abopt_align_sequences(const uint8_t* q, const uint8_t* qmask, const uint8_t* r, const uint8_t* rmask, const int32_t* table, int T, int gap_open,
                          int gap_extend, int Q, int R, int na, int nb, void* score, void* matches, void* columns, abopt_stream stream);
int abopt_gapped_rmsd(const float* qca, const uint8_t* qmask, const float* rca, const uint8_t* rmask, int Q, int R, int na, int nb, void* sd, void* m,
                      abopt_stream stream);

/* ---- RMSD after superposition (ABI 59, an addition): every one of Q query rows against every one of R reference rows, fitted on one
 * subset of the paired points and measured on another.  "Is this the same loop shape" for designs that live in different frames; fit on the framework and
 * score on the CDR for the loop-modelling number; a panel of known loops against every design.  Nothing in the reference is matched (its eval stage takes its
 * RMSD without superposition, abopt_gapped_rmsd above); the definition is this library's own.
 *   q [Q,na,3] fp32, r [R,nb,3] fp32; qfit, qscore [Q,na] and rfit, rscore [R,nb]: one byte per element.  qfit / rfit NULL = all true; qscore / rscore NULL =
 *   the same as that row's fit mask.  Masks need not be prefixes.
 *   pairing     by RANK: the k-th fit-true element of the query row pairs with the k-th fit-true element of the reference row; the score elements likewise.
 *               The query x is the mobile side, the reference y the target.
 *   fit         cx, cy = the means of the n_f fit points; S[a][b] = sum (x_a - cx_a)(y_b - cy_b) over the fit pairs; R = the rotation of the unit quaternion
 *               that is the largest-eigenvalue eigenvector of Horn's 4x4 key matrix of S (a cyclic Jacobi solve of at most 16 sweeps): a proper rotation, never
 *               a reflection.  All in double from the fp32 inputs, summed in index order by ONE lane per pair: a pair's result is a pure function of its two
 *               point lists and is that of a call on the pair alone, bit for bit.
 *   residuals   ss = sum |R (x - cx) - (y - cy)|^2 over the n_s score pairs, in double, with the rotation applied.
 *   rmsd [Q,R] fp32 = (float) sqrt(ss / n_s); n_fit, n_score [Q,R] int32 (DEVICE, spelled void*): n_f and n_s of the pair.
 *   rot (may be NULL) [Q,R,3,3] fp32 row-major and trans (may be NULL) [Q,R,3] fp32: R and t = cy - R cx, so that y ~ R x + t.
 *   NOT SCORED  a pair whose two fit counts differ, or whose two score counts differ, or with n_f < 3 (no rotation is determined), or with n_s = 0:
 *               rmsd = -1, n_fit = n_score = 0, rot = the identity, trans = 0.
 *   COLLINEAR   with n_f >= 3 collinear fit points the two largest eigenvalues coincide and the result is that of SOME optimal rotation (whatever turn about the
 *               line the sweeps leave).  With score == fit the rmsd is unique all the same; rot, trans and an rmsd over other points are not.
 *   Coordinates are expected to be finite; a NaN in a scored pair's points gives rmsd = NaN (the solve ends whatever the data).
 * One launch, 16 x 16 pairs per workgroup, a lane per pair; no atomic, no workspace, nothing allocated, no host synchronisation, capturable into a hipGraph; the
 * outputs are written whole by plain stores.  Q, R >= 0, na, nb >= 1, Q R <= 2^31 - 1 (ABOPT_EINVAL); na, nb <= 256 (beyond: ABOPT_EUNSUPPORTED, nothing
 * launched); Q = 0 or R = 0 is a no-op; every check precedes the launch. */
int abopt_superposed_rmsd(const float* q, const uint8_t* qfit, const uint8_t* qscore, const float* r, const uint8_t* rfit, const uint8_t* rscore, int Q, int R,
                          int na, int nb, void* rmsd, void* n_fit, void* n_score, void* rot, void* trans, abopt_stream stream);

/* ---- The alignment itself, and superposition on its pairs (ABI 59, additions).
 *
 * abopt_align_traceback -- integers only.  The rows, masks, table, gaps and prices of abopt_align_sequences above, for P chosen pairs of rows.
 *   pairs       (may be NULL) [P,2] int32 (DEVICE): (query row, reference row) of pair p, in any order, repeats allowed.  NULL: all Q R pairs, row-major, and P
 *               is ignored.  The intended use: score everything with abopt_align_sequences, choose, trace the chosen pairs only -- tracing 10^6 pairs of
 *               rows of 256 writes 0.5 GB of maps.  A pair outside [0, Q) x [0, R) reads nothing and writes score 0, matches 0, columns 0, ops 0, maps -1.
 *   word        an alignment of a (the query's sequence, n residues) and b (m residues) is a word over three letters: P, a pair; A, a residue of a against a
 *               gap; B, a gap against a residue of b.  It spells both sequences and is priced as above (gap runs, free ends, a match iff the raw bytes are equal).
 *   THE ALIGNMENT  among the words that attain the lexicographic maximum of (score, matches, -columns): the word that is lexicographically least when read
 *               from its LAST column to its first, with P < A < B.  This names one alignment whatever computes it (tests/alignment_trace_statement.py
 *               enumerates the words; the kernel walks the Gotoh tables backwards over SETS of states, closing each set under the ties X = H and Y = H and
 *               writing the least letter any state can write over a tight edge -- a single-state walk with a fixed preference is wrong on ties).
 *               If either sequence is empty: the word is all A or all B.  If nothing is worth pairing: B^m A^n.
 *   score, matches, columns [P] int32 (DEVICE, spelled void*): equal to abopt_align_sequences on the same pair, exactly; 100 matches / columns is the seqid of
 *               THE alignment.
 *   ops         (may be NULL) [P, na + nb] uint8: column c < columns of the alignment, left to right: 1 = P, 2 = A, 3 = B; 0 beyond.
 *   qmap        (may be NULL) [P, na] int16: for ELEMENT k of the query row (an index into the row, not a rank: masks that are no prefixes map directly) the
 *               element index of the reference row it is paired with; -1 if the element is masked out, against a gap or in a free overhang.
 *   rmap        (may be NULL) [P, nb] int16: the inverse.
 * One launch, a wave per pair, 4, 2 or 1 pairs per workgroup (na round8(nb) bytes of LDS per pair, at most 64 KiB); no atomic, no workspace, nothing allocated,
 * no host synchronisation, capturable; every output written whole by plain stores; the walk takes `columns` steps whatever the bytes.  Checks: dims (P >= 0
 * with pairs), na, nb <= 256 (beyond: ABOPT_EUNSUPPORTED), T and the gaps, the no-op (P = 0 with pairs, Q R = 0 without), pointers.
 *
 * abopt_superposed_rmsd_mapped -- abopt_superposed_rmsd on the pairs a map names, so that rows of DIFFERENT lengths superpose.
 *   q [Q,na,3], r [R,nb,3] fp32; qmap [P,na] int16 (DEVICE, spelled void*, read only); pairs as above; qfit, qscore [Q,na] and rfit, rscore [R,nb] bytes.
 *   fit pairs   of pair p: the (k, j = qmap[p][k]) in ascending k with 0 <= j < nb, qfit true at k and rfit true at j (NULL = all).  The score pairs likewise
 *               from the score masks; a NULL score mask on a side is that side's fit mask.  A j outside [0, nb) means "unpaired" and is never dereferenced.
 *               The map need not come from abopt_align_traceback, nor be monotone: a caller's own pairing is legal.
 *   rmsd, n_fit, n_score [P]; rot (may be NULL) [P,3,3], trans (may be NULL) [P,3]: as abopt_superposed_rmsd defines them, by the same pair function on the
 *               same two point lists -- so the result equals abopt_superposed_rmsd on the pairs gathered into rows of equal count, bit for bit.
 *   NOT SCORED  fewer than 3 fit pairs, no score pair, or a pair outside the panels: rmsd = -1, n_fit = n_score = 0, rot = the identity, trans = 0.
 * One launch, a lane per pair, rows read straight from memory; no atomic, no workspace, capturable.  Checks as above. */
int abopt_align_traceback(const uint8_t* q, const uint8_t* qmask, const uint8_t* r, const uint8_t* rmask, const int32_t* table, int T, int gap_open,
                          int gap_extend, const int32_t* pairs, int P, int Q, int R, int na, int nb, void* score, void* matches, void* columns, void* ops,
                          void* qmap, void* rmap, abopt_stream stream);
int abopt_superposed_rmsd_mapped(const float* q, const float* r, void* qmap, const int32_t* pairs, int P, const uint8_t* qfit, const uint8_t* qscore,
                                 const uint8_t* rfit, const uint8_t* rscore, int Q, int R, int na, int nb, void* rmsd, void* n_fit, void* n_score, void* rot,
                                 void* trans, abopt_stream stream);

/* ---- Measurement hook (bench.py's roofline leg).  When enabled, every launch of the IPA-core kernel is bracketed
 * by hipEvents on the stream it is launched on; abopt_prof_collect synchronises those events and returns the number
 * of launches and their summed duration since the last enable.  Process-global, off by default, not for concurrent
 * use from several host threads (the only global state in the library). */
int abopt_prof_enable(int on);   /* 1: on (forgets earlier pairs), 0: off (forgets), 2: off but keep the recorded pairs;
                                    3: launch spans on (below), 4: stop handing out span slots */
/* Launch spans: the dominant kernel timed INSIDE a replayed hipGraph, where host-recorded event pairs cannot be placed.  While mode 3 is on
 * (e.g. during the capture), every 32-row IPA launch (core, or fused core + tail) is given a slot number; each of its workgroups folds the
 * 100 MHz wall clock of its first / last instruction into {min, max} of the slot.  abopt_prof_spans_reset (stream-ordered) clears the slots --
 * call it before the replay to be read --, abopt_prof_spans synchronises the device and returns the number of launches that ran since and
 * the sum of their (max end - min start) in milliseconds. */
int abopt_prof_spans_reset(abopt_stream stream);
int abopt_prof_spans(int* launches, double* total_ms);
int abopt_prof_collect(int* launches, double* total_ms);
/* Clock probe: shader cycles and 100 MHz wall-clock ticks that wave 0 of workgroup 0 of the most recent 32-row IPA launch (core or fused
 * core + tail) spent from its first to its last instruction: cycles / (10 ns * ticks) = the clock the chip sustained under that kernel.
 * Synchronises the device.  Zeros when no such launch has run. */
int abopt_prof_clock(long long* cycles, long long* wall_ticks_100mhz);
/* The same sum without forgetting the event pairs: records captured into a hipGraph are re-recorded by every replay. */
int abopt_prof_peek(int* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* ABOPT_H */
