// Which launches a denoiser forward is made of: the ONE place that decides (api.hip reads the switches once per entry, builds a ForwardQuery and walks the plan;
// the launchers of ipa_core.hip / ipa.hip take the CorePlan they are handed).  plan_ipa_core (ipa_plan.h) is called from here and from nowhere else on the
// forward path.  Plain host C++17, no HIP: tests/forward_plan_table.cpp, tests/forward_plan_carry_table.cpp, tests/forward_plan_rows_table.cpp and tests/forward_plan_compact_table.cpp
// tabulate the functions without a device (tests/test_forward_plan.py, tests/test_forward_plan_carry.py, tests/test_forward_plan_rows.py, tests/test_forward_plan_compact.py).
#pragma once
#include "ipa_plan.h"

namespace abopt {

constexpr int kMaxBlocks = 8;       // blocks of one encoder (the pair-bias cache holds as many layers)

// The environment switches as values (api.hip: read_switches, once per C-ABI call -- callers flip them between calls of one process)
struct Switches {
    int core32_override = -1;       // ABOPT_CORE32: -1 unset, 0, 1
    bool no_split = false;          // ABOPT_CORE_NO_SPLIT
    bool fuse_tail = true;          // ABOPT_FUSE_TAIL=0: core and tail as two launches where the 32-row core runs
    bool x_terms = true;            // ABOPT_X_TERMS=0: no kernel writes x as fp16 terms, every node_frags splits x for itself
    bool fuse_heads = true;         // ABOPT_FUSE_HEADS=0: the heads' geometric epilogue as a launch of its own
    bool fuse_step = true;          // ABOPT_FUSE_STEP=0: a denoising step's transitions and the next evaluation's mixer as launches of their own (abopt_eps_net_step)
    bool fuse_node = true;          // ABOPT_FUSE_NODE=0: every block's node_frags as a launch of its own (no block writes its successor's fragments)
    bool step_rows = true;          // ABOPT_STEP_ROWS=0: the last block of a step streams pair data for every query row, wanted or not (query_rows_masked)
    bool step_compact = true;       // ABOPT_STEP_COMPACT=0: the last block of a step keeps one workgroup per 32 rows, generated or not (query_rows_compact)
};

struct BlockWeights { bool node_frag, out_frag, mlp_frag, out_terms; };     // which packed operands of abopt_ga_weights are given

// A forward by what the choice depends on, and nothing else
struct ForwardQuery {
    int N, L, z_shared, cus;
    bool cache, terms;              // a pair-bias cache / the pair terms of the same pair_feat are given
    bool dbg, dump;                 // abopt_ga_debug is given; it asks for logits or alpha (the dumping core)
    bool feat_out;                  // the core's features are wanted in the caller's buffer
    bool split_ws;                  // key-split scratch is held, of
    size_t split_ws_floats;         // ... this many floats
    int num_blocks;
    BlockWeights blocks[kMaxBlocks];
    bool mix_frag, heads_frag, prmsd;       // network only: w_mix_frag + mix_table, w_heads_frag, the prmsd head
    Switches sw;
    // abopt_eps_net_step only: the forward is followed by the step's transitions; they report the perplexity; the workspace holds this evaluation's mixer output
    // (carry_in: the previous call of the entry wrote it); the next evaluation's is wanted (carry_out)
    bool step = false, ppl = false, carry_in = false, carry_out = false;
    bool frag2 = false;             // the workspace holds a second fragment pair (api.hip: carve_ga aliases it onto proj | feat where it fits)
    bool context_unused = false;    // abopt_eps_net_step with context_outputs_unused or a row list: the caller reads nothing of the network's outputs on rows that are not generated
    int query_row_tiles = 0;        // abopt_eps_net_step with a row list: the caller's list of generated rows fills at most this many 16-row tiles per sample; 0: no list
};

enum class NodeForm { Kernel, Gemm };               // node_frags | projection GEMM + ipa_frags
enum class TailForm { InCore, OutLnMlp, Gemm };     // epilogue of ipa_core32_kernel<true, *> | out_ln_mlp | split-K GEMM + fused_ln_mlp
struct BlockPlan {
    NodeForm node;
    bool qk_terms;                  // node_frags writes the q / k channel slots as fp16 terms: read by ipa_core32_kernel<*, true> and by no other core
    CorePlan core;
    TailForm tail;
    int xt_read, xt_write;          // slot of the workspace's x-terms pair that node_frags reads / the tail writes; -1: none
    // Carried fragments (plan_encoder): the fused kernel of block i (ipa_core32_kernel<true, *, true>) ends by writing block i + 1's fragments from the rows it holds
    bool carry_next = false;        // this block's fused kernel also writes the next block's fragments
    bool carried = false;           // this block's fragments were written by its predecessor: no node_frags launch
    int frag_slot = 0;              // which of the workspace's fragment pairs the block's core reads (and its own node_frags, if it runs, writes)
    // Masked query rows (plan_encoder): the block's output is read on generated rows only, so its fused kernel (ipa_core32_kernel<true, *, false, true>) streams pair
    // data and bias for those rows alone; the other rows of its output are finite and otherwise unspecified
    bool query_rows_masked = false;
    // Gathered query rows (plan_encoder): on top of query_rows_masked, the caller's row list packs the generated rows of a sample into 16-row tiles and the fused
    // kernel (ipa_core32_kernel<true, *, false, true, true>) runs one workgroup per tile -- compact_grid = N tiles of them -- and writes generated rows only
    int query_rows_compact = 0;     // tiles per sample; 0: one workgroup per 32 rows (core.grid)
    unsigned compact_grid = 0;
};
struct EncoderPlan {
    bool ok;                        // false: the last planned block's core is Unsupported and nothing is planned after it
    int num_blocks;
    BlockPlan blocks[kMaxBlocks];
};
struct NetPlan {
    bool mixer_kernel;              // the mixer kernel (with R = exp(v_t) fused) | so3_exp + embed_concat + two GEMMs
    int mixer_xt;                   // slot the mixer writes x's terms to; -1: none
    EncoderPlan enc;
    bool heads_kernel;              // the heads kernel | the GEMM chain
    bool heads_epilogue;            // the geometric epilogue rides in the heads kernel
    bool build_infeat, prmsd;       // build_infeat runs (GEMM heads, or the prmsd head's LayerNorm'd copy); the prmsd chain runs
    bool step_fused;                // abopt_eps_net_step: heads, transitions (and the next mixer) as ONE launch (heads.hip: step_tail_kernel) | heads launch(es) + denoise_step
    bool mixer_launch;              // the mixer step runs at the head of this call (false: carried in by the previous call's fused tail)
    bool step_carry;                // the fused tail also writes the next evaluation's mixer output (x, its terms in slot mixer_xt, R) into the workspace
};

// Whether a second fragment pair fits over proj | feat as the workspace carves them (256-byte carves; api.hip: carve_ga sets ForwardQuery::frag2 from this)
inline bool plan_frag2_fits(size_t proj_floats, size_t feat_floats, size_t kvfrag_floats, size_t qfrag_floats) {
    const auto carve = [](size_t nfloat) { return (nfloat * sizeof(float) + 255) & ~(size_t)255; };
    return carve(kvfrag_floats) + carve(qfrag_floats) <= carve(proj_floats) + carve(feat_floats);
}

inline CoreQuery core_query(const ForwardQuery& q) {
    return {q.N, q.L, q.z_shared, q.cus, q.cache, q.dump, q.split_ws, q.split_ws_floats, q.sw.core32_override, q.sw.no_split};
}

// What abopt_pair_terms_used answers: the cached forward of this geometry takes the 32-row kernels (which alone read the terms), whatever scratch is held
inline bool plan_pair_terms_used(int N, int L, int z_shared, int cus, const Switches& sw) {
    return plan_is_core32({N, L, z_shared, cus, true, false, false, 0, sw.core32_override, sw.no_split});
}

// Whether a step's tail runs as one launch (NetPlan::step_fused).  The two per-sample scalars (prmsd, perplexity) need a reduction across the workgroups of a sample
// in a fixed order: a call that wants either keeps the launches of its own.
inline bool plan_step_fused(const ForwardQuery& q) {
    return q.step && q.mix_frag && q.heads_frag && q.sw.fuse_heads && q.sw.fuse_step && !q.prmsd && !q.ppl;
}

// Block i of the query.  x as fp16 terms travels with x: the block reads the slot its producer wrote (`produced`; -1: none) if its node step is the kernel, and
// writes `next_slot` for a successor whose node step is the kernel -- from one of the two term-writing tails, never the slot it reads
inline BlockPlan plan_block(const ForwardQuery& q, int i, int produced = -1, int next_slot = -1) {
    const BlockWeights& w = q.blocks[i];
    BlockPlan p;
    p.node = w.node_frag ? NodeForm::Kernel : NodeForm::Gemm;
    p.core = plan_ipa_core(core_query(q));
    const bool core32 = p.core.form == CoreForm::Core32 && !q.dbg;        // (Core32 implies a cache and no dump)
    p.qk_terms = core32 && q.terms && w.node_frag;
    p.tail = (core32 && w.out_terms && w.mlp_frag && !q.feat_out && q.sw.fuse_tail) ? TailForm::InCore
           : (w.out_frag && w.mlp_frag) ? TailForm::OutLnMlp : TailForm::Gemm;
    p.xt_read = w.node_frag ? produced : -1;
    const bool writes = q.sw.x_terms && next_slot >= 0 && next_slot != p.xt_read && i + 1 < q.num_blocks && q.blocks[i + 1].node_frag && w.out_frag && w.mlp_frag;
    p.xt_write = writes ? next_slot : -1;
    return p;
}

// Gathered query rows (BlockPlan::query_rows_compact), where the last block's query rows are masked already.  The fused kernel's instruction stream is that of 32
// rows however few of them are wanted; with the generated rows of a sample packed into 16-row tiles a workgroup runs one row tile of the A and C roles and two
// of its four pair waves.  The rule:
//   the caller gave a row list (query_row_tiles > 0) and ABOPT_STEP_COMPACT is not 0;
//   N tiles <= CUs: one round, as the 32-row grid of the same launch would be where it pays most;
//   tiles <= ceil(L / 32): at most half the rows are generated -- from there on the gathered form has as many workgroups as the plain one, each with half
//     the rows (the initial rule: no measured point has moved it yet);
//   three blocks or more: the gathered form writes generated rows only, and the heads read every row of the encoder's output.  Blocks alternate between two
//     output buffers and the last one writes the caller's, so with three blocks or more block num_blocks - 3 of the SAME forward wrote every row of it (finite
//     wherever the forward is); a one- or two-block net would leave the heads whatever the buffer held before the call.
inline bool plan_rows_compact(const ForwardQuery& q, int num_blocks) {
    const int t = q.query_row_tiles;
    return t > 0 && q.sw.step_compact && (int64_t)q.N * t <= q.cus && t <= (q.L + BI2 - 1) / BI2 && num_blocks >= 3;
}

// The blocks of an encoder: block 0's producer wrote `produced` (the mixer; -1: nobody), block i writes slot i & 1.
// Carried fragments: block i + 1 is carried iff block i's tail is InCore (its workgroups end holding their 32 finished rows), block i + 1's node step is the kernel
// (packed weights) and its tail is InCore too (the second fragment pair aliases proj | feat, which only Gemm node steps and out-of-core tails touch), the switch
// is on, the workspace has the second pair and nobody debugs.  A carried block reads the slot its producer wrote, which is NEVER the slot the producer's own
// core reads: other workgroups of the sample are still in their key loops on that one when the first workgroup starts writing.  So slots alternate along a
// chain; block 0 and every uncarried block use slot 0 (their own node_frags writes it behind a launch boundary).
// One round: measured, not structural.  The phase costs a workgroup about 18 us for its 32 rows whatever the batch (the next block's 1.18 MB of weights come from L2 per
// workgroup), the launch keeps its weights in LDS and costs 24 us per 256 workgroups' worth of rows.  Where the fused kernel's workgroups fit the CUs in ONE round (the bench
// shape: 256 on 256) the phase wins by the launch's ramp and boundary; carried over several rounds it lost (N = 64 x L = 256: 2.05 -> 2.23 ms per step, N = 1000 x L = 48:
// 3.70 -> 3.87; profiles/node_carry_shapes.txt), so such a forward is not carried.  DESIGN.md section 3.3 has what is and is not known about the cause.
// Masked query rows: the LAST block's output x feeds the heads and nothing else, and in a step whose tail is fused (plan_step_fused: the heads' outputs go straight
// into the transitions, which keep the old state on every row that is not generated, and no per-sample reduction over all rows -- prmsd, perplexity -- is formed)
// a caller who says it reads none of the network's outputs on those rows (context_unused) cannot tell what x was there.  The block must be the fused 32-row
// kernel on a pair-bias cache that carries nothing (the last block never does).
inline EncoderPlan plan_encoder(const ForwardQuery& q, int produced = -1) {
    EncoderPlan e{true, 0, {}};
    for (int i = 0; i < q.num_blocks && e.ok; ++i) {
        const BlockPlan& p = e.blocks[e.num_blocks++] = plan_block(q, i, produced, i & 1);
        produced = p.xt_write;
        e.ok = p.core.form != CoreForm::Unsupported;
    }
    if (e.ok && e.num_blocks > 0 && q.context_unused && q.sw.step_rows && plan_step_fused(q) && !q.dbg) {
        BlockPlan& last = e.blocks[e.num_blocks - 1];
        last.query_rows_masked = last.core.form == CoreForm::Core32 && q.cache && last.tail == TailForm::InCore && !last.carry_next;
        if (last.query_rows_masked && plan_rows_compact(q, e.num_blocks)) {
            last.query_rows_compact = q.query_row_tiles;
            last.compact_grid = (unsigned)q.N * (unsigned)q.query_row_tiles;
        }
    }
    if (!e.ok || !q.sw.fuse_node || !q.frag2 || q.dbg) return e;
    for (int i = 0; i + 1 < e.num_blocks; ++i) {
        BlockPlan &a = e.blocks[i], &b = e.blocks[i + 1];
        if (a.tail != TailForm::InCore || b.node != NodeForm::Kernel || b.tail != TailForm::InCore) continue;
        if (a.core.grid > (unsigned)q.cus) continue;                        // more than one round of workgroups: node_frags as a launch is the faster form (see above)
        a.carry_next = b.carried = true;
        b.frag_slot = 1 - a.frag_slot;
    }
    return e;
}

inline NetPlan plan_network(const ForwardQuery& q) {
    NetPlan n{};
    n.mixer_kernel = q.mix_frag;
    n.mixer_xt = (q.mix_frag && q.sw.x_terms && q.num_blocks > 0 && q.blocks[0].node_frag) ? 1 : -1;     // slot 1: block 0 writes slot 0 after it has read this one
    n.mixer_launch = true;
    n.enc = plan_encoder(q, n.mixer_xt);
    if (!n.enc.ok) return n;
    n.heads_kernel = q.heads_frag;
    n.heads_epilogue = q.heads_frag && q.sw.fuse_heads;
    n.build_infeat = !q.heads_frag || q.prmsd;
    n.prmsd = q.prmsd;
    // The fused tail of a step (plan_step_fused).  At the time the tail runs, the mixer's outputs are free: x (block 0 alone read it) and x-terms slot mixer_xt
    // (slot 1: the last writer's reader, an even block's node_frags, is long done), R after the epilogue of the same rows has read it.
    n.step_fused = plan_step_fused(q);
    n.mixer_launch = !(n.step_fused && q.carry_in);
    n.step_carry = n.step_fused && q.carry_out;
    return n;
}

}  // namespace abopt
