// gat_plan.h -- which kernels one GatModel::forward runs, decided in ONE place from plain values: plain C++ (no HIP, no engine), so a
// CPU test can pin the decision on every input (tests/test_resident_plan_cpu.py).  As gcn_plan.h.
#pragma once

namespace fg {

struct GatPlanInput {
    // options (GatModel::configure)
    bool resident = true;      // gat_resident
    bool fold_readout = true;  // gat_fold_readout
    bool split = true;         // gat_mfma != 32: the two contractions per layer as split-f16 products
    // model state
    bool qmode = false;   // FLOWGNN_NUMERIC_Q6_10
    bool keep_h = false;  // a per-node tap wants the last layer's rows in HBM (flowgnn_get_h)
    bool exact = false;   // the engine asked for the fp32 pipe after the range flag tripped
    // batch
    bool tiles = false;  // every graph fits a graph tile, and there is one: gtiles.ok && n_tiles > 0
    double fill = 0.0;   // gtiles.fill
    // outputs asked for
    bool emb = false, node_emb = false, node_logits = false;
    bool attention = false;  // attn_mask != 0
    int pooling = 0;         // FLOWGNN_POOL_*: 0 mean, 1 sum, 2 max
};

enum class GatPath { FixedPoint, Resident, PerLayer };
// the translation unit whose gat_resident_kernel runs: gat.hip, gat_poolsum.hip, gat_attn.hip, gat_nlogit.hip
enum class GatResidentInstance { Default, PoolSum, Attention, NodeLogits };

struct GatPlan {
    GatPath path = GatPath::PerLayer;
    // ---- the resident path: all five layers in one launch when the batch packs into graph tiles.  Tiles under half full (graphs of
    // 65..128 nodes) waste MFMA columns, so the per-layer kernels take those; so do per-node taps and the fp32 pipe.  The kernel folds the
    // last layer's skip contraction into the readout and never forms a 16-wide row: graph and node embeddings, and the maximum, are the
    // per-layer path's.  The sum has an instance, but not one that stores attention too
    GatResidentInstance instance = GatResidentInstance::Default;  // (Attention also stores the node logits when those are on)
    // ---- the per-layer path
    bool split_products = false;     // the contractions as split-f16 products, else on the fp32 pipe
    bool attention_kernels = false;  // one gat_attention_kernel per selected layer, from the scores that layer's launch reads
    // the last layer leaves emb[v] . w per node, no 16-wide row.  Not with a pooled or per-node row asked for, and not with the maximum:
    // W . max is not a maximum of per-node scores
    bool fold = false;
    bool pool_rows = false;                // graph embeddings, from the 16-wide rows
    bool node_logits_from_scores = false;  // the folded scores plus the head's bias
    bool node_logits_from_rows = false;    // ... or the head applied to the 16-wide rows
};

inline GatPlan gat_plan(const GatPlanInput& in) {
    GatPlan p;
    if (in.qmode) {
        p.path = GatPath::FixedPoint;
        return p;
    }
    if (in.resident && !in.keep_h && !in.emb && !in.node_emb && in.fold_readout && in.split && !in.exact && in.tiles && in.fill >= 0.5 &&
        (in.pooling == 0 || (in.pooling == 1 && !in.attention))) {
        p.path = GatPath::Resident;
        p.instance = in.pooling == 1 ? GatResidentInstance::PoolSum
                     : in.attention ? GatResidentInstance::Attention
                     : in.node_logits ? GatResidentInstance::NodeLogits
                                      : GatResidentInstance::Default;
        return p;
    }
    p.split_products = in.split && !in.exact;
    p.attention_kernels = in.attention;
    p.fold = in.fold_readout && !in.emb && !in.node_emb && in.pooling != 2;
    p.pool_rows = in.emb;
    p.node_logits_from_scores = in.node_logits && p.fold;
    p.node_logits_from_rows = in.node_logits && !p.fold;
    return p;
}

}  // namespace fg
