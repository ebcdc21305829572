// gcn_plan.h -- which kernels one GcnModel::forward runs, decided in ONE place from plain values: plain C++ (no HIP, no engine), so a
// CPU test can pin the decision on every input (tests/test_resident_plan_cpu.py).  GcnModel's forward, needs_csr,
// wants_packed_tile_lists and aggregation_only read this and nothing else.
#pragma once

namespace fg {

struct GcnPlanInput {
    // options (GcnModel::configure)
    bool resident = true;    // gcn_resident
    bool tile_build = true;  // gcn_tile_build
    bool binpack = true;     // gcn_binpack
    bool split = true;       // gcn_mfma != 32: the dense layers as split-f16 products
    bool fused = true;       // !gcn_unfused
    // model state
    bool table_ok = true;  // the resident walk's scaled messages are exact for these weights (set_weights)
    bool qmode = false;    // FLOWGNN_NUMERIC_Q6_10
    bool keep_h = false;   // a per-node tap wants x_4 in HBM (flowgnn_get_h)
    bool exact = false;    // the engine asked for the fp32 pipe after the range flag tripped
    int num_tasks = 1;
    // batch
    bool tiles = false;      // every graph fits a graph tile, and there is one: gtiles.ok && n_tiles > 0
    double fill = 0.0;       // gtiles.fill
    bool bp_lists = false;   // flowgnn_set_batch made the bin-packed tile lists: gtiles.bp_tiles > 0
    bool edge_attr = false;  // the caller passed edge attributes
    bool edges = false;      // e_tot > 0
    // outputs asked for
    bool emb = false, node_emb = false, node_logits = false;
    int pooling = 0;  // FLOWGNN_POOL_*: 0 mean, 1 sum, 2 max
    // model state, again (the last field: an initialiser list written before it existed means what it meant)
    bool ogb_vn = false;  // OGB's virtual node is on (flowgnn_set_gcn_virtual_node)
};

enum class GcnPath { FixedPoint, Resident, PerLayer };
// the translation unit whose gcn_resident_kernel runs: gcn.hip, gcn_rows.hip, gcn_poolsum.hip, gcn_nlogit.hip
enum class GcnResidentInstance { Default, Rows, PoolSum, NodeLogits };

struct GcnPlan {
    GcnPath path = GcnPath::PerLayer;
    bool needs_csr = true;  // false: this forward reads the caller's arrays itself (resident, one-pass) and the engine skips the index build
    // ---- the resident path: everything in one launch when the batch packs into graph tiles.  Tiles under half full waste MFMA columns, so
    // the per-layer kernels take those; so do per-node taps, the multi-task readout, the fp32 pipe, and the maximum (pooled from rows in HBM)
    bool one_pass = false;    // gcn_tile_build_kernel + the kernel's own encoder (no CSR, no x_0 in HBM); else projected encoder + CSR
    bool bin_packed = false;  // ... over the bin-packed tile lists: fewer, fuller tiles; a row's sums depend on the row alone, so the same bits
    GcnResidentInstance instance = GcnResidentInstance::Default;
    // behind the launch.  The kernel folds the head per node and never forms a pooled row, so every further output comes from the rows the
    // storing instance (Rows) left in HBM -- which is why graph embeddings run here only with node embeddings on
    bool sum_from_rows = false;  // the storing instance's readout is the mean: the sum is taken from its rows
    // ---- the per-layer path
    bool fused_encoder = false;  // x_0 = W_0 (atom encoder) + b_0 in one kernel
    bool fused_layers = false;   // aggregation + dense in one kernel per layer (needs an edge)
    // last stage with the readout's linear head folded in: per-node scores, no rows.  Not with a pooled or per-node row asked for, and
    // not with the maximum: W . max is not a maximum of per-node scores (the sum keeps the fold)
    bool folded_last = false;
    bool multi_task = false;              // NUM_TASK outputs per graph from the un-folded rows
    bool node_logits_from_scores = false; // the folded last stage's scores plus the head's bias
    // OGB's virtual node, on the per-layer path alone (the resident kernel has no instance with it).  true: vn_l is added in the fused
    // kernels' registers and pooled from there (gcn_ogbvn.h); false with the virtual node on: in place on the rows in front of each
    // dense launch, which needs the rows in HBM -- so the encoder fuses only where the layers do
    bool vn_fused = false;
    // ---- either path, from rows in HBM (the storing instance's, or the un-folded last stage's)
    bool pool_rows = false;              // graph embeddings
    bool node_logits_from_rows = false;  // node logits
};

// flowgnn_set_batch also bin-packs the graphs into tile lists: asked before there is a batch, so from the options and the model state alone
inline bool gcn_wants_packed_tile_lists(const GcnPlanInput& in) {
    return in.binpack && in.tile_build && in.resident && !in.qmode && !in.ogb_vn && in.num_tasks == 1;
}

inline GcnPlan gcn_plan(const GcnPlanInput& in) {
    GcnPlan p;
    if (in.qmode) {
        p.path = GcnPath::FixedPoint;
        return p;
    }
    const bool fast = in.split && !in.exact && in.fused;
    if (in.resident && !in.ogb_vn && in.table_ok && !in.keep_h && (!in.emb || in.node_emb) && fast && in.num_tasks == 1 && in.tiles && in.fill >= 0.5 &&
        in.pooling != 2) {
        p.path = GcnPath::Resident;
        p.one_pass = in.tile_build && in.edge_attr;
        p.needs_csr = !p.one_pass;
        p.bin_packed = p.one_pass && in.binpack && in.bp_lists;
        p.instance = in.node_emb ? GcnResidentInstance::Rows
                     : in.pooling == 1 ? GcnResidentInstance::PoolSum
                     : in.node_logits ? GcnResidentInstance::NodeLogits
                                      : GcnResidentInstance::Default;
        p.pool_rows = in.emb;
        p.sum_from_rows = in.node_emb && in.pooling == 1;
        p.node_logits_from_rows = in.node_emb && in.node_logits;
        return p;
    }
    p.fused_layers = fast && in.edges;
    p.fused_encoder = fast && (!in.ogb_vn || p.fused_layers);
    p.vn_fused = in.ogb_vn && p.fused_encoder && p.fused_layers;
    p.folded_last = p.fused_layers && in.num_tasks == 1 && !in.emb && !in.node_emb && in.pooling != 2;
    p.multi_task = !p.folded_last && in.num_tasks > 1;
    p.node_logits_from_scores = p.folded_last && in.node_logits;
    p.pool_rows = in.emb;
    p.node_logits_from_rows = !p.folded_last && in.node_logits;
    return p;
}

}  // namespace fg
