// dgn_plan.h -- which kernels one DgnModel::forward runs, decided in ONE place from plain values: plain C++ (no HIP, no engine), so a
// CPU test can pin the decision on every input (tests/test_resident_plan_cpu.py).  DgnModel's forward, needs_csr and
// wants_packed_tile_lists read this and nothing else.
#pragma once

namespace fg {

struct DgnPlanInput {
    // options (DgnModel::configure)
    bool fused = true;           // dgn_fused: the graph-tile kernels (one launch per layer, or the resident one) may run at all
    bool split = true;           // dgn_mfma != 32: the dense products as split-f16 products
    int mfma_agg = -1;           // dgn_mfma_agg: 1 / 0 aggregate on the matrix pipe / by the in-edge walk; -1: by the job's density
    bool fold_readout = true;    // dgn_fold_readout: the last matrix-pipe layer may hand the readout partial sums instead of rows
    bool rowinfo_direct = true;  // dgn_rowinfo_direct: the matrix-pipe layers take the in-edge pass from the caller's edge list
    int resident = 1;            // dgn_resident: 0 never; 1 where the layers would aggregate on the matrix pipe; 2 for every batch that tiles
    bool binpack = true;         // dgn_binpack
    // model state
    bool qmode = false;   // FLOWGNN_NUMERIC_Q6_10
    bool f16 = false;     // FLOWGNN_NUMERIC_F16: the single-product instances of the matrix-pipe kernels (dgn_f16.hip)
    bool keep_h = false;  // a per-node tap wants h_4 in HBM (flowgnn_get_h)
    bool exact = false;   // the engine asked for the fp32 pipe after the range flag tripped
    // batch
    bool nonempty = false;         // n_tot > 0
    bool eigen = false;            // the batch has its eigenvector column: node_eigen != nullptr
    bool tiles = false;            // every graph fits a graph tile, and there is one: gtiles.ok && n_tiles > 0
    double fill = 0.0;             // gtiles.fill
    bool bp_lists = false;         // flowgnn_set_batch made the bin-packed tile lists: gtiles.bp_tiles > 0
    bool edges = false;            // e_tot > 0
    long long job_n = 0, job_e = 0;  // nodes and edges of the whole JOB: every shard of a job takes the same path
    bool csr_built = false;        // an earlier forward of this batch had the engine build the CSR
    // outputs asked for
    bool emb = false, node_emb = false;
};

enum class DgnPath { FixedPoint, Resident, PerLayer };
// the translation unit whose dgn_resident_kernel runs: dgn.hip, dgn_emb.hip, dgn_rows.hip (which stores the graph embeddings too)
enum class DgnResidentInstance { Default, Emb, Rows };

// The plan of a forward that runs.  DgnModel::forward returns before its first launch for an empty batch and for one without the
// eigenvector column: there every flag is clear and the CSR is asked for, as it always was.
// ONE relation ties the two questions the engine and forward ask at different times: needs_csr is asked BEFORE the index build and so
// cannot depend on csr_built; rowinfo_from_edge_list is decided after and does.  rowinfo_from_edge_list implies !needs_csr -- the layer
// kernels read the CSR exactly where the engine was told to build it, or where an earlier forward of this batch had it built.
struct DgnPlan {
    DgnPath path = DgnPath::PerLayer;
    bool needs_csr = true;  // false: this forward takes the graph structure from the caller's edge list and the engine skips the index build
    // ---- the resident path: per-row records from the caller's arrays, then every layer and the readout in one launch
    bool bin_packed = false;  // over the bin-packed tile lists: fewer, fuller tiles of the same graphs
    DgnResidentInstance instance = DgnResidentInstance::Default;
    // ---- the per-layer path
    bool fused_layers = false;               // one graph-tile kernel per layer; else aggregate + dense, two kernels
    bool mfma_aggregation = false;           // ... with both aggregates as MFMAs over the tile's adjacency (dense tiles); else the in-edge walk
    bool rowinfo_from_edge_list = false;     // the matrix-pipe layers' per-row pass runs once, ahead of them, on the caller's edge list: no CSR
    bool first_layer_makes_rowinfo = false;  // ... or the first layer's launch makes and stores it from the CSR
    bool pooled_last = false;        // the last layer keeps its rows on chip: the readout reads per-wave partial sums, and h is not valid after
    bool prepare_aggregate = false;  // the two-kernel layer's row tiles ...
    bool edge_scalar = false;        // ... and eig1[src] per CSR entry (needs an edge)
    bool split_dense = false;        // the two-kernel layer's dense one as split-f16 products, else on the fp32 pipe
    bool emb_readout = false;        // the readout also stores the pooled rows
    // ---- either path: the matrix-pipe kernels it runs (dgn_resident_kernel, dgn_layer_mfma_kernel) are their single-product instances
    // (FLOWGNN_NUMERIC_F16).  Path, instance and every other flag are the ones the same input gets with f16 off; the in-edge walk
    // (dgn_layer_fused_kernel), the two-kernel layer and the fp32 pipe (dgn_mfma=32, the exact re-run) have no such instance and run as they are
    bool single_product = false;
};

// flowgnn_set_batch also bin-packs the graphs into tile lists: asked before there is a batch, so from the options and the model state alone
inline bool dgn_wants_packed_tile_lists(const DgnPlanInput& in) { return in.fused && in.resident != 0 && in.binpack && !in.qmode; }

inline DgnPlan dgn_plan(const DgnPlanInput& in) {
    DgnPlan p;
    if (in.qmode) {
        p.path = DgnPath::FixedPoint;
        return p;
    }
    if (!in.nonempty || !in.eigen) return p;
    // tiles that are mostly empty (graphs of 65..128 nodes) waste MFMA columns: below 40 % full the two-kernel layer is used
    const bool tile_kernels = in.fused && in.split && !in.exact && in.tiles && in.fill >= 0.4;
    // dense tiles (kNN graphs: 16 in-edges per row): both aggregates as MFMAs; sparse ones (molecules, ~2 per row): the in-edge walk
    const bool dense = in.mfma_agg < 0 ? (double)in.job_e >= 8.0 * (double)in.job_n : in.mfma_agg != 0;
    // the graph-resident kernel: every layer's h stays on chip, nothing per node is written (flowgnn_get_h repeats the pass per layer)
    if (in.resident != 0 && !in.keep_h && tile_kernels && (in.resident == 2 || dense)) {
        p.path = DgnPath::Resident;
        p.needs_csr = false;
        p.bin_packed = in.binpack && in.bp_lists;
        p.instance = in.node_emb ? DgnResidentInstance::Rows : in.emb ? DgnResidentInstance::Emb : DgnResidentInstance::Default;
        p.single_product = in.f16;  // (qmode has returned above: it wins over f16; tile_kernels holds split && !exact)
        return p;
    }
    p.fused_layers = tile_kernels;
    p.mfma_aggregation = tile_kernels && dense;
    p.needs_csr = !(p.mfma_aggregation && in.rowinfo_direct);
    p.rowinfo_from_edge_list = !p.needs_csr && !in.csr_built;
    p.first_layer_makes_rowinfo = p.mfma_aggregation && !p.rowinfo_from_edge_list;
    p.pooled_last = p.mfma_aggregation && in.fold_readout && !in.keep_h && !in.node_emb;
    p.prepare_aggregate = !p.fused_layers;
    p.edge_scalar = p.prepare_aggregate && in.edges;
    p.split_dense = p.prepare_aggregate && in.split && !in.exact;
    p.emb_readout = in.emb;
    p.single_product = in.f16 && p.fused_layers && p.mfma_aggregation;
    return p;
}

}  // namespace fg
