// pna_plan.h -- which kernels one PnaModel::forward runs, decided in ONE place from plain values: plain C++ (no HIP, no engine), so a
// CPU test can pin the decision on every input (tests/test_resident_plan_cpu.py).  PnaModel's forward, needs_csr and
// wants_packed_tile_lists read this and nothing else.
#pragma once

namespace fg {

struct PnaPlanInput {
    // options (PnaModel::configure)
    bool fused = true;       // pna_fused: the graph-tile kernels (one launch per layer, or the resident one) may run at all
    bool split = true;       // pna_mfma != 32: the dense products as split-f16 products
    bool resident = true;    // pna_resident
    bool tile_build = true;  // pna_tile_build
    bool binpack = true;     // pna_binpack
    // model state
    bool qmode = false;   // FLOWGNN_NUMERIC_Q6_10
    bool f16 = false;     // FLOWGNN_NUMERIC_F16: the single-product instances of the split kernels (pna_f16.hip)
    bool keep_h = false;  // a per-node tap wants h_4 in HBM (flowgnn_get_h)
    bool exact = false;   // the engine asked for the fp32 pipe after the range flag tripped
    // batch
    bool tiles = false;     // every graph fits a graph tile, and there is one: gtiles.ok && n_tiles > 0
    double fill = 0.0;      // gtiles.fill
    bool bp_lists = false;  // flowgnn_set_batch made the bin-packed tile lists: gtiles.bp_tiles > 0
    // outputs asked for
    bool emb = false, node_emb = false;
};

enum class PnaPath { FixedPoint, Resident, PerLayer };
// the translation unit whose pna_resident_kernel runs: pna.hip, pna_emb.hip, pna_rows.hip (which stores the graph embeddings too)
enum class PnaResidentInstance { Default, Emb, Rows };

struct PnaPlan {
    PnaPath path = PnaPath::PerLayer;
    bool needs_csr = true;  // false: this forward reads the caller's arrays itself (resident, one-pass) and the engine skips the index build
    // ---- the resident path: tile descriptors, then every layer and the readout in one launch
    bool one_pass = false;    // pna_tile_build_kernel, from the caller's arrays (no CSR in HBM); else the CSR + pna_tile_desc_kernel
    bool bin_packed = false;  // ... over the bin-packed tile lists: fewer, fuller tiles of the same graphs
    PnaResidentInstance instance = PnaResidentInstance::Default;
    // ---- the per-layer path
    bool fused_layers = false;  // one graph-tile kernel per layer; else aggregate + dense, two kernels ...
    bool split_dense = false;   // ... the dense one as split-f16 products, else on the fp32 pipe
    bool emb_readout = false;   // the readout also stores the pooled rows
    // ---- either path: the split kernels it runs are their single-product instances (FLOWGNN_NUMERIC_F16).  The path itself is the one
    // the same input takes with f16 off; the fp32 pipe (pna_mfma=32, the exact re-run) has no such instance and runs as it is
    bool single_product = false;
};

// flowgnn_set_batch also bin-packs the graphs into tile lists: asked before there is a batch, so from the options and the model state alone
inline bool pna_wants_packed_tile_lists(const PnaPlanInput& in) { return in.binpack && in.tile_build && in.resident && in.fused && !in.qmode; }

inline PnaPlan pna_plan(const PnaPlanInput& in) {
    PnaPlan p;
    if (in.qmode) {
        p.path = PnaPath::FixedPoint;
        return p;
    }
    // tiles that are mostly empty (graphs of 65..128 nodes) waste MFMA columns: below 40 % full the two-kernel layer is used
    const bool tile_kernels = in.fused && in.split && !in.exact && in.tiles && in.fill >= 0.4;
    p.single_product = in.f16 && in.split && !in.exact;  // (qmode has returned above: it wins over f16)
    // the graph-resident kernel: every layer's h stays in LDS, nothing per node is written (flowgnn_get_h repeats the pass per layer)
    if (in.resident && !in.keep_h && tile_kernels) {
        p.path = PnaPath::Resident;
        p.one_pass = in.tile_build;
        p.needs_csr = !p.one_pass;
        p.bin_packed = p.one_pass && in.binpack && in.bp_lists;
        p.instance = in.node_emb ? PnaResidentInstance::Rows : in.emb ? PnaResidentInstance::Emb : PnaResidentInstance::Default;
        return p;
    }
    p.fused_layers = tile_kernels;
    p.split_dense = !p.fused_layers && in.split && !in.exact;
    p.emb_readout = in.emb;
    return p;
}

}  // namespace fg
