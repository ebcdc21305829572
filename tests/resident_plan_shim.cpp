// C face of flowgnn_amd/csrc/gcn_plan.h, gat_plan.h, dgn_plan.h and pna_plan.h for tests/resident_plan.py (ctypes).  One case = one 32-bit word of packed inputs,
// one plan = one 32-bit word of packed results; the bit layouts are the field lists of tests/resident_plan.py, in order.
#include <cstdint>

#include "dgn_plan.h"
#include "gat_plan.h"
#include "gcn_plan.h"
#include "pna_plan.h"

namespace {
struct Bits {
    uint32_t w;
    int at = 0;
    bool flag() { return (w >> at++) & 1u; }
    int two() { const int v = (w >> at) & 3u; at += 2; return v; }
};
struct Out {
    uint32_t w = 0;
    int at = 0;
    void put(int v, int bits) { w |= (uint32_t)v << at; at += bits; }
};
}  // namespace

extern "C" {
// cases[i]: GCN_INPUT_FLAGS (one bit each), then num_tasks - 1 (one bit), the index into fills (two bits), pooling (two bits)
void rp_gcn_bulk(const uint32_t* cases, long long n, const double* fills, uint32_t* plans) {
    for (long long i = 0; i < n; i++) {
        Bits b{cases[i]};
        fg::GcnPlanInput in;
        in.resident = b.flag(); in.tile_build = b.flag(); in.binpack = b.flag(); in.split = b.flag(); in.fused = b.flag();
        in.table_ok = b.flag(); in.qmode = b.flag(); in.keep_h = b.flag(); in.exact = b.flag();
        in.tiles = b.flag(); in.bp_lists = b.flag(); in.edge_attr = b.flag(); in.edges = b.flag();
        in.emb = b.flag(); in.node_emb = b.flag(); in.node_logits = b.flag();
        in.num_tasks = 1 + (int)b.flag();
        in.fill = fills[b.two()];
        in.pooling = b.two();
        const fg::GcnPlan p = fg::gcn_plan(in);
        Out o;
        o.put((int)p.path, 2); o.put((int)p.instance, 2);
        o.put(p.needs_csr, 1); o.put(fg::gcn_wants_packed_tile_lists(in), 1); o.put(p.one_pass, 1); o.put(p.bin_packed, 1);
        o.put(p.sum_from_rows, 1); o.put(p.fused_encoder, 1); o.put(p.fused_layers, 1); o.put(p.folded_last, 1); o.put(p.multi_task, 1);
        o.put(p.node_logits_from_scores, 1); o.put(p.pool_rows, 1); o.put(p.node_logits_from_rows, 1);
        plans[i] = o.w;
    }
}

// cases[i]: GAT_INPUT_FLAGS (one bit each), then the index into fills (two bits), pooling (two bits)
void rp_gat_bulk(const uint32_t* cases, long long n, const double* fills, uint32_t* plans) {
    for (long long i = 0; i < n; i++) {
        Bits b{cases[i]};
        fg::GatPlanInput in;
        in.resident = b.flag(); in.fold_readout = b.flag(); in.split = b.flag();
        in.qmode = b.flag(); in.keep_h = b.flag(); in.exact = b.flag();
        in.tiles = b.flag();
        in.emb = b.flag(); in.node_emb = b.flag(); in.node_logits = b.flag(); in.attention = b.flag();
        in.fill = fills[b.two()];
        in.pooling = b.two();
        const fg::GatPlan p = fg::gat_plan(in);
        Out o;
        o.put((int)p.path, 2); o.put((int)p.instance, 2);
        o.put(p.split_products, 1); o.put(p.attention_kernels, 1); o.put(p.fold, 1); o.put(p.pool_rows, 1);
        o.put(p.node_logits_from_scores, 1); o.put(p.node_logits_from_rows, 1);
        plans[i] = o.w;
    }
}

// cases[i]: DGN_INPUT_FLAGS (one bit each), then dgn_mfma_agg + 1, dgn_resident, the index into fills, job_e - (8 job_n - 1) (two bits each)
void rp_dgn_bulk(const uint32_t* cases, long long n, const double* fills, uint32_t* plans) {
    for (long long i = 0; i < n; i++) {
        Bits b{cases[i]};
        fg::DgnPlanInput in;
        in.fused = b.flag(); in.split = b.flag(); in.fold_readout = b.flag(); in.rowinfo_direct = b.flag(); in.binpack = b.flag();
        in.qmode = b.flag(); in.keep_h = b.flag(); in.exact = b.flag();
        in.nonempty = b.flag(); in.eigen = b.flag(); in.tiles = b.flag(); in.bp_lists = b.flag(); in.edges = b.flag(); in.csr_built = b.flag();
        in.emb = b.flag(); in.node_emb = b.flag();
        in.mfma_agg = b.two() - 1;
        in.resident = b.two();
        in.fill = fills[b.two()];
        in.job_n = 1000;  // DGN_JOB_N
        in.job_e = 8 * in.job_n - 1 + b.two();
        const fg::DgnPlan p = fg::dgn_plan(in);
        Out o;
        o.put((int)p.path, 2); o.put((int)p.instance, 2);
        o.put(p.needs_csr, 1); o.put(fg::dgn_wants_packed_tile_lists(in), 1); o.put(p.bin_packed, 1); o.put(p.fused_layers, 1);
        o.put(p.mfma_aggregation, 1); o.put(p.rowinfo_from_edge_list, 1); o.put(p.first_layer_makes_rowinfo, 1); o.put(p.pooled_last, 1);
        o.put(p.prepare_aggregate, 1); o.put(p.edge_scalar, 1); o.put(p.split_dense, 1); o.put(p.emb_readout, 1);
        plans[i] = o.w;
    }
}

// cases[i]: PNA_INPUT_FLAGS (one bit each), then the index into fills (two bits)
void rp_pna_bulk(const uint32_t* cases, long long n, const double* fills, uint32_t* plans) {
    for (long long i = 0; i < n; i++) {
        Bits b{cases[i]};
        fg::PnaPlanInput in;
        in.fused = b.flag(); in.split = b.flag(); in.resident = b.flag(); in.tile_build = b.flag(); in.binpack = b.flag();
        in.qmode = b.flag(); in.keep_h = b.flag(); in.exact = b.flag();
        in.tiles = b.flag(); in.bp_lists = b.flag();
        in.emb = b.flag(); in.node_emb = b.flag();
        in.fill = fills[b.two()];
        const fg::PnaPlan p = fg::pna_plan(in);
        Out o;
        o.put((int)p.path, 2); o.put((int)p.instance, 2);
        o.put(p.needs_csr, 1); o.put(fg::pna_wants_packed_tile_lists(in), 1); o.put(p.one_pass, 1); o.put(p.bin_packed, 1);
        o.put(p.fused_layers, 1); o.put(p.split_dense, 1); o.put(p.emb_readout, 1);
        plans[i] = o.w;
    }
}
}
