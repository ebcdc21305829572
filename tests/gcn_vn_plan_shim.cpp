// C face of flowgnn_amd/csrc/gcn_plan.h with its ogb_vn field, for tests/test_gcn_vn_cpu.py (ctypes): tests/resident_plan_shim.cpp's
// rp_gcn_bulk with one more argument and one more result bit.  The case words and the first sixteen result bits are laid out as there
// (the field lists of tests/resident_plan.py, in order), so the two shims' plans compare word for word.
#include <cstdint>

#include "gcn_plan.h"

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
// ogb_vn < 0: the field is left as GcnPlanInput initialises it
void gvp_gcn_bulk(const uint32_t* cases, long long n, const double* fills, int ogb_vn, uint32_t* plans) {
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
        if (ogb_vn >= 0) in.ogb_vn = ogb_vn != 0;
        const fg::GcnPlan p = fg::gcn_plan(in);
        Out o;
        o.put((int)p.path, 2); o.put((int)p.instance, 2);
        o.put(p.needs_csr, 1); o.put(fg::gcn_wants_packed_tile_lists(in), 1); o.put(p.one_pass, 1); o.put(p.bin_packed, 1);
        o.put(p.sum_from_rows, 1); o.put(p.fused_encoder, 1); o.put(p.fused_layers, 1); o.put(p.folded_last, 1); o.put(p.multi_task, 1);
        o.put(p.node_logits_from_scores, 1); o.put(p.pool_rows, 1); o.put(p.node_logits_from_rows, 1);
        o.put(p.vn_fused, 1);
        plans[i] = o.w;
    }
}
}
