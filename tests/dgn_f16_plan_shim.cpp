// C face of flowgnn_amd/csrc/dgn_plan.h for tests/test_dgn_f16_cpu.py (ctypes): the plan of one input with the f16 field, as one word.
// (tests/resident_plan_shim.cpp, the shim of tests/test_resident_plan_cpu.py, never sets that field.)
#include <cstdint>

#include "dgn_plan.h"

extern "C" {
// bits of `in`: 0 f16, 1 qmode, 2 exact, 3 split, 4 fused, 5 tiles, 6 keep_h, 7 emb, 8 node_emb, 9 fold_readout, 10 rowinfo_direct,
// 11 binpack, 12 bp_lists, 13 edges, 14 csr_built, 15 nonempty, 16 eigen; mfma_agg: dgn_mfma_agg (-1, 0, 1); resident: dgn_resident (0, 1, 2);
// dense: job_e = 8 job_n (1) or one edge under it (0)
// result: bit 0 single_product, then every other field of the plan (path 2 bits, instance 2 bits, eleven flags)
uint32_t dgn_f16_plan(uint32_t in, int mfma_agg, int resident, int dense, double fill) {
    fg::DgnPlanInput i;
    i.f16 = in & 1u; i.qmode = (in >> 1) & 1u; i.exact = (in >> 2) & 1u; i.split = (in >> 3) & 1u; i.fused = (in >> 4) & 1u;
    i.tiles = (in >> 5) & 1u; i.keep_h = (in >> 6) & 1u; i.emb = (in >> 7) & 1u; i.node_emb = (in >> 8) & 1u;
    i.fold_readout = (in >> 9) & 1u; i.rowinfo_direct = (in >> 10) & 1u; i.binpack = (in >> 11) & 1u; i.bp_lists = (in >> 12) & 1u;
    i.edges = (in >> 13) & 1u; i.csr_built = (in >> 14) & 1u; i.nonempty = (in >> 15) & 1u; i.eigen = (in >> 16) & 1u;
    i.mfma_agg = mfma_agg; i.resident = resident;
    i.job_n = 1000; i.job_e = dense ? 8000 : 7999;
    i.fill = fill;
    const fg::DgnPlan p = fg::dgn_plan(i);
    uint32_t o = p.single_product ? 1u : 0u;
    o |= (uint32_t)p.path << 1;
    o |= (uint32_t)p.instance << 3;
    o |= (uint32_t)p.needs_csr << 5 | (uint32_t)p.bin_packed << 6 | (uint32_t)p.fused_layers << 7 | (uint32_t)p.mfma_aggregation << 8 |
         (uint32_t)p.rowinfo_from_edge_list << 9 | (uint32_t)p.first_layer_makes_rowinfo << 10 | (uint32_t)p.pooled_last << 11 |
         (uint32_t)p.prepare_aggregate << 12 | (uint32_t)p.edge_scalar << 13 | (uint32_t)p.split_dense << 14 | (uint32_t)p.emb_readout << 15;
    return o;
}
// n inputs in one call (the CPU test sweeps every combination)
void dgn_f16_plan_many(int n, const uint32_t* in, const int32_t* mfma_agg, const int32_t* resident, const int32_t* dense, const double* fill, uint32_t* out) {
    for (int k = 0; k < n; k++) out[k] = dgn_f16_plan(in[k], mfma_agg[k], resident[k], dense[k], fill[k]);
}
// dgn_wants_packed_tile_lists does not move with f16 either
int dgn_f16_wants_packed(uint32_t in, int resident) {
    fg::DgnPlanInput i;
    i.f16 = in & 1u; i.qmode = (in >> 1) & 1u; i.fused = (in >> 4) & 1u; i.binpack = (in >> 11) & 1u; i.resident = resident;
    return fg::dgn_wants_packed_tile_lists(i) ? 1 : 0;
}
}
