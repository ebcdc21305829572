// C face of flowgnn_amd/csrc/pna_plan.h for tests/test_pna_f16_cpu.py (ctypes): the plan of one input with the f16 field, as one word.
// (tests/resident_plan_shim.cpp, the shim of tests/test_resident_plan_cpu.py, never sets that field.)
#include <cstdint>

#include "pna_plan.h"

extern "C" {
// bits of `in`: 0 f16, 1 qmode, 2 exact, 3 split, 4 resident, 5 fused, 6 tiles, 7 keep_h, 8 emb, 9 node_emb
// result: bit 0 single_product, then every other field of the plan (path 2 bits, instance 2 bits, six flags)
uint32_t pna_f16_plan(uint32_t in, double fill) {
    fg::PnaPlanInput i;
    i.f16 = in & 1u; i.qmode = (in >> 1) & 1u; i.exact = (in >> 2) & 1u; i.split = (in >> 3) & 1u;
    i.resident = (in >> 4) & 1u; i.fused = (in >> 5) & 1u; i.tiles = (in >> 6) & 1u; i.keep_h = (in >> 7) & 1u;
    i.emb = (in >> 8) & 1u; i.node_emb = (in >> 9) & 1u;
    i.fill = fill;
    const fg::PnaPlan p = fg::pna_plan(i);
    uint32_t o = p.single_product ? 1u : 0u;
    o |= (uint32_t)p.path << 1;
    o |= (uint32_t)p.instance << 3;
    o |= (uint32_t)p.needs_csr << 5 | (uint32_t)p.one_pass << 6 | (uint32_t)p.bin_packed << 7 | (uint32_t)p.fused_layers << 8 |
         (uint32_t)p.split_dense << 9 | (uint32_t)p.emb_readout << 10;
    return o;
}
}
