// gin_wide_el_f16.h -- GIN at width 300 with OGB's linear edge encoder in the walk AND the f16 node MLP behind it
// (flowgnn_set_edge_linear_numeric): the launcher of gin_wide_el_f16.hip's two layer kernels.  The device code
// exists once, in that translation unit; GinWideModel (gin_wide.hip) calls the launcher only while the encoder is on and its numeric
// mode is FLOWGNN_NUMERIC_F16, under a profiler slot of its own.  emb_dim: 300, the one instantiation (anything else:
// FLOWGNN_ERR_UNSUPPORTED).
#pragma once
#include "common.h"

namespace fg {

// Layer l: launch_gw_layer_el's arguments (gin_wide_el.h: the encoder's blob, ef [E][F] in the caller's edge order, eid) with wchunks
// the layer's hi-only stream (GwF16Dims, gin_wide_f16.h) where that launcher takes the split one; tailp is the split stream's tail as
// ever.  a, the hidden units and both matrices are rounded to f16 (to nearest even), one MFMA per product; the encoder stays split
// (fp32-accurate).  node_graph non-null: the virtual-node instance (relu_out is 1 there)
int launch_gw_layer_el_f16(int emb_dim, const void* blob, int edge_dim, int l, const float* h, float* hout, const int* row_ptr, const int* src,
                           const int* eid, const float* ef, const uint8_t* wchunks, const float* tailp, int n_tot, int relu_out, float self_s,
                           int* range_flag, const int* node_graph, const float* vn_add, hipStream_t s);

}  // namespace fg
