// gcn_wide_el_f16.h -- GCN at width 300 with OGB's linear edge encoder in the walk AND the f16 product behind it
// (flowgnn_set_model_edge_linear_numeric): the launcher of gcn_wide_el_f16.hip's two layer kernels.  The device
// code exists once, in that translation unit; GcnWideModel (gcn_wide.hip) calls the launcher only while the encoder is on and its
// numeric mode is FLOWGNN_NUMERIC_F16, under a profiler slot of its own, and never for the last stage (launch_gcw_final_el, which has no
// product).  emb_dim: 300, the one instantiation (anything else: FLOWGNN_ERR_UNSUPPORTED).
#pragma once
#include "common.h"

namespace fg {

// Stage l (not the last): launch_gcw_layer_el's arguments (gcn_wide_el.h: the encoder's blob, ef [E][F] in the caller's edge order, eid,
// the layer's table for its three epilogue rows) with wchunks16 the layer's hi-only stream (GcwF16Dims, gcn_wide_f16.h) where that
// launcher takes the split one; tailp is the split stream's tail as ever.  a and the matrix are rounded to f16 (to nearest even), one
// MFMA per product; the encoder stays split (fp32-accurate).  node_graph non-null: the virtual-node instance (vn, and part or null)
int launch_gcw_layer_el_f16(int emb_dim, const void* blob, int edge_dim, int l, const float* x, float* xout, const int* row_ptr, const int* src,
                            const int* eid, const float* ef, const float* esc, const int* out_deg, const float* tab, const uint8_t* wchunks16,
                            const float* tailp, int n_tot, int* range_flag, const int* node_graph, const float* vn, float* part, hipStream_t s);

}  // namespace fg
