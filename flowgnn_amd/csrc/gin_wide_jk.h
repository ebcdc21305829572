// gin_wide_jk.h -- GIN at width 300 with OGB's residual=True and JK="sum" (flowgnn_set_jk_residual): the
// launchers of gin_wide_jk.hip's kernels.  The device code exists once, in that translation unit: the instances of gin_wide_body.h's
// and gin_wide_f16_body.h's layer bodies whose epilogues do the two adds, and the element-wise add of the exact (fp32) re-run.
// GinWideModel (gin_wide.hip) calls them under the profiler slots of the launches they stand in for, and only while the setting is
// on: in the default state no launch comes from here.  emb_dim: 300, the one instantiation (anything else: FLOWGNN_ERR_UNSUPPORTED).
#pragma once
#include "common.h"

namespace fg {

// The layer launch of gin_wide.hip (f16 false: the split stream) or of gin_wide_f16.hip (f16 true: the hi-only stream), arguments as
// there; node_graph non-null: the virtual-node instance (relu_out is 1 there).  On top, all fp32:
//   residual      hout[v] = act(layer)[v] + h[v], added before vn_add[node_graph[v]]
//   jk_out        non-null: jk_out[v] = jk_in[v] + hout[v] (what the launch stores).  jk_in: the layer's input rows for layer 0, the
//                 running sum after it; jk_in may be jk_out, and neither may be hout
int launch_gw_layer_jk(int emb_dim, bool f16, const float* h, float* hout, const int* row_ptr, const int* src, const uint8_t* ecode,
                       const float* ecomb, const uint8_t* wchunks, const float* tailp, int n_tot, int relu_out, float self_s, int* range_flag,
                       const int* node_graph, const float* vn_add, bool residual, const float* jk_in, float* jk_out, hipStream_t s);

// The virtual node's update under residual=True: vn_next[g] = vn_prev[g * vn_prev_stride] + relu(W2 relu(W1 t[g] + b1) + b2), one fp32
// add after the ReLU.  wchunks / tailp: the update's split stream and tail (GwVnBlob, gin_wide.hip); vn_prev_stride in floats: D, or
// 0 for layer 0, where every graph's previous vector is E
int launch_gw_vn_update_res(int emb_dim, const float* t, float* vn_next, const uint8_t* wchunks, const float* tailp, int num_graphs,
                            int* range_flag, const float* vn_prev, int vn_prev_stride, hipStream_t s);

// out[v] = a[v] + b[v * b_stride] for n_rows rows of emb_dim floats (b_stride in floats): the exact (fp32) re-run's residual and JK adds
// on the dense kernel's output -- its speed is no goal.  out may be a
int launch_gw_add_rows(int emb_dim, float* out, const float* a, const float* b, int b_stride, int n_rows, hipStream_t s);

}  // namespace fg
