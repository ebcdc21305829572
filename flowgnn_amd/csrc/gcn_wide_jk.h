// gcn_wide_jk.h -- GCN at width 300 with OGB's residual=True and JK="sum" (flowgnn_set_model_jk_residual): the
// launchers of gcn_wide_jk.hip's kernels.  The device code exists once, in that translation unit: the instances of gcn_wide_body.h's
// bodies that add and store the pre-linear rows behind the walk.  GcnWideModel (gcn_wide.hip) calls them under the profiler slot of the
// launches they stand in for, and only while the setting is on: in the default state no launch comes from here.  emb_dim: 300, the one
// instantiation (anything else: FLOWGNN_ERR_UNSUPPORTED).
#pragma once
#include "common.h"

namespace fg {

// Stage s = 0..3 of gcn_wide.hip (gcw_layer_kernel; node_graph non-null: gcw_layer_vn_kernel with vn = vn_{s+1} and part, which may be
// null), arguments as there.  x / xout are the POST-linear rows W_s x_s + b_s and W_{s+1} x_{s+1} + b_{s+1}; the rows below are the
// pre-linear ones, [N][D] fp32, and every one of the four may be null:
//   rin        residual: a = relu(pre_s)[v] + rin[v], added before vn[node_graph[v]] (so the partial rows hold it)
//   rout       rout[v] = a, the rows x_{s+1} (after the virtual node's add); may be rin
//   jk_out     jk_out[v] = jk_in[v] + a; jk_in may be jk_out or rin, jk_out is neither rin nor rout
int launch_gcw_layer_jk(int emb_dim, const float* x, float* xout, const int* row_ptr, const int* src, const uint8_t* ecode, const float* esc,
                        const int* out_deg, const float* tab, const uint8_t* wchunks, const float* tailp, int n_tot, int* range_flag,
                        const int* node_graph, const float* vn, float* part, const float* rin, float* rout, const float* jk_in, float* jk_out,
                        hipStream_t s);

// Stage 4 (gcw_final_kernel): out[v] = h_5[v] = pre_4[v] (+ rin[v]); jk_out non-null: jk_out[v] = jk_in[v] + h_5[v] (jk_out is not out)
int launch_gcw_final_jk(int emb_dim, const float* x, float* out, const int* row_ptr, const int* src, const uint8_t* ecode, const float* esc,
                        const int* out_deg, const float* tab, int n_tot, const float* rin, const float* jk_in, float* jk_out, hipStream_t s);

}  // namespace fg
