// wide_s2s.h -- OGB's graph_pooling="set2set" readout at width 300 (flowgnn_set_set2set_pooling): the device form
// of its six tensors and the launches that stand in for gw_pool_rows_kernel and launch_pooled_head in the readout of gin_wide.hip and
// gcn_wide.hip (GwReadout, wide_common.h).  Per step t = 1 .. steps, q*_0 = 0, h_0 = c_0 = 0:
//   z = W_ih q*_{t-1} + b_ih + W_hh h_{t-1} + b_hh;  (h_t, c_t) = the LSTM cell of z and c_{t-1}, gates i, f, g, o
//   e[v] = r[v] . h_t[g(v)];  r_t[g] = sum_v softmax_g(e)[v] r[v], the sums in node order;  q*_t = [h_t, r_t]
// and logit[g][k] = head_b[k] + head_W[k] . q*_steps[g].  The softmax-weighted sum is wide_attn.h's launch_attn_pool_rows over e.
// The kernels exist once, in wide_s2s.hip; the engine packs the blob through s2s_blob_pack and DeviceBatch::s2s points at its device copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace fg {

// bytes of the device form of (w_ih [4D][2D], w_hh [4D][D], b_ih [4D], b_hh [4D], head_w [T][2D], head_b [T]); 0: no kernel of this width
size_t s2s_blob_bytes(int emb_dim, int num_tasks);
void s2s_blob_pack(int emb_dim, int num_tasks, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* head_w,
                   const float* head_b, void* out);

// one LSTM step on the num_graphs rows, h and c in place (profile slot s2s_lstm).  first: q*_0 = h_0 = c_0 = 0, so z is the bias and
// neither h, c nor r is read.  exact: the fp32 form, through q [G][2D] and z [G][4D]; otherwise split-f16 MFMAs, and *range_flag is
// raised when an operand leaves the f16 range
int launch_s2s_lstm(int emb_dim, const void* blob, float* h, float* c, const float* r, float* q, float* z, int num_graphs, bool first,
                    bool exact, int* range_flag, hipStream_t s);
// e[v] = rows[v] . h[g(v)] for the nodes of every graph (profile slot s2s_dot_rows)
int launch_s2s_dot_rows(int emb_dim, const float* rows, const float* h, const int* node_off, float* e, int num_graphs, hipStream_t s);
// out[g][k] = head_b[k] + head_w[k] . [h[g], r[g]] (profile slot s2s_head)
int launch_s2s_head(int emb_dim, const void* blob, const float* h, const float* r, float* out, int num_graphs, int num_tasks, hipStream_t s);

}  // namespace fg
