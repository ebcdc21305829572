// wide_attn.h -- OGB's graph_pooling="attention" readout at width 300 (flowgnn_set_attention_pooling): the
// gate's device form and the two launches that stand in for gw_pool_rows_kernel in the readout of gin_wide.hip and gcn_wide.hip
// (GwReadout, wide_common.h).
//   s[v] = w2 . relu(W1 r[v] + b1);  pooled[g] = sum_v softmax_g(s)[v] r[v], the sums in node order
// The kernels exist once, in wide_attn.hip; the engine packs the blob through attn_pool_blob_pack and DeviceBatch::attn_pool points
// at its device copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace fg {

// bytes of the device form of (w1 [2D][D], b1 [2D], w2 [2D]) at this width; 0: no kernel of this width
size_t attn_pool_blob_bytes(int emb_dim);
void attn_pool_blob_pack(int emb_dim, const float* w1, const float* b1, const float* w2, void* out);

// s[v] for the n_tot rows (profile slot attn_gate).  exact: the fp32 form, through `hid` [n_tot][2D]; otherwise split-f16 MFMAs, and
// *range_flag is raised when an operand leaves the f16 range
int launch_attn_gate(int emb_dim, const void* blob, const float* rows, float* s_out, float* hid, int n_tot, bool exact, int* range_flag,
                     hipStream_t s);
// pooled[g] from the rows and their gates (profile slot attn_pool_rows); a graph without nodes gets zeros
int launch_attn_pool_rows(int emb_dim, const float* rows, const float* gate, const int* node_off, float* pooled, int num_graphs,
                          hipStream_t s);

}  // namespace fg
