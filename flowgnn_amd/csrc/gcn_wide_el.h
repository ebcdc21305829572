// gcn_wide_el.h -- GCN at width 300 with OGB's linear edge encoder, the GCNConv of ogbg-ppa (flowgnn_set_model_edge_linear; DESIGN.md
// section 4.32): the device form of the encoder's tensors and the launchers of gcn_wide_el.hip's kernels.  The message of an edge is
// dinv[u] dinv[v] relu(x_u + W_e e_uv + b_e) with e_uv the edge's F float features (1 <= F <= FLOWGNN_MAX_EDGE_DIM), where every other
// stage kernel looks a row of a 60-row table up.  GcnWideModel (gcn_wide.hip) calls the launchers only while the encoder is on: in the
// default state no launch comes from here.  emb_dim: 300, the one instantiation (anything else: 0 bytes / FLOWGNN_ERR_UNSUPPORTED).
#pragma once
#include "common.h"

namespace fg {

// The device form of w [L][D][F] and b [L][D]: GIN's (wide_el_pack.h, gin_wide_el.h), per layer the T fragments | 1 / scale | w | b
size_t gcw_el_blob_bytes(int emb_dim, int layers, int edge_dim);
void gcw_el_blob_pack(int emb_dim, int layers, int edge_dim, const float* w, const float* b, void* out);

// Stage l (not the last) on the matrix pipe: gcw_layer_kernel's arguments with the encoder's blob, the edges' features ef [E][F] in the
// caller's edge order and eid (CSR position -> the caller's edge) where the edge codes go; of `tab`, the layer's table, the three
// epilogue rows are read.  node_graph non-null: the virtual-node instance (vn, and part or null, as GcwVnArgs has them)
int launch_gcw_layer_el(int emb_dim, const void* blob, int edge_dim, int l, const float* x, float* xout, const int* row_ptr, const int* src,
                        const int* eid, const float* ef, const float* esc, const int* out_deg, const float* tab, const uint8_t* wchunks,
                        const float* tailp, int n_tot, int* range_flag, const int* node_graph, const float* vn, float* part, hipStream_t s);

// The last stage: the walk and the epilogue without ReLU and without a product
int launch_gcw_final_el(int emb_dim, const void* blob, int edge_dim, int l, const float* x, float* out, const int* row_ptr, const int* src,
                        const int* eid, const float* ef, const float* esc, const int* out_deg, const float* tab, int n_tot, int* range_flag,
                        hipStream_t s);

// The exact (fp32) form of a stage's aggregate: gcw_aggregate_kernel with the edge term b + sum_k w[k] e[k], one fma chain per column,
// k ascending, CSR order; gw_dense_f32_kernel takes a from there
int launch_gcw_aggregate_el(int emb_dim, const void* blob, int edge_dim, int l, const float* x, float* a, const int* row_ptr, const int* src,
                            const int* eid, const float* ef, const float* esc, const int* out_deg, const float* tab, int n_tot, int relu_out,
                            hipStream_t s);

}  // namespace fg
