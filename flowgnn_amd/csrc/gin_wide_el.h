// gin_wide_el.h -- GIN at width 300 with OGB's linear edge encoder, the ogbg-ppa form of the layer (flowgnn_set_edge_linear; DESIGN.md
// section 4.31): the device form of the encoder's tensors and the launchers of gin_wide_el.hip's kernels.  The message of an edge is
// relu(x_u + W_e e_uv + b_e) with e_uv the edge's F float features (1 <= F <= FLOWGNN_MAX_EDGE_DIM), where every other layer kernel
// looks a row of a 60-row table up.  GinWideModel (gin_wide.hip) calls the launchers only while the encoder is on: in the default
// state no launch comes from here.  emb_dim: 300, the one instantiation (anything else: 0 bytes / FLOWGNN_ERR_UNSUPPORTED).
#pragma once
#include "common.h"

namespace fg {

// The device form of w [L][D][F] and b [L][D], per layer, in bytes (every part a multiple of 16):
//   T2 fragments of 1 KiB: the A operands of the encoder's MFMA, one per 16-column output tile (the slot table of section 4.31)
//   | 1 / scale, padded to 16 bytes | w [D][F] | b [D]     (the two fp32 parts: the exact form)
size_t gw_el_blob_bytes(int emb_dim, int layers, int edge_dim);
void gw_el_blob_pack(int emb_dim, int layers, int edge_dim, const float* w, const float* b, void* out);

// Layer l on the matrix pipe: gw_layer_kernel's arguments with the encoder's blob, the edges' features ef [E][F] in the caller's edge
// order and eid (CSR position -> the caller's edge) where the edge codes and the table go.  node_graph non-null: the virtual-node
// instance (relu_out is 1 there)
int launch_gw_layer_el(int emb_dim, const void* blob, int edge_dim, int l, const float* h, float* hout, const int* row_ptr, const int* src,
                       const int* eid, const float* ef, const uint8_t* wchunks, const float* tailp, int n_tot, int relu_out, float self_s,
                       int* range_flag, const int* node_graph, const float* vn_add, hipStream_t s);

// The exact (fp32) form's aggregate: a[v] = fma(h[v], self_s, sum over v's in-edges of relu(h[src] + (b + sum_k w[k] e[k]))), one fma
// chain per column, k ascending, CSR order; launch_gw_mlp_f32 takes a from there
int launch_gw_aggregate_el(int emb_dim, const void* blob, int edge_dim, int l, const float* h, float* a, const int* row_ptr, const int* src,
                           const int* eid, const float* ef, int n_tot, float self_s, hipStream_t s);

}  // namespace fg
