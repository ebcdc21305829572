// gin_wide_vn.h -- OGB's virtual node at width 300, the parts that gcn_wide.hip runs as well (section 4.19):
// the device form of the five tensors (GwVnBlob, gin_wide.hip), the update MLP on G rows t, and the pool and add on rows.  The
// device code exists once, in gin_wide.hip's translation unit; these are its only launchers -- GinWideModel::forward calls them as
// gcn_wide.hip does, each under the caller's own profiler slot.  emb_dim: 300, the one instantiation (anything else: 0 bytes /
// FLOWGNN_ERR_UNSUPPORTED).
#pragma once
#include "common.h"

namespace fg {

// n_updates: the updates the tensors hold, the model's depth - 1 (flowgnn_set_num_layers, section 4.30; 4 at the default depth)
size_t gw_vn_blob_bytes(int emb_dim, int n_updates);
// host tensors E [D], w1 [U][2D][D], b1 [U][2D], w2 [U][D][2D], b2 [U][D], U = n_updates -> gw_vn_blob_bytes(emb_dim, U) bytes at out
void gw_vn_blob_pack(int emb_dim, int n_updates, const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2, void* out);

// vn_next[g] = relu(W2[l] relu(W1[l] t[g] + b1[l]) + b2[l]) for num_graphs rows t; blob: the device form.  exact: the fp32 form
// (gw_dense_f32_kernel twice; hid [num_graphs][2D] is its hidden rows), else gw_vn_update_kernel, which raises *range_flag itself.
// vn_prev non-null (residual=True: GIN, section 4.24, and GCN, section 4.25; null otherwise): vn_next[g] = vn_prev[g * vn_prev_stride] + that,
// one fp32 add, by gin_wide_jk.hip's instance of the update kernel (exact: by its element-wise add); stride in floats, 0 for E.
// n_updates: what the blob was packed with -- l outside 0 .. n_updates - 1 is refused, never read
int launch_gw_vn_update(int emb_dim, const void* blob, int n_updates, int l, const float* t, float* vn_next, float* hid, int num_graphs, bool exact,
                        int* range_flag, const float* vn_prev, int vn_prev_stride, hipStream_t s);
// t[g] = (the rows of graph g in node order) + vn[g * vn_stride]; node_graph non-null: also the node -> graph array (gw_vn_pool_kernel)
int launch_gw_vn_pool(int emb_dim, const float* rows, const int* node_off, const float* vn, int vn_stride, float* t, int* node_graph,
                      int num_graphs, hipStream_t s);
// rows[v] += vn[node_graph[v]] (gw_vn_add_kernel)
int launch_gw_vn_add(int emb_dim, float* rows, const int* node_graph, const float* vn, int n_tot, hipStream_t s);

}  // namespace fg
