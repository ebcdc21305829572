// gin_ogbvn.h -- OGB's virtual node for GIN (flowgnn_set_ogb_virtual_node; kernel and packing: gin_ogbvn.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace fg {

constexpr int GIN_OGBVN_D = 100;        // embedding width
constexpr int GIN_OGBVN_H = 200;        // hidden width of the virtual-node MLP (FLOWGNN_OGB_VN_HIDDEN)
constexpr int GIN_OGBVN_LAYERS = 4;     // updates: between the five GIN layers (FLOWGNN_OGB_VN_LAYERS)
constexpr int GIN_OGBVN_GPW = 16;       // consecutive graphs owned by one workgroup
constexpr int GIN_OGBVN_BIG = 128;      // a graph of more nodes than this is walked by the whole workgroup, not by one wave
// device form of the five tensors: E [100] | per update l: W1^T [100][200] | W2^T [200][100] | b1 [200] | b2 [100]
constexpr size_t GIN_OGBVN_LAYER_FLOATS = (size_t)2 * GIN_OGBVN_D * GIN_OGBVN_H + GIN_OGBVN_H + GIN_OGBVN_D;
constexpr size_t GIN_OGBVN_FLOATS = GIN_OGBVN_D + GIN_OGBVN_LAYERS * GIN_OGBVN_LAYER_FLOATS;  // 161 300, as the file

// host tensors (E [100], w1 [4][200][100], b1 [4][200], w2 [4][100][200], b2 [4][100]) -> the device form, GIN_OGBVN_FLOATS floats
void gin_ogbvn_pack(const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2, float* out);

// Layer l's launch (0..4), in front of that layer's kernel: h[v] += vn_l[g(v)] in place and, for l < 4, vn_{l+1} into `vn`.
// packed: the device form above; vn: [num_graphs][100], read for l >= 1 (vn_0 is E) and written for l < 4.
void launch_gin_ogbvn(float* h, const int* node_off, int num_graphs, const float* packed, float* vn, int l, hipStream_t s);

}  // namespace fg
