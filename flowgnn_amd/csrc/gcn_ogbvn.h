// gcn_ogbvn.h -- OGB's virtual node for GCN (gnn_type = 'gcn-virtual'; flowgnn_set_gcn_virtual_node).
//
//   vn_0[g] = E
//   layer l:  x_l[v] = h_l[v] + vn_l[g(v)];  h_{l+1} = GCN layer l on x_l  (its linear map W_l x_l + b_l comes FIRST)
//             l < 4:  t = sum_{v in g} x_l[v] + vn_l[g];  vn_{l+1}[g] = relu(W2_l relu(W1_l t + b1_l) + b2_l)     (BatchNorms folded)
// The fused form: h_l lives in the registers of the kernel that projects it (gcn_layer_fused_kernel, gcn.hip), so that kernel's VN
// instance adds vn_l there, in front of the f16 split, and leaves the per-graph sums of x_l as partial rows, one per (16-node tile,
// graph) pair; gcn_ogbvn_update_kernel (gcn_ogbvn.hip) adds a graph's partials and runs the update.  Layer 0: vn_0 = E is a constant,
// folded into the bias (b_0' = b_0 + W_0 E); the VN instance of gcn_encoder_dense_kernel leaves the partial sums of h_0 the same way, and
// the first update forms t = sum_v h_0[v] + (n + 1) E from them.
// The tensors are GIN's (gin_ogbvn.h: the same five, the same device form); so is the in-place form of the configurations that do
// not fuse (launch_gin_ogbvn on the rows in front of each dense launch).
#pragma once
#include "gin_ogbvn.h"

namespace fg {

// what the VN instance of gcn_layer_fused_kernel takes besides the layer's own arguments
struct GcnVnArgs {
    const int* node_graph;  // [N] the graph of every node (launch_gcn_ogbvn_node_graph)
    const float* vn;        // [G][100] vn_l (the encoder's instance: unused, vn_0 is in its bias)
    float* part;            // [(G + n_tiles)][100] partial sums of x_l (the encoder: of h_0), or null: the launch of layer 4, which feeds no update
};
struct GcnNoVnArgs {};

// slots of the partial rows: the pair (tile, graph) has slot graph + tile -- unique, increasing along the batch, and graph g owns the
// contiguous slots g + (node_off[g] >> 4) .. g + ((node_off[g + 1] - 1) >> 4), each written by the one wave that has the tile.
inline size_t gcn_ogbvn_part_floats(int num_graphs, long long n_tot) { return ((size_t)num_graphs + (size_t)((n_tot + 15) / 16)) * GIN_OGBVN_D; }

#ifdef __HIPCC__
// the value of lane - d / lane + d of the same row of 16 lanes (DPP row_shr / row_shl), `old` where the row has no such lane
template <int D>
__device__ __forceinline__ int gcn_ogbvn_row_shr(int x, int old) { return __builtin_amdgcn_update_dpp(old, x, 0x110 + D, 0xf, 0xf, false); }
__device__ __forceinline__ int gcn_ogbvn_row_shl1(int x, int old) { return __builtin_amdgcn_update_dpp(old, x, 0x101, 0xf, 0xf, false); }

template <int D>
__device__ __forceinline__ void gcn_ogbvn_scan_step(float (&s)[25], int gi) {
    const bool take = gcn_ogbvn_row_shr<D>(gi, -2) == gi;  // graphs are contiguous: lane j - D of my graph means every lane between is
#pragma unroll
    for (int k = 0; k < 25; k++) {
        const float y = __builtin_bit_cast(float, gcn_ogbvn_row_shr<D>(__builtin_bit_cast(int, s[k]), 0));
        s[k] = take ? s[k] + y : s[k];
    }
}

// Lane (j, g) of a wave holds x[k], its 25 columns (16 q + 4 g .. + 3 and 96 + g) of node j of 16-node tile `tile`; gi is that node's
// graph, or -1 for a lane without a node (the clamped lanes behind the batch's last node: they add nothing and store nothing).  Per
// graph present in the tile, the column sums over its lanes go to the partial row of slot gi + tile.  A segmented scan along the row
// of 16 lanes, cross-lane moves only, in an order fixed by the lanes' places in the tile; the last lane of a graph stores.
__device__ __forceinline__ void gcn_ogbvn_tile_partials(const float (&x)[25], int gi, int j, int g, long long tile, float* __restrict__ part) {
    float s[25];
#pragma unroll
    for (int k = 0; k < 25; k++) s[k] = gi >= 0 ? x[k] : 0.0f;
    gcn_ogbvn_scan_step<1>(s, gi);
    gcn_ogbvn_scan_step<2>(s, gi);
    gcn_ogbvn_scan_step<4>(s, gi);
    gcn_ogbvn_scan_step<8>(s, gi);
    // (read by EVERY lane, in front of the test on j: a lane that is switched off counts as a lane the row does not have, and behind
    // `j == 15 ||` lane 15 would be off -- lane 14 would take itself for its graph's last and store a sum without lane 15's node)
    const int next_gi = gcn_ogbvn_row_shl1(gi, -2);
    const bool last = j == 15 || next_gi != gi;
    if (gi >= 0 && last) {
        float* pr = part + ((size_t)gi + (size_t)tile) * GIN_OGBVN_D;
#pragma unroll
        for (int q = 0; q < 6; q++)
            *reinterpret_cast<float4*>(pr + 16 * q + 4 * g) = make_float4(s[4 * q + 0], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
        pr[96 + g] = s[24];
    }
}
#endif

// node_graph[v] = the graph of node v, for the n_tot nodes of the batch
void launch_gcn_ogbvn_node_graph(const int* node_off, int num_graphs, int n_tot, int* node_graph, hipStream_t s);

// Update l (0..3): vn_{l+1} into `vn` [num_graphs][100] from the graph's partial rows, added in slot order.  l = 0: they are sums of
// h_0, and t = sum + (n + 1) E (every node's x_0 = h_0 + E, and vn_0 = E once more); l >= 1: of x_l, and t = sum + vn_l (read from `vn`).
// packed: the device form of gin_ogbvn.h.
void launch_gcn_ogbvn_update(const int* node_off, int num_graphs, const float* part, const float* packed, float* vn, int l, hipStream_t s);

// b_0' = b_0 + W_0 E in double (w0 [100][100] row-major by output, b0 [100], E [100])
void gcn_ogbvn_fold_bias(const float* w0, const float* b0, const float* vn_embedding, float* out);

}  // namespace fg
