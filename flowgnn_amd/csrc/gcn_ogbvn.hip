// gcn_ogbvn.hip -- OGB's virtual node for GCN, the launches of its own (gcn_ogbvn.h): the node -> graph map of a batch
// and the per-graph update between two layers.  The add itself and the partial sums are in the VN instance of gcn_layer_fused_kernel
// (gcn.hip); the dense steps are gin_ogbvn_kernel's (ogbvn_dense.h).
//
// One workgroup owns GIN_OGBVN_GPW consecutive graphs.  t of a graph is formed by ONE wave, two row lanes x 25 float4 columns: lane
// (r, c) takes the graph's partial rows r, r + 2, .. in order, the two sums are added r = 0 first.  The partial rows are cut at the batch's 16-node tiles, so t, and with it vn, is a function of the graph AND of where it stands in the
// batch -- the same bits from run to run and for the same batch in any input form, within rounding otherwise.  No atomics.
#include "common.h"
#include "gcn_ogbvn.h"
#include "ogbvn_dense.h"

namespace fg {

namespace {
using namespace ov;

__global__ __launch_bounds__(256) void gcn_ogbvn_node_graph_kernel(const int* __restrict__ node_off, int num_graphs, int n_tot,
                                                                    int* __restrict__ node_graph) {
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < n_tot; v += (long long)gridDim.x * 256) {
        int lo = 0, hi = num_graphs - 1;  // the last graph whose first node is <= v
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (node_off[mid] <= (int)v) lo = mid; else hi = mid - 1;
        }
        node_graph[v] = lo;
    }
}

// FIRST: update 0, the partial rows are sums of h_0 and vn_in is E: t = sum + (n + 1) E; else of x_l: t = sum + vn_l
template <bool FIRST>
__global__ __launch_bounds__(256) void gcn_ogbvn_update_kernel(const int* __restrict__ node_off, int num_graphs,
                                                                const float* __restrict__ part, const float* vn_in,
                                                                float* vn_out /* = vn_in from update 1 on */, const float* __restrict__ wl) {
    __shared__ __attribute__((aligned(16))) float s_w[OV_SLAB];
    __shared__ __attribute__((aligned(16))) float s_t[OV_GPW * OV_D];
    __shared__ __attribute__((aligned(16))) float s_hid[OV_GPW * OV_H];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane / OV_C, c = lane - rl * OV_C;  // row lane 0 / 1 (lanes 50..63: none), float4 column
    const bool active = lane < 2 * OV_C;
    const int g0 = blockIdx.x * OV_GPW;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = wave; s < OV_GPW; s += 4) {
        const int g = g0 + s;
        if (g >= num_graphs) {
            if (lane < OV_C) reinterpret_cast<float4*>(s_t)[s * OV_C + c] = zero4;  // (computed, never stored)
            continue;
        }
        const int r0 = node_off[g], r1 = node_off[g + 1];
        float4 acc = zero4, v = zero4;
        if (active) v = reinterpret_cast<const float4*>(FIRST ? vn_in : vn_in + (size_t)g * OV_D)[c];  // FIRST: E, the same for every graph
        const int lo = g + (r0 >> 4), hi = g + ((r1 - 1) >> 4);  // (a graph without nodes: hi < lo)
        if (active)
            for (int p = lo + rl; p <= hi; p += 2) acc = f4add(acc, reinterpret_cast<const float4*>(part + (size_t)p * OV_D)[c]);
        const float4 other = make_float4(__shfl_down(acc.x, OV_C), __shfl_down(acc.y, OV_C), __shfl_down(acc.z, OV_C), __shfl_down(acc.w, OV_C));
        if (lane < OV_C) {
            float4 t = f4add(acc, other);
            // FIRST: every node's x_0 = h_0 + E, and vn_0 = E once more
            t = FIRST ? ov_fma4(v, (float)(r1 - r0 + 1), t) : f4add(t, v);
            reinterpret_cast<float4*>(s_t)[s * OV_C + c] = t;
        }
    }
    ogbvn_dense_steps(wl, s_w, s_t, s_hid, vn_out, g0, num_graphs, tid);
}
}  // namespace

void launch_gcn_ogbvn_node_graph(const int* node_off, int num_graphs, int n_tot, int* node_graph, hipStream_t s) {
    if (n_tot <= 0 || num_graphs <= 0) return;
    const long long wgs = ceil_div_ll(n_tot, 256);
    gcn_ogbvn_node_graph_kernel<<<(int)(wgs < 4096 ? wgs : 4096), 256, 0, s>>>(node_off, num_graphs, n_tot, node_graph);
}

void launch_gcn_ogbvn_update(const int* node_off, int num_graphs, const float* part, const float* packed, float* vn, int l, hipStream_t s) {
    if (num_graphs <= 0) return;
    const int grid = (num_graphs + OV_GPW - 1) / OV_GPW;
    const float* wl = packed + OV_D + (size_t)l * GIN_OGBVN_LAYER_FLOATS;
    if (l == 0)
        gcn_ogbvn_update_kernel<true><<<grid, 256, 0, s>>>(node_off, num_graphs, part, packed /* E */, vn, wl);
    else
        gcn_ogbvn_update_kernel<false><<<grid, 256, 0, s>>>(node_off, num_graphs, part, vn, vn, wl);
}

void gcn_ogbvn_fold_bias(const float* w0, const float* b0, const float* vn_embedding, float* out) {
    for (int o = 0; o < OV_D; o++) {
        double a = (double)b0[o];
        for (int i = 0; i < OV_D; i++) a += (double)w0[(size_t)o * OV_D + i] * (double)vn_embedding[i];
        out[o] = (float)a;
    }
}

}  // namespace fg
