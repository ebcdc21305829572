// gin_ogbvn.hip -- OGB's virtual node for GIN (gnn_type = 'gin-virtual'; flowgnn_set_ogb_virtual_node).
//
// OGB keeps one vector per graph beside the nodes (ogb/examples/graphproppred/mol/conv.py, GNN_node_Virtualnode):
//   vn_0[g] = E
//   layer l:  x_l[v] = h_l[v] + vn_l[g(v)];  h_{l+1} = GIN layer l on x_l
//             l < 4:  t = sum_{v in g} x_l[v] + vn_l[g];  vn_{l+1}[g] = relu(W2_l relu(W1_l t + b1_l) + b2_l)     (BatchNorms folded)
// One launch per layer in front of that layer's kernel, in place on the layer's input rows.  A workgroup owns GIN_OGBVN_GPW
// consecutive graphs: it adds vn_l to their rows, sums the rows it has just written per column, and (l < 4) runs the two dense steps
// for its graphs on the vector ALUs with the weights staged through LDS in slabs that all its graphs share.  A graph's vector is
// read and written by this one workgroup, so vn_{l+1} replaces vn_l in the same [G][100] buffer.
//
// Every summation order is a function of the graph's own node count: a graph of at most GIN_OGBVN_BIG nodes is walked by ONE wave
// (two row lanes x 25 float4 columns: lane (r, c) takes rows r, r + 2, .. in order, the two partial sums are added r = 0 first), a
// larger one by the four waves (eight row lanes; the four wave sums are added wave 0 first); a dot product is one FMA chain over k
// ascending that starts from the bias.  No atomics.  So a graph's vector has the same bits wherever the graph stands in a batch.
#include "gin_ogbvn.h"
#include "ogbvn_dense.h"

namespace fg {

namespace {
using namespace ov;

// rows r, r + step, .. < r_end of column chunk c: x = h + v written back, and (SUM) added up in that order
template <bool SUM>
__device__ __forceinline__ float4 ov_rows(float4* __restrict__ h4, int r, int r_end, int step, int c, float4 v) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (; r + 3 * step < r_end; r += 4 * step) {  // four rows in flight
        float4* p0 = h4 + (size_t)r * OV_C + c;
        float4* p1 = p0 + (size_t)step * OV_C;
        float4* p2 = p1 + (size_t)step * OV_C;
        float4* p3 = p2 + (size_t)step * OV_C;
        float4 x0 = *p0, x1 = *p1, x2 = *p2, x3 = *p3;
        x0 = f4add(x0, v); x1 = f4add(x1, v); x2 = f4add(x2, v); x3 = f4add(x3, v);
        *p0 = x0; *p1 = x1; *p2 = x2; *p3 = x3;
        if (SUM) { acc = f4add(acc, x0); acc = f4add(acc, x1); acc = f4add(acc, x2); acc = f4add(acc, x3); }
    }
    for (; r < r_end; r += step) {
        float4* p = h4 + (size_t)r * OV_C + c;
        const float4 x = f4add(*p, v);
        *p = x;
        if (SUM) acc = f4add(acc, x);
    }
    return acc;
}

__device__ __forceinline__ float4 ov_shfl_down(float4 a, int d) {
    return make_float4(__shfl_down(a.x, d), __shfl_down(a.y, d), __shfl_down(a.z, d), __shfl_down(a.w, d));
}
}  // namespace

// UPDATE = false: the last layer's launch, the add alone
template <bool UPDATE>
__global__ __launch_bounds__(256) void gin_ogbvn_kernel(float* __restrict__ h, const int* __restrict__ node_off, int num_graphs,
                                                         const float* vn_in, int vn_in_stride,  // stride 0: vn_0 = E for every graph
                                                         float* vn_out /* = vn_in from layer 1 on */, const float* __restrict__ wl) {
    __shared__ __attribute__((aligned(16))) float s_w[UPDATE ? OV_SLAB : 4];
    __shared__ __attribute__((aligned(16))) float s_t[UPDATE ? OV_GPW * OV_D : 4];
    __shared__ __attribute__((aligned(16))) float s_hid[UPDATE ? OV_GPW * OV_H : 4];
    __shared__ __attribute__((aligned(16))) float s_wp[UPDATE ? 4 * OV_D : 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane / OV_C, c = lane - rl * OV_C;  // row lane 0 / 1 (lanes 50..63: none), float4 column
    const bool active = lane < 2 * OV_C;
    const int g0 = blockIdx.x * OV_GPW;
    float4* h4 = reinterpret_cast<float4*>(h);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // ---- steps 1 + 2, graphs of at most GIN_OGBVN_BIG nodes: one wave each, no workgroup barrier
    for (int s = wave; s < OV_GPW; s += 4) {
        const int g = g0 + s;
        if (g >= num_graphs) {
            if (UPDATE && lane < OV_C) reinterpret_cast<float4*>(s_t)[s * OV_C + c] = zero4;  // (computed, never stored)
            continue;
        }
        const int r0 = node_off[g], r1 = node_off[g + 1];
        if (r1 - r0 > GIN_OGBVN_BIG) continue;
        float4 v = zero4;
        if (active) v = reinterpret_cast<const float4*>(vn_in + (size_t)g * vn_in_stride)[c];
        float4 acc = zero4;
        if (active) acc = ov_rows<UPDATE>(h4, r0 + rl, r1, 2, c, v);
        if (UPDATE) {
            const float4 hi = ov_shfl_down(acc, OV_C);  // row lane 1's partial sum
            if (lane < OV_C) reinterpret_cast<float4*>(s_t)[s * OV_C + c] = f4add(f4add(acc, hi), v);
        }
    }
    // ---- ... and the larger ones: the four waves together (eight row lanes)
    for (int s = 0; s < OV_GPW; s++) {
        const int g = g0 + s;
        if (g >= num_graphs) break;
        const int r0 = node_off[g], r1 = node_off[g + 1];
        if (r1 - r0 <= GIN_OGBVN_BIG) continue;  // (uniform over the workgroup: the barriers below are safe)
        float4 v = zero4;
        if (active) v = reinterpret_cast<const float4*>(vn_in + (size_t)g * vn_in_stride)[c];
        float4 acc = zero4;
        if (active) acc = ov_rows<UPDATE>(h4, r0 + 2 * wave + rl, r1, 8, c, v);
        if (UPDATE) {
            const float4 hi = ov_shfl_down(acc, OV_C);
            if (lane < OV_C) reinterpret_cast<float4*>(s_wp)[wave * OV_C + c] = f4add(acc, hi);
            __syncthreads();
            if (tid < OV_C) {
                const float4* wp = reinterpret_cast<const float4*>(s_wp);
                float4 t = f4add(wp[tid], wp[OV_C + tid]);
                t = f4add(t, wp[2 * OV_C + tid]);
                t = f4add(t, wp[3 * OV_C + tid]);
                reinterpret_cast<float4*>(s_t)[s * OV_C + tid] = f4add(t, v);  // (tid < 25: wave 0, row lane 0, c = tid)
            }
            __syncthreads();
        }
    }
    if (!UPDATE) return;

    // ---- steps 3 + 4: hid = relu(W1 t + b1), vn' = relu(W2 hid + b2) for the workgroup's graphs (ogbvn_dense.h)
    ogbvn_dense_steps(wl, s_w, s_t, s_hid, vn_out, g0, num_graphs, tid);
}

void gin_ogbvn_pack(const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2, float* out) {
    for (int d = 0; d < OV_D; d++) out[d] = vn_embedding[d];
    for (int l = 0; l < GIN_OGBVN_LAYERS; l++) {
        float* o = out + OV_D + (size_t)l * GIN_OGBVN_LAYER_FLOATS;
        const float* W1 = w1 + (size_t)l * OV_H * OV_D;  // [200][100]
        const float* W2 = w2 + (size_t)l * OV_D * OV_H;  // [100][200]
        for (int k = 0; k < OV_D; k++)
            for (int u = 0; u < OV_H; u++) o[(size_t)k * OV_H + u] = W1[(size_t)u * OV_D + k];
        o += (size_t)OV_D * OV_H;
        for (int k = 0; k < OV_H; k++)
            for (int d = 0; d < OV_D; d++) o[(size_t)k * OV_D + d] = W2[(size_t)d * OV_H + k];
        o += (size_t)OV_D * OV_H;
        for (int u = 0; u < OV_H; u++) o[u] = b1[(size_t)l * OV_H + u];
        for (int d = 0; d < OV_D; d++) o[OV_H + d] = b2[(size_t)l * OV_D + d];
    }
}

void launch_gin_ogbvn(float* h, const int* node_off, int num_graphs, const float* packed, float* vn, int l, hipStream_t s) {
    if (num_graphs <= 0) return;
    const int grid = (num_graphs + OV_GPW - 1) / OV_GPW;
    const float* vn_in = l == 0 ? packed : vn;  // vn_0 = E
    const int stride = l == 0 ? 0 : OV_D;
    if (l < GIN_OGBVN_LAYERS)
        gin_ogbvn_kernel<true><<<grid, 256, 0, s>>>(h, node_off, num_graphs, vn_in, stride, vn, packed + OV_D + (size_t)l * GIN_OGBVN_LAYER_FLOATS);
    else
        gin_ogbvn_kernel<false><<<grid, 256, 0, s>>>(h, node_off, num_graphs, vn_in, stride, nullptr, nullptr);
}

}  // namespace fg
