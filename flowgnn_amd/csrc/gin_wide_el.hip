// GIN at OGB's default width with OGB's linear edge encoder, the layer of ogbg-ppa (flowgnn_set_edge_linear):
//   a[v] = s_l h[v] + sum over v's in-edges (u, v) of relu(h[u] + W_e e_uv + b_e),   e_uv: F float features, W_e [300][F]
// where every other instance of the layer looks W_e e + b_e up in a 60-row table.
//
// The encoder runs on the matrix pipe inside the in-edge walk.  In gw_layer_body lane (j = lane & 15, g = lane >> 4) walks the in-edges
// of row j of the wave's tile, one per trip, and owns columns 16 t + 4 g .. + 3 of that row for every tile t -- the accumulator layout
// of v_mfma_f32_16x16x32_f16 with the output transposed (tile t's C: lane (j, g) holds rows 4 g .. 4 g + 3 of column j).  So the 16
// edges of a trip, one per row, are the 16 columns of ONE B operand, the A operand of tile t is a fragment of W_e, and the MFMA
// leaves every lane with the embedding of its own edge in its own columns: no shuffle, no LDS round trip.  fp32 accuracy comes from
// the project's split scheme folded into the 32 K slots of that one instruction (F <= 10: 3 F + 2 <= 32):
//   K slot         A (host, times a power of two)   B (the lane's edge)
//   0 .. F-1       w_hi[k]                          e_hi[k]
//   F .. 2F-1      w_hi[k]                          e_lo[k]
//   2F .. 3F-1     w_lo[k]                          e_hi[k]
//   3F, 3F + 1     b_hi, b_lo                       1, 1
//   the rest       0                                0
// A trip is T2 = 19 fragment reads (LDS, 19 KiB per layer, DMA'd where the edge table goes otherwise and resident until the barrier in
// front of the MLP) and 19 MFMAs; the fp32 adds of the walk are what they always were.  A feature at or beyond 6e4 or not finite
// raises *range_flag, and the engine repeats the pass on gw_aggregate_el_kernel (plain fp32 FMAs: also the VALU form of the encoder).
//
// The walk (gw_el_walk, declared in gin_wide_body.h) is defined in gin_wide_el_walk.h, which gin_wide_el_f16.hip includes as well
// (section 4.37).  This file is the one translation unit that instantiates the body with EL = true; gin_wide.hip's, gin_wide_jk.hip's
// and gin_wide_f16.hip's kernels do not contain it.
#include <cmath>

#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "gin_wide_body.h"
#include "gin_wide_el.h"
#include "gin_wide_el_walk.h"  // gw_el_walk
#include "wide_common.h"
#include "wide_el_pack.h"  // GwElBlob and the host packer, which gcn_wide_el.hip shares (section 4.32)

namespace fg {
namespace {

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_layer_el_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                    const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                    const int* __restrict__ eid, const float* __restrict__ ef,
                                                                    const uint8_t* __restrict__ lblob, int el_f,
                                                                    const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                    int n_tot, int relu_out, float self_s, int* __restrict__ range_flag) {
    const float el_inv = *reinterpret_cast<const float*>(lblob + GwElBlob<D>::INV_OFF);
    gw_layer_body<D, GW_PLAIN, false, true>(h, hout, row_ptr, src, nullptr, reinterpret_cast<const float*>(lblob), wchunks, tailp, n_tot, relu_out,
                                            self_s, range_flag, nullptr, nullptr, nullptr, 0, nullptr, nullptr, eid, ef, el_f, el_inv);
}

// the VN instance: x_{l+1}[v] = relu(layer l of x_l)[v] + vn_{l+1}[node_graph[v]], as gw_layer_vn_kernel
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_layer_vn_el_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                       const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                       const int* __restrict__ eid, const float* __restrict__ ef,
                                                                       const uint8_t* __restrict__ lblob, int el_f,
                                                                       const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                       int n_tot, float self_s, int* __restrict__ range_flag,
                                                                       const int* __restrict__ node_graph, const float* __restrict__ vn_add) {
    const float el_inv = *reinterpret_cast<const float*>(lblob + GwElBlob<D>::INV_OFF);
    gw_layer_body<D, GW_VN, false, true>(h, hout, row_ptr, src, nullptr, reinterpret_cast<const float*>(lblob), wchunks, tailp, n_tot, 1, self_s,
                                         range_flag, node_graph, vn_add, nullptr, 0, nullptr, nullptr, eid, ef, el_f, el_inv);
}

// the exact form: gw_aggregate_kernel with the edge term b + sum_k w[k] e[k] as one fma chain, k ascending, W_e read through the caches;
// one lane per (node, float4 piece)
template <int D>
__global__ __launch_bounds__(256) void gw_aggregate_el_kernel(const float* __restrict__ h, float* __restrict__ a, const int* __restrict__ row_ptr,
                                                              const int* __restrict__ src, const int* __restrict__ eid,
                                                              const float* __restrict__ ef, const float* __restrict__ w,
                                                              const float* __restrict__ b, int el_f, int n_tot, float self_s) {
    constexpr int C = D / 4;
    const long long items = (long long)n_tot * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const long long v = i / C;
        const int c = (int)(i - v * C);
        const float4 bias = reinterpret_cast<const float4*>(b)[c];
        const float* wr = w + (size_t)4 * c * el_f;
        float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
        const int e1 = row_ptr[v + 1];
        for (int e = row_ptr[v]; e < e1; e++) {
            const float4 x = reinterpret_cast<const float4*>(h)[(size_t)src[e] * C + c];
            const float* fr = ef + (size_t)eid[e] * el_f;
            float4 t = bias;
            for (int k = 0; k < el_f; k++) {
                const float f = fr[k];
                t.x = __builtin_fmaf(wr[k], f, t.x);
                t.y = __builtin_fmaf(wr[el_f + k], f, t.y);
                t.z = __builtin_fmaf(wr[2 * el_f + k], f, t.z);
                t.w = __builtin_fmaf(wr[3 * el_f + k], f, t.w);
            }
            m.x += relu1(t.x + x.x); m.y += relu1(t.y + x.y); m.z += relu1(t.z + x.z); m.w += relu1(t.w + x.w);
        }
        const float4 x = reinterpret_cast<const float4*>(h)[(size_t)v * C + c];
        reinterpret_cast<float4*>(a)[(size_t)v * C + c] =
            make_float4(__builtin_fmaf(x.x, self_s, m.x), __builtin_fmaf(x.y, self_s, m.y), __builtin_fmaf(x.z, self_s, m.z), __builtin_fmaf(x.w, self_s, m.w));
    }
}

constexpr int GWE_D = FLOWGNN_EMB_DIM_OGB;  // the launchers' one width: the public constant's

inline bool gw_el_args(int emb_dim, int edge_dim) { return emb_dim == GWE_D && edge_dim >= 1 && edge_dim <= FLOWGNN_MAX_EDGE_DIM; }

}  // namespace

size_t gw_el_blob_bytes(int emb_dim, int layers, int edge_dim) {
    return gw_el_args(emb_dim, edge_dim) && layers > 0 ? (size_t)layers * GwElBlob<GWE_D>::layer_stride(edge_dim) : 0;
}

void gw_el_blob_pack(int emb_dim, int layers, int edge_dim, const float* w, const float* b, void* out) {
    if (!gw_el_args(emb_dim, edge_dim)) return;
    constexpr int D = GWE_D;
    for (int l = 0; l < layers; l++)
        gw_el_pack_layer<D>(edge_dim, w + (size_t)l * D * edge_dim, b + (size_t)l * D,
                            static_cast<uint8_t*>(out) + (size_t)l * GwElBlob<D>::layer_stride(edge_dim));
}

int launch_gw_layer_el(int emb_dim, const void* blob, int edge_dim, int l, const float* h, float* hout, const int* row_ptr, const int* src,
                       const int* eid, const float* ef, const uint8_t* wchunks, const float* tailp, int n_tot, int relu_out, float self_s,
                       int* range_flag, const int* node_graph, const float* vn_add, hipStream_t s) {
    if (!gw_el_args(emb_dim, edge_dim)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || l < 0) return FLOWGNN_ERR_ARG;
    if (n_tot <= 0) return 0;
    constexpr int D = GWE_D;
    const uint8_t* const lblob = static_cast<const uint8_t*>(blob) + (size_t)l * GwElBlob<D>::layer_stride(edge_dim);
    const int grid = (int)ceil_div_ll(n_tot, GW_ROWS);
    if (node_graph)
        gw_layer_vn_el_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(h, hout, row_ptr, src, eid, ef, lblob, edge_dim, wchunks, tailp, n_tot, self_s,
                                                                range_flag, node_graph, vn_add);
    else
        gw_layer_el_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(h, hout, row_ptr, src, eid, ef, lblob, edge_dim, wchunks, tailp, n_tot, relu_out,
                                                             self_s, range_flag);
    return 0;
}

int launch_gw_aggregate_el(int emb_dim, const void* blob, int edge_dim, int l, const float* h, float* a, const int* row_ptr, const int* src,
                           const int* eid, const float* ef, int n_tot, float self_s, hipStream_t s) {
    if (!gw_el_args(emb_dim, edge_dim)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || l < 0) return FLOWGNN_ERR_ARG;
    if (n_tot <= 0) return 0;
    constexpr int D = GWE_D;
    using B = GwElBlob<D>;
    const uint8_t* const lblob = static_cast<const uint8_t*>(blob) + (size_t)l * B::layer_stride(edge_dim);
    gw_aggregate_el_kernel<D><<<grid_for((long long)n_tot * (D / 4), 256, 256 * 8), 256, 0, s>>>(
        h, a, row_ptr, src, eid, ef, reinterpret_cast<const float*>(lblob + B::W_OFF), reinterpret_cast<const float*>(lblob + B::b_off(edge_dim)),
        edge_dim, n_tot, self_s);
    return 0;
}

}  // namespace fg
