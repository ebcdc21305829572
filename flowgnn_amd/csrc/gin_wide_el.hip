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
// This file defines the walk (gw_el_walk, declared in gin_wide_body.h) and is the one translation unit that instantiates the body
// with EL = true; gin_wide.hip's, gin_wide_jk.hip's and gin_wide_f16.hip's kernels do not contain it.
#include <cmath>

#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "gin_wide_body.h"
#include "gin_wide_el.h"
#include "wide_common.h"
#include "wide_el_pack.h"  // GwElBlob and the host packer, which gcn_wide_el.hip shares (section 4.32)

namespace fg {
namespace {

// The walk.  K index of slot e (0..7) of lane group gk: 16 (e >> 2) + 4 gk + (e & 3), the map of gw_pack_tile.  What a lane's eight
// slots hold is fixed for the launch: which feature (el_foff), and per 32-bit word of the operand which halves take the hi part, the
// lo part or the constant 1 -- so a trip builds its column with eight cached loads, four splits and four mask merges.
template <int D>
__device__ __forceinline__ void gw_el_walk(const float* __restrict__ h, const int* __restrict__ src, const int* __restrict__ eid,
                                           const float* __restrict__ ef, int el_f, float el_inv, const char* s_frag, int e_cur, int e_end,
                                           int lane, float (&bq)[4 * GwDims<D>::Q], float& vmax) {
    using M = GwDims<D>;
    const int g = lane >> 4;
    int foff[8];
    uint32_t m_hi[4] = {0, 0, 0, 0}, m_lo[4] = {0, 0, 0, 0}, m_one[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int kk = 16 * (e >> 2) + 4 * g + (e & 3);
        const int part = kk < el_f ? 0 : kk < 2 * el_f ? 1 : 2;
        foff[e] = kk < 3 * el_f ? kk - part * el_f : 0;  // (a slot beyond 3 F reads feature 0 and masks it away)
        const int sh = 16 * (e & 1);
        if (kk < 3 * el_f) {
            if (part == 1) m_lo[e >> 1] |= 0xffffu << sh;
            else m_hi[e >> 1] |= 0xffffu << sh;
        } else if (kk < 3 * el_f + 2) {
            m_one[e >> 1] |= 0x3c00u << sh;  // f16 1.0: the bias slots
        }
    }
    // the trip count is the wave's longest row: the MFMAs are executed by all 64 lanes, a row with no edge left contributes a zero
    // column and drops what comes back
    while (__any(e_cur < e_end)) {
        const bool act = e_cur < e_end;
        int u = 0;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (act) {
            u = src[e_cur];
            const float* fr = ef + (size_t)eid[e_cur] * el_f;  // the four g groups of a row read the same 4 F bytes
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = fr[foff[e]];
        }
        e_cur++;
        ds_uint4_t b;
        uint32_t bw[4];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            // every feature is slot kk < F of some lane of its row: the range check sees all of them (NaN fails the compare too)
            vmax = (__builtin_fabsf(v[2 * w]) < 6.0e4f && __builtin_fabsf(v[2 * w + 1]) < 6.0e4f) ? vmax : __builtin_inff();
            uint32_t hi, lo;
            DS_SPLIT2(v[2 * w], v[2 * w + 1], hi, lo);
            bw[w] = act ? ((hi & m_hi[w]) | (lo & m_lo[w]) | m_one[w]) : 0u;
        }
        b.x = bw[0]; b.y = bw[1]; b.z = bw[2]; b.w = bw[3];
        const float* hr = h + (size_t)u * D + 4 * g;
#pragma unroll
        for (int q0 = 0; q0 < M::Q; q0 += M::KS1) {
            float4 x[M::KS1];
            if (act) {
#pragma unroll
                for (int q = 0; q < M::KS1; q++)
                    if (16 * (q0 + q) + 4 * g < D) x[q] = *reinterpret_cast<const float4*>(hr + 16 * (q0 + q));
            }
#pragma unroll
            for (int q = 0; q < M::KS1; q++) {
                const int t = q0 + q;
                if (t < M::T2) {  // (compile time: the pieces beyond the last tile do not exist)
                    const ds_uint4_t a = *reinterpret_cast<const ds_uint4_t*>(s_frag + t * 1024 + lane * 16);
                    const float4_t c = DS_MFMA16(a, b, ((float4_t){0.f, 0.f, 0.f, 0.f}));
                    if (act && 16 * t + 4 * g < D) {  // W_e e + b_e = c / scale, exactly; one rounding in the add, as the table path has
                        bq[4 * t + 0] += relu1(__builtin_fmaf(c.x, el_inv, x[q].x));
                        bq[4 * t + 1] += relu1(__builtin_fmaf(c.y, el_inv, x[q].y));
                        bq[4 * t + 2] += relu1(__builtin_fmaf(c.z, el_inv, x[q].z));
                        bq[4 * t + 3] += relu1(__builtin_fmaf(c.w, el_inv, x[q].w));
                    }
                }
            }
        }
    }
}

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
