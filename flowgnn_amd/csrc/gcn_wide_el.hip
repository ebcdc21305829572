// GCN at OGB's default width with OGB's linear edge encoder, the GCNConv of ogbg-ppa (flowgnn_set_model_edge_linear; DESIGN.md
// section 4.32):
//   m[v] = sum over v's in-edges (u, v) of dinv[u] dinv[v] relu(x[u] + W_e e_uv + b_e),   e_uv: F float features, W_e [300][F]
// where every other instance of the stage looks W_e e + b_e up in a 60-row table; the epilogue and the product are section 4.18's.
//
// The encoder is section 4.31's: gcw_walk's lane (j = lane & 15, g = lane >> 4) walks the in-edges of row j of the wave's tile and
// owns columns 16 q + 4 g .. + 3, the accumulator layout of v_mfma_f32_16x16x32_f16 with the output transposed, so a trip's 16 edges
// are the 16 columns of ONE B operand, the A operand of tile q is a fragment of W_e, and every lane receives the embedding of its own
// edge in its own columns.  Operand layout, K slots, scaling and packer are GIN's (wide_el_pack.h; the slot table: gin_wide_el.hip).
//
// What is this kernel's own is the trip (gcw_el_trips, gcn_wide_el_walk.h), which keeps the three properties of the table walk:
//   one path     the trip count is the wave's longest row; a lane whose row is done supplies a zero column and norm = 0, and
//                fma(0, finite, a) = a leaves its 76 accumulators alone without a branch around them
//   prefetch     src, dinv[src] and the eight feature words of the NEXT edge are requested while this edge's 19 MFMAs run.  The
//                features hang on eid[e], a second dependent load, so eid runs TWO entries ahead: a trip issues no load whose
//                address it has to wait for
//   one rounding fma(c, 1 / scale, x_u) -> relu -> fma(norm, ., a): the unscaling is exact (a power of two), so the add rounds once,
//                as the table path's w + x does
// LDS: the layer's block (GcwElLds: 19 fragments | 1 / scale | root | BN scale | BN shift, 23 072 bytes) stands where the 75 600-byte
// table stood, beside the two 40 960-byte weight buffers; the final stage holds the block alone.  A feature at or beyond 6e4 or not
// finite raises *range_flag, and the engine repeats the pass on gcw_aggregate_el_kernel (plain fp32 FMAs) and gw_dense_f32_kernel.
//
// The trips are defined in gcn_wide_el_walk.h (declared in gcn_wide_body.h); this is the one translation unit that instantiates the
// bodies with EL = true -- gcn_wide.hip's, gcn_wide_jk.hip's and gcn_wide_f16.hip's kernels do not contain it, and gcn_wide_el_f16.hip
// (section 4.38) has a body of its own behind the same walk.
#include <cmath>

#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "gcn_wide_body.h"
#include "gcn_wide_el.h"
#include "gcn_wide_el_walk.h"  // gcw_el_trips: the walk's trips, shared with gcn_wide_el_f16.hip
#include "wide_common.h"
#include "wide_el_pack.h"

namespace fg {
namespace {

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_layer_el_kernel(const float* __restrict__ x, float* __restrict__ xout,
                                                                     const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                     const int* __restrict__ eid, const float* __restrict__ ef,
                                                                     const uint8_t* __restrict__ lblob, int el_f, const float* __restrict__ esc,
                                                                     const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                                     const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                     int n_tot, int* __restrict__ range_flag) {
    gcw_layer_body<D, false, false, true>(x, xout, row_ptr, src, lblob, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, GcwNoVnArgs{},
                                          GcwNoExtArgs{}, GcwElArgs{eid, ef, el_f, nullptr});
}

// the VN instance: the virtual node's add and the partial rows behind the walk, as gcw_layer_vn_kernel
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_layer_vn_el_kernel(const float* __restrict__ x, float* __restrict__ xout,
                                                                        const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                        const int* __restrict__ eid, const float* __restrict__ ef,
                                                                        const uint8_t* __restrict__ lblob, int el_f, const float* __restrict__ esc,
                                                                        const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                                        const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                        int n_tot, int* __restrict__ range_flag, GcwVnArgs vna) {
    gcw_layer_body<D, true, false, true>(x, xout, row_ptr, src, lblob, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, vna, GcwNoExtArgs{},
                                         GcwElArgs{eid, ef, el_f, nullptr});
}

// out[v] = pre_{L-1}[v]: the last stage, the walk and the epilogue without ReLU and without a product (gcw_final_kernel with the
// encoder's block where the table goes, and the features' range check, which that kernel has no need of)
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_final_el_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                     const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                     const int* __restrict__ eid, const float* __restrict__ ef,
                                                                     const uint8_t* __restrict__ lblob, int el_f, const float* __restrict__ esc,
                                                                     const int* __restrict__ out_deg, const float* __restrict__ tab, int n_tot,
                                                                     int* __restrict__ range_flag) {
    using M = GcwDims<D>;
    __shared__ __attribute__((aligned(16))) char s_blk[GcwElLds<D>::BYTES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const long long node0 = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;
    const bool valid = node0 < n_tot;
    const long long node = valid ? node0 : (long long)n_tot - 1;
    gcw_el_issue_block<D>(lblob, tab, s_blk, wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    float a[4 * M::Q];
    float vmax = 0.0f;
    gcw_walk<D, false, true>(x, row_ptr, src, nullptr, esc, out_deg, reinterpret_cast<const float*>(s_blk), node, valid, g, a,
                             GcwElArgs{eid, ef, el_f, &vmax});
    if (valid) {
        float* row = out + (size_t)node * D + 4 * g;
#pragma unroll
        for (int q = 0; q < M::Q; q++)
            if (16 * q + 4 * g < D) *reinterpret_cast<float4*>(row + 16 * q) = make_float4(a[4 * q + 0], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
    }
    if (__any(!(vmax < 6.0e4f))) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

// the exact form: gcw_aggregate_kernel with the edge term b + sum_k w[k] e[k] as one fma chain, k ascending, W_e read through the
// caches; one lane per (node, float4 piece); tab: the layer's table in global memory, of which the three epilogue rows are read
template <int D>
__global__ __launch_bounds__(256) void gcw_aggregate_el_kernel(const float* __restrict__ x, float* __restrict__ a, const int* __restrict__ row_ptr,
                                                               const int* __restrict__ src, const int* __restrict__ eid,
                                                               const float* __restrict__ ef, const float* __restrict__ w,
                                                               const float* __restrict__ b, int el_f, const float* __restrict__ esc,
                                                               const int* __restrict__ out_deg, const float* __restrict__ tab, int n_tot,
                                                               int relu_out) {
    using M = GcwDims<D>;
    constexpr int C = M::C;
    const float4* const ep = reinterpret_cast<const float4*>(tab + M::ECOMB_FLOATS);
    const long long items = (long long)n_tot * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const long long v = i / C;
        const int c = (int)(i - v * C);
        const int dv = out_deg[v];
        const float dinv_v = dv > 0 ? 1.0f / sqrtf((float)(dv + 1)) : 0.0f;
        const float idp1 = 1.0f / (float)(dv + 1);
        const float4 bias = reinterpret_cast<const float4*>(b)[c];
        const float* wr = w + (size_t)4 * c * el_f;
        float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
        const int e1 = row_ptr[v + 1];
        for (int e = row_ptr[v]; e < e1; e++) {
            const float norm = esc[e] * dinv_v;
            const float4 xv = reinterpret_cast<const float4*>(x)[(size_t)src[e] * C + c];
            const float* fr = ef + (size_t)eid[e] * el_f;
            float4 t = bias;
            for (int k = 0; k < el_f; k++) {
                const float f = fr[k];
                t.x = __builtin_fmaf(wr[k], f, t.x);
                t.y = __builtin_fmaf(wr[el_f + k], f, t.y);
                t.z = __builtin_fmaf(wr[2 * el_f + k], f, t.z);
                t.w = __builtin_fmaf(wr[3 * el_f + k], f, t.w);
            }
            m.x = __builtin_fmaf(norm, relu1(t.x + xv.x), m.x); m.y = __builtin_fmaf(norm, relu1(t.y + xv.y), m.y);
            m.z = __builtin_fmaf(norm, relu1(t.z + xv.z), m.z); m.w = __builtin_fmaf(norm, relu1(t.w + xv.w), m.w);
        }
        const float4 xs = reinterpret_cast<const float4*>(x)[(size_t)v * C + c];
        const float4 rt = ep[c], sc = ep[C + c], sh = ep[2 * C + c];
        float4 r;
        r.x = __builtin_fmaf(__builtin_fmaf(relu1(xs.x + rt.x), idp1, m.x), sc.x, sh.x);
        r.y = __builtin_fmaf(__builtin_fmaf(relu1(xs.y + rt.y), idp1, m.y), sc.y, sh.y);
        r.z = __builtin_fmaf(__builtin_fmaf(relu1(xs.z + rt.z), idp1, m.z), sc.z, sh.z);
        r.w = __builtin_fmaf(__builtin_fmaf(relu1(xs.w + rt.w), idp1, m.w), sc.w, sh.w);
        if (relu_out) { r.x = relu1(r.x); r.y = relu1(r.y); r.z = relu1(r.z); r.w = relu1(r.w); }
        reinterpret_cast<float4*>(a)[(size_t)v * C + c] = r;
    }
}

constexpr int GCWE_D = FLOWGNN_EMB_DIM_OGB;  // the launchers' one width: the public constant's
static_assert(GwElBlob<GCWE_D>::T == GcwDims<GCWE_D>::T, "the encoder's fragments are the walk's 16-column pieces");

inline bool gcw_el_args(int emb_dim, int edge_dim) { return emb_dim == GCWE_D && edge_dim >= 1 && edge_dim <= FLOWGNN_MAX_EDGE_DIM; }

inline const uint8_t* gcw_el_layer(const void* blob, int edge_dim, int l) {
    return static_cast<const uint8_t*>(blob) + (size_t)l * GwElBlob<GCWE_D>::layer_stride(edge_dim);
}

}  // namespace

size_t gcw_el_blob_bytes(int emb_dim, int layers, int edge_dim) {
    return gcw_el_args(emb_dim, edge_dim) && layers > 0 ? (size_t)layers * GwElBlob<GCWE_D>::layer_stride(edge_dim) : 0;
}

void gcw_el_blob_pack(int emb_dim, int layers, int edge_dim, const float* w, const float* b, void* out) {
    if (!gcw_el_args(emb_dim, edge_dim)) return;
    constexpr int D = GCWE_D;
    for (int l = 0; l < layers; l++)
        gw_el_pack_layer<D>(edge_dim, w + (size_t)l * D * edge_dim, b + (size_t)l * D,
                            static_cast<uint8_t*>(out) + (size_t)l * GwElBlob<D>::layer_stride(edge_dim));
}

int launch_gcw_layer_el(int emb_dim, const void* blob, int edge_dim, int l, const float* x, float* xout, const int* row_ptr, const int* src,
                        const int* eid, const float* ef, const float* esc, const int* out_deg, const float* tab, const uint8_t* wchunks,
                        const float* tailp, int n_tot, int* range_flag, const int* node_graph, const float* vn, float* part, hipStream_t s) {
    if (!gcw_el_args(emb_dim, edge_dim)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || l < 0) return FLOWGNN_ERR_ARG;
    if (n_tot <= 0) return 0;
    constexpr int D = GCWE_D;
    const uint8_t* const lblob = gcw_el_layer(blob, edge_dim, l);
    const int grid = (int)ceil_div_ll(n_tot, GW_ROWS);
    if (node_graph)
        gcw_layer_vn_el_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(x, xout, row_ptr, src, eid, ef, lblob, edge_dim, esc, out_deg, tab, wchunks, tailp, n_tot,
                                                                 range_flag, GcwVnArgs{node_graph, vn, part});
    else
        gcw_layer_el_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(x, xout, row_ptr, src, eid, ef, lblob, edge_dim, esc, out_deg, tab, wchunks, tailp, n_tot,
                                                              range_flag);
    return 0;
}

int launch_gcw_final_el(int emb_dim, const void* blob, int edge_dim, int l, const float* x, float* out, const int* row_ptr, const int* src,
                        const int* eid, const float* ef, const float* esc, const int* out_deg, const float* tab, int n_tot, int* range_flag,
                        hipStream_t s) {
    if (!gcw_el_args(emb_dim, edge_dim)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || l < 0) return FLOWGNN_ERR_ARG;
    if (n_tot <= 0) return 0;
    constexpr int D = GCWE_D;
    gcw_final_el_kernel<D><<<(int)ceil_div_ll(n_tot, GW_ROWS), GW_WAVES * 64, 0, s>>>(x, out, row_ptr, src, eid, ef, gcw_el_layer(blob, edge_dim, l), edge_dim,
                                                                                      esc, out_deg, tab, n_tot, range_flag);
    return 0;
}

int launch_gcw_aggregate_el(int emb_dim, const void* blob, int edge_dim, int l, const float* x, float* a, const int* row_ptr, const int* src,
                            const int* eid, const float* ef, const float* esc, const int* out_deg, const float* tab, int n_tot, int relu_out,
                            hipStream_t s) {
    if (!gcw_el_args(emb_dim, edge_dim)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || l < 0) return FLOWGNN_ERR_ARG;
    if (n_tot <= 0) return 0;
    constexpr int D = GCWE_D;
    using B = GwElBlob<D>;
    const uint8_t* const lblob = gcw_el_layer(blob, edge_dim, l);
    gcw_aggregate_el_kernel<D><<<grid_for((long long)n_tot * (D / 4), 256, 256 * 8), 256, 0, s>>>(
        x, a, row_ptr, src, eid, ef, reinterpret_cast<const float*>(lblob + B::W_OFF), reinterpret_cast<const float*>(lblob + B::b_off(edge_dim)), edge_dim,
        esc, out_deg, tab, n_tot, relu_out);
    return 0;
}

}  // namespace fg
