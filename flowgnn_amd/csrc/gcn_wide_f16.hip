// GCN at OGB's default width in FLOWGNN_NUMERIC_F16 (flowgnn_set_model_numeric_mode_dim): stages 0..3 of
// gcn_wide.hip with both operands of the layer's one product ONE f16 value each, rounded to nearest even, and one MFMA per product.
//
// gcw_layer_f16_body<D, VN, EXT>: a wave owns one 16-node column tile; the walk, the epilogue (root, 1 / (deg + 1), the folded
// BatchNorm, ReLU), the residual add, the virtual node's add with its partial rows and the stores of the pre-linear rows are
// gcn_wide_body.h's own functions, called as gcw_layer_body calls them and in its order -- all fp32, and what they store is the
// unrounded a.  Where that body splits a into hi and lo halves this one rounds it pair by pair (one v_cvt_pk_f16_f32 each) into the B
// operands: no lo registers, KS operand registers fewer times four.  The weights are the hi halves of the split stream, r(W s), and
// nothing else (gcw_pack_layer_f16, gcn_wide.hip): a tile is half as long, so a chunk carries four output tiles where the split
// stream's carries two, in the same two LDS buffers beside the table -- half the steps, half the barriers.  The step count is odd:
// the loop runs pairs of steps on alternating buffers and the last step stands behind it, with nothing in flight.  The chunks go
// L2 -> LDS by LDS-DMA; the only synchronisation is s_waitcnt vmcnt(0) + a workgroup barrier per step, nothing counted.
// Biases (pre-scaled), 1 / s, the range flag at 6e4 (the engine then repeats the pass on the fp32 exact path) are as they were.
// The body is a copy and not an instance of gcw_layer_body: DESIGN.md section 4.21 records that sharing device code between the wide
// files moves their register allocation.
#include <type_traits>

#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "gcn_wide_body.h"  // GcwDims, gcw_walk, gcw_vn_add_partials, gcw_ext_residual, gcw_ext_store, the argument blocks
#include "gcn_wide_f16.h"
#include "wide_common.h"

namespace fg {
namespace {

template <int D>
struct GcwfDims : GcwF16Dims<D> {
    using F = GcwF16Dims<D>;
    using W = GcwDims<D>;  // the walk's: the table, Q
    static_assert(F::KS == W::KS && F::T == W::T, "the two streams cut a product into the same tiles and K-steps");
    static_assert(F::SCALE_AT == W::SCALE_AT, "the tail is the split stream's");
    static_assert(F::STEPS * F::TPC >= F::T, "every output tile has a chunk");
    static_assert(F::CHUNK_BYTES % 1024 == 0, "LDS-DMA moves whole 1 KiB pieces of a chunk");
    static_assert(2 * F::CHUNK_BYTES + W::TAB_BYTES <= 160 * 1024, "two weight buffers and the table must fit the CU's LDS");
};

typedef _Float16 gcwf_half2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t gcwf_pack_rne(float a, float b) {  // to nearest even: one v_cvt_pk_f16_f32
    return __builtin_bit_cast(uint32_t, (gcwf_half2_t){(_Float16)a, (_Float16)b});
}

// the TPC output tiles of chunk c from the fragments in `wb`: one f16 MFMA per product, stored as soon as they are done
template <int D>
__device__ __forceinline__ void gcwf_step(const char* wb, int c, int lane, int g, const ds_uint4_t (&in)[GcwfDims<D>::KS],
                                          const float* __restrict__ tailp, float oscale, float* __restrict__ row, bool valid) {
    using M = GcwfDims<D>;
    float4_t acc[M::TPC];
#pragma unroll
    for (int tl = 0; tl < M::TPC; tl++) {
        const float4 b = *reinterpret_cast<const float4*>(tailp + 16 * (c * M::TPC + tl) + 4 * g);
        acc[tl] = (float4_t){b.x, b.y, b.z, b.w};
    }
#pragma unroll
    for (int ks = 0; ks < M::KS; ks++) {
        ds_uint4_t w[M::TPC];
#pragma unroll
        for (int tl = 0; tl < M::TPC; tl++) w[tl] = *reinterpret_cast<const ds_uint4_t*>(wb + (tl * M::KS + ks) * 1024 + lane * 16);
#pragma unroll
        for (int tl = 0; tl < M::TPC; tl++) acc[tl] = DS_MFMA16(w[tl], in[ks], acc[tl]);
    }
#pragma unroll
    for (int tl = 0; tl < M::TPC; tl++) {
        const int col = 16 * (c * M::TPC + tl) + 4 * g;
        if (col < D && valid) {
            const float4_t r = acc[tl] * oscale;
            *reinterpret_cast<float4*>(row + col) = make_float4(r.x, r.y, r.z, r.w);
        }
    }
}

// xout[v] = W r(a[v]) + b, a[v] = relu(pre[v]) (+ rin[v]) (+ vn[g(v)]): gcw_layer_body (gcn_wide_body.h) with one rounding where it
// splits.  tab: the layer's table; wchunks: the NEXT layer's hi-only stream (GcwF16Dims); tailp: the split stream's tail of that layer.
template <int D, bool VN, bool EXT>
__device__ __forceinline__ void gcw_layer_f16_body(const float* __restrict__ x, float* __restrict__ xout,
                                                   const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                   const uint8_t* __restrict__ ecode, const float* __restrict__ esc,
                                                   const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                   const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                   int n_tot, int* __restrict__ range_flag,
                                                   typename std::conditional<VN, GcwVnArgs, GcwNoVnArgs>::type vna,
                                                   typename std::conditional<EXT, GcwExtArgs, GcwNoExtArgs>::type ext) {
    using M = GcwfDims<D>;
    using W = GcwDims<D>;
    // three DISTINCT LDS objects: the DMA into one weight buffer does not alias the reads of the other, and the table stays
    __shared__ __attribute__((aligned(16))) char s_tab[W::TAB_BYTES];
    __shared__ __attribute__((aligned(16))) char s_w0[M::CHUNK_BYTES];  // the even chunks
    __shared__ __attribute__((aligned(16))) char s_w1[M::CHUNK_BYTES];  // the odd chunks
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const long long node0 = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;
    const bool valid = node0 < n_tot;
    const long long node = valid ? node0 : (long long)n_tot - 1;

    gw_issue_pieces<W::TAB_PIECES>(reinterpret_cast<const uint8_t*>(tab), s_tab, W::TAB_PIECES, W::TAB_LAST_LANES, wave, lane);
    gw_issue_pieces<M::PIECES>(wchunks, s_w0, M::PIECES, 64, wave, lane);  // chunk 0
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    float a[4 * W::Q];
    gcw_walk<D, true>(x, row_ptr, src, ecode, esc, out_deg, reinterpret_cast<const float*>(s_tab), node, valid, g, a);
    if constexpr (EXT) {
        if (ext.rin) gcw_ext_residual<D>(a, ext.rin, node, valid, g);  // (uniform over the launch)
    }
    if constexpr (VN) {
        const int gi = valid ? vna.node_graph[node] : -1;
        gcw_vn_add_partials<D>(a, vna.vn, gi, j, g, (long long)blockIdx.x * GW_WAVES + wave, vna.part);
    }
    float vmax = 0.0f;
#pragma unroll
    for (int k = 0; k < 4 * W::Q; k += 2) vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, __builtin_fabsf(a[k])), __builtin_fabsf(a[k + 1]));
    if constexpr (EXT) gcw_ext_store<D>(a, ext.rout, ext.jk_in, ext.jk_out, node, valid, g);
    ds_uint4_t in[M::KS];
#pragma unroll
    for (int ks = 0; ks < M::KS; ks++) {
        in[ks].x = gcwf_pack_rne(a[8 * ks + 0], a[8 * ks + 1]);
        in[ks].y = gcwf_pack_rne(a[8 * ks + 2], a[8 * ks + 3]);
        in[ks].z = gcwf_pack_rne(a[8 * ks + 4], a[8 * ks + 5]);
        in[ks].w = gcwf_pack_rne(a[8 * ks + 6], a[8 * ks + 7]);
    }
    const float oscale = tailp[M::SCALE_AT];
    float* const row = xout + (size_t)node * D;

    // ---- the product, weights streamed through LDS (chunk 0 has been resident since the first barrier; nobody has touched s_w1).
    // Two steps per trip on alternating buffers; an odd step count leaves the last one behind the loop, on s_w0, whose chunk the
    // trip before it requested and waited for: nothing is in flight there, and nobody writes either buffer again.
#pragma unroll 1
    for (int c = 0; c + 1 < M::STEPS; c += 2) {
        gw_issue_pieces<M::PIECES>(wchunks + (size_t)(c + 1) * M::CHUNK_BYTES, s_w1, M::PIECES, 64, wave, lane);
        gcwf_step<D>(s_w0, c, lane, g, in, tailp, oscale, row, valid);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of chunk c + 1 have landed
        __syncthreads();                                  // everyone's have; everyone is done with s_w0
        if (c + 2 < M::STEPS) gw_issue_pieces<M::PIECES>(wchunks + (size_t)(c + 2) * M::CHUNK_BYTES, s_w0, M::PIECES, 64, wave, lane);
        gcwf_step<D>(s_w1, c + 1, lane, g, in, tailp, oscale, row, valid);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if constexpr (M::STEPS % 2 == 1) gcwf_step<D>(s_w0, M::STEPS - 1, lane, g, in, tailp, oscale, row, valid);
    if (__any(!(vmax < 6.0e4f))) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_layer_f16_kernel(const float* __restrict__ x, float* __restrict__ xout,
                                                                      const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                      const uint8_t* __restrict__ ecode, const float* __restrict__ esc,
                                                                      const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                                      const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                      int n_tot, int* __restrict__ range_flag) {
    gcw_layer_f16_body<D, false, false>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, GcwNoVnArgs{},
                                        GcwNoExtArgs{});
}

// the VN instance: stage s adds vn_{s+1} behind the walk and (s < 3) leaves the partial rows of xin_{s+1}
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_layer_vn_f16_kernel(const float* __restrict__ x, float* __restrict__ xout,
                                                                         const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                         const uint8_t* __restrict__ ecode, const float* __restrict__ esc,
                                                                         const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                                         const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                         int n_tot, int* __restrict__ range_flag, GcwVnArgs vna) {
    gcw_layer_f16_body<D, true, false>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, vna, GcwNoExtArgs{});
}

// the EXT instances: OGB's residual and JK sum behind the walk (section 4.25), on the unrounded a
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_layer_jk_f16_kernel(const float* __restrict__ x, float* __restrict__ xout,
                                                                         const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                         const uint8_t* __restrict__ ecode, const float* __restrict__ esc,
                                                                         const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                                         const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                         int n_tot, int* __restrict__ range_flag, GcwExtArgs ext) {
    gcw_layer_f16_body<D, false, true>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, GcwNoVnArgs{}, ext);
}

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_layer_vn_jk_f16_kernel(const float* __restrict__ x, float* __restrict__ xout,
                                                                            const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                            const uint8_t* __restrict__ ecode, const float* __restrict__ esc,
                                                                            const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                                            const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                            int n_tot, int* __restrict__ range_flag, GcwVnArgs vna, GcwExtArgs ext) {
    gcw_layer_f16_body<D, true, true>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, vna, ext);
}

constexpr int GCWF_D = FLOWGNN_EMB_DIM_OGB;  // the launcher's one width: the public constant's

}  // namespace

int launch_gcw_layer_f16(int emb_dim, const float* x, float* xout, const int* row_ptr, const int* src, const uint8_t* ecode, const float* esc,
                         const int* out_deg, const float* tab, const uint8_t* wchunks, const float* tailp, int n_tot, int* range_flag,
                         const int* node_graph, const float* vn, float* part, const float* rin, float* rout, const float* jk_in, float* jk_out,
                         hipStream_t s) {
    if (emb_dim != GCWF_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (jk_out && (!jk_in || jk_out == rin || jk_out == rout || jk_out == xout)) return FLOWGNN_ERR_ARG;
    if (rout && (rout == xout || rout == x)) return FLOWGNN_ERR_ARG;
    if (node_graph && !vn) return FLOWGNN_ERR_ARG;
    if (n_tot <= 0) return 0;
    constexpr int D = GCWF_D;
    const int grid = (int)ceil_div_ll(n_tot, GW_ROWS);
    const bool ext_on = rin || rout || jk_out;
    const GcwExtArgs ext{rin, rout, jk_in, jk_out};
    if (node_graph && ext_on)
        gcw_layer_vn_jk_f16_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag,
                                                                     GcwVnArgs{node_graph, vn, part}, ext);
    else if (node_graph)
        gcw_layer_vn_f16_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag,
                                                                  GcwVnArgs{node_graph, vn, part});
    else if (ext_on)
        gcw_layer_jk_f16_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, ext);
    else
        gcw_layer_f16_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag);
    return 0;
}

}  // namespace fg
