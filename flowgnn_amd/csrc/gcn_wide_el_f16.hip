// GCN at OGB's default width with OGB's linear edge encoder in the walk and the f16 product behind it: the stage of ogbg-ppa's gcn and
// gcn-virtual in its throughput mode (flowgnn_set_model_edge_linear_numeric).
//   m[v]    = sum over v's in-edges (u, v) of dinv[u] dinv[v] relu(x[u] + W_e e_uv + b_e)      fp32, CSR order: gcw_el_trips, unchanged
//   a[v]    = relu(BN(m[v] + relu(x[v] + root) / (deg(v) + 1))) (+ vn[g(v)])                    fp32: gcw_walk's epilogue, gcw_vn_add_partials
//   xout[v] = W r(a[v]) + b                                                                     r: to f16, nearest even (section 4.27)
//
// gcw_layer_el_f16_kernel<D> / gcw_layer_vn_el_f16_kernel<D>: stages 0 .. L - 2 while the encoder is on.  A wave owns one 16-node column
// tile.  The walk is gcn_wide_el.hip's own function (gcn_wide_el_walk.h): per trip one B operand out of the 16 rows' edges, T = 19
// fragment reads and 19 MFMAs whose split K slots keep the encoder fp32-accurate; the epilogue, the virtual node's add and its partial
// rows are gcn_wide_body.h's.  What follows is gcn_wide_f16.hip's arithmetic: a rounded pair by pair into the B operands (no lo
// registers: `in` is KS = 10 operand registers times four, not twenty), then per step KS x TPC = 40 MFMAs on the hi-only weight stream
// r(W s), four output tiles at a time, fp32 accumulators that start at the pre-scaled bias and leave through 1 / s.
//
// LDS, three distinct objects, 104 992 bytes: the encoder's block (GcwElLds: 19 fragments | 1 / scale | root | BN scale | BN shift,
// 23 072 B) where the 75 600-byte table stood, and the two 40 960-byte weight buffers of GcwF16Dims.  The block, chunk 0 AND chunk 1 are
// requested together in front of ONE s_waitcnt vmcnt(0) and ONE barrier (the block is 52 KB smaller than the table, so a second
// buffer's worth of requests costs the first wait little), and nothing is in flight while the walk runs (a request made there would be drained by the compiler's own waits in front of the walk's
// loads, section 4.22).  Both buffers are resident when the product starts, so steps 0 and 1 have only a barrier between them -- it
// orders the readers of s_w0 in front of chunk 2's request, the loop's first -- and no wait: the wave has no request outstanding there.
// From then on one s_waitcnt vmcnt(0) and one workgroup barrier per step, as in gcn_wide_f16.hip; the odd fifth step stands behind the
// loop, on s_w0, with nothing in flight.
//
// fp32 and gcn_wide.hip's: the biases (pre-scaled), 1 / s, everything in front of the rounding.  The range flag is raised by an a or an
// edge feature at or beyond 6e4 or not finite; the engine then repeats the pass on the fp32 exact path (launch_gcw_aggregate_el +
// launch_gw_dense_f32).  The body is this file's own and not an EL flag on gcw_layer_f16_body: sections 4.21 and 4.22 record that a
// body shared between the wide files moves their register allocation.
#include <type_traits>

#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "gcn_wide_body.h"     // GcwDims, GcwElLds, gcw_walk, gcw_el_issue_block, gcw_vn_add_partials, the argument blocks
#include "gcn_wide_el_f16.h"
#include "gcn_wide_el_walk.h"  // gcw_el_trips
#include "gcn_wide_f16.h"      // GcwF16Dims: the hi-only stream
#include "wide_common.h"       // GW_WAVES / GW_ROWS, the LDS-DMA issue
#include "wide_el_pack.h"      // GwElBlob: a layer's part of the encoder's blob

namespace fg {
namespace {

template <int D>
struct GcwElF16Dims : GcwF16Dims<D> {
    using F = GcwF16Dims<D>;
    using W = GcwDims<D>;  // the walk's: Q, and the tail's layout
    using E = GcwElLds<D>;
    static_assert(F::KS == W::KS && F::T == W::T && F::T == GwElBlob<D>::T, "the walk, the encoder's blob and the f16 stream cut a row into the same tiles");
    static_assert(F::SCALE_AT == W::SCALE_AT, "the tail is the split stream's");
    static_assert(F::STEPS >= 3 && F::STEPS % 2 == 1, "two chunks resident before the walk, pairs of steps in the loop, the last step behind it");
    static_assert(F::STEPS * F::TPC >= F::T, "every output tile has a chunk");
    static_assert(F::CHUNK_BYTES % 1024 == 0, "LDS-DMA moves whole 1 KiB pieces of a chunk");
    static constexpr int LDS_BYTES = E::BYTES + 2 * F::CHUNK_BYTES;
    static_assert(LDS_BYTES <= 160 * 1024, "the encoder's block and two weight buffers must fit the CU's LDS");
};

typedef _Float16 gcwef_half2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t gcwef_pack_rne(float a, float b) {  // to nearest even: one v_cvt_pk_f16_f32
    return __builtin_bit_cast(uint32_t, (gcwef_half2_t){(_Float16)a, (_Float16)b});
}

// the TPC output tiles of chunk c from the fragments in `wb`: one f16 MFMA per (tile, K-step), stored as soon as the chunk is done.
// The TPC fragment reads of a K-step stand in front of its TPC MFMAs: four independent accumulators, so no MFMA waits for the one before
template <int D>
__device__ __forceinline__ void gcwef_step(const char* wb, int c, int lane, int g, const ds_uint4_t (&in)[GcwElF16Dims<D>::KS],
                                           const float* __restrict__ tailp, float oscale, float* __restrict__ row, bool valid) {
    using M = GcwElF16Dims<D>;
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

// xout[v] = W r(a[v]) + b, a[v] = relu(pre[v]) (+ vn[g(v)]), pre from the encoder's walk.  lblob: the layer's part of the encoder's blob
// (GwElBlob); tab: the layer's table in global memory, of which the three epilogue rows are read; wchunks: the NEXT layer's hi-only
// stream (GcwF16Dims); tailp: the split stream's tail of that layer.
template <int D, bool VN>
__device__ __forceinline__ void gcwef_layer_body(const float* __restrict__ x, float* __restrict__ xout, const int* __restrict__ row_ptr,
                                                 const int* __restrict__ src, const int* __restrict__ eid, const float* __restrict__ ef,
                                                 const uint8_t* __restrict__ lblob, int el_f, const float* __restrict__ esc,
                                                 const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                 const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp, int n_tot,
                                                 int* __restrict__ range_flag, typename std::conditional<VN, GcwVnArgs, GcwNoVnArgs>::type vna) {
    using M = GcwElF16Dims<D>;
    using W = GcwDims<D>;
    // three DISTINCT LDS objects: the DMA into one weight buffer does not alias the reads of the other, nor those of the block
    __shared__ __attribute__((aligned(16))) char s_blk[M::E::BYTES];   // the encoder's block, resident for the whole launch
    __shared__ __attribute__((aligned(16))) char s_w0[M::CHUNK_BYTES];  // the even chunks
    __shared__ __attribute__((aligned(16))) char s_w1[M::CHUNK_BYTES];  // the odd chunks
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const long long node0 = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;
    const bool valid = node0 < n_tot;
    const long long node = valid ? node0 : (long long)n_tot - 1;

    gcw_el_issue_block<D>(lblob, tab, s_blk, wave, lane);
    gw_issue_pieces<M::PIECES>(wchunks, s_w0, M::PIECES, 64, wave, lane);                                 // chunk 0
    gw_issue_pieces<M::PIECES>(wchunks + (size_t)M::CHUNK_BYTES, s_w1, M::PIECES, 64, wave, lane);        // chunk 1
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // the block and the first two chunks are resident: nothing is in flight while the walk runs

    // ---- the walk and its epilogue, fp32: one in-edge per row and trip, in CSR order, the encoder on the matrix pipe
    float a[4 * W::Q];
    float vmax = 0.0f;  // (the trips set it to infinity at a feature beyond the range)
    gcw_walk<D, true, true>(x, row_ptr, src, nullptr, esc, out_deg, reinterpret_cast<const float*>(s_blk), node, valid, g, a,
                            GcwElArgs{eid, ef, el_f, &vmax});
    if constexpr (VN) {
        const int gi = valid ? vna.node_graph[node] : -1;
        gcw_vn_add_partials<D>(a, vna.vn, gi, j, g, (long long)blockIdx.x * GW_WAVES + wave, vna.part);
    }
    // a IS the fp32 value: r(a) below rounds it a second time, as the mode defines it and as gcn_wide_f16.hip's kernels compute it.
    // Without packed fp32 the compiler contracts the last fp32 operation (the virtual node's add, the epilogue's fma) and the
    // conversion into v_fma_mixlo_f16 / v_fma_mixhi_f16, which round the exact result ONCE -- another f16 value wherever the fp32
    // rounding crosses an f16 tie (section 4.37 found it in GIN's unit)
#pragma unroll
    for (int k = 0; k < 4 * W::Q; k++) asm volatile("" : "+v"(a[k]));
#pragma unroll
    for (int k = 0; k < 4 * W::Q; k += 2) vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, __builtin_fabsf(a[k])), __builtin_fabsf(a[k + 1]));
    ds_uint4_t in[M::KS];
#pragma unroll
    for (int ks = 0; ks < M::KS; ks++) {
        in[ks].x = gcwef_pack_rne(a[8 * ks + 0], a[8 * ks + 1]);
        in[ks].y = gcwef_pack_rne(a[8 * ks + 2], a[8 * ks + 3]);
        in[ks].z = gcwef_pack_rne(a[8 * ks + 4], a[8 * ks + 5]);
        in[ks].w = gcwef_pack_rne(a[8 * ks + 6], a[8 * ks + 7]);
    }
    const float oscale = tailp[M::SCALE_AT];
    float* const row = xout + (size_t)node * D;

    // ---- the product, weights streamed through LDS.  Chunks 0 and 1 have been resident since the first barrier and no request is
    // outstanding: step 0 ends in a barrier alone (everyone is done with s_w0), behind which chunk 2 is requested into it.  Every later
    // request is waited for by its wave and then by the workgroup before the buffer is read; the last step reads s_w0, whose chunk the
    // trip before it requested and waited for, and nobody writes either buffer again.
#pragma unroll 1
    for (int c = 0; c + 1 < M::STEPS; c += 2) {
        if (c > 0) gw_issue_pieces<M::PIECES>(wchunks + (size_t)(c + 1) * M::CHUNK_BYTES, s_w1, M::PIECES, 64, wave, lane);
        gcwef_step<D>(s_w0, c, lane, g, in, tailp, oscale, row, valid);
        if (c > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of chunk c + 1 have landed
        __syncthreads();                                             // everyone's have; everyone is done with s_w0
        gw_issue_pieces<M::PIECES>(wchunks + (size_t)(c + 2) * M::CHUNK_BYTES, s_w0, M::PIECES, 64, wave, lane);  // (c + 2 < STEPS: STEPS is odd)
        gcwef_step<D>(s_w1, c + 1, lane, g, in, tailp, oscale, row, valid);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    gcwef_step<D>(s_w0, M::STEPS - 1, lane, g, in, tailp, oscale, row, valid);
    if (__any(!(vmax < 6.0e4f))) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_layer_el_f16_kernel(const float* __restrict__ x, float* __restrict__ xout,
                                                                         const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                         const int* __restrict__ eid, const float* __restrict__ ef,
                                                                         const uint8_t* __restrict__ lblob, int el_f, const float* __restrict__ esc,
                                                                         const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                                         const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                         int n_tot, int* __restrict__ range_flag) {
    gcwef_layer_body<D, false>(x, xout, row_ptr, src, eid, ef, lblob, el_f, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, GcwNoVnArgs{});
}

// the VN instance: stage s adds vn_{s+1} behind the walk and (while an update follows) leaves the partial rows of xin_{s+1}
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_layer_vn_el_f16_kernel(const float* __restrict__ x, float* __restrict__ xout,
                                                                            const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                            const int* __restrict__ eid, const float* __restrict__ ef,
                                                                            const uint8_t* __restrict__ lblob, int el_f, const float* __restrict__ esc,
                                                                            const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                                            const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                            int n_tot, int* __restrict__ range_flag, GcwVnArgs vna) {
    gcwef_layer_body<D, true>(x, xout, row_ptr, src, eid, ef, lblob, el_f, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, vna);
}

constexpr int GCWEF_D = FLOWGNN_EMB_DIM_OGB;  // the launcher's one width: the public constant's

}  // namespace

int launch_gcw_layer_el_f16(int emb_dim, const void* blob, int edge_dim, int l, const float* x, float* xout, const int* row_ptr, const int* src,
                            const int* eid, const float* ef, const float* esc, const int* out_deg, const float* tab, const uint8_t* wchunks16,
                            const float* tailp, int n_tot, int* range_flag, const int* node_graph, const float* vn, float* part, hipStream_t s) {
    if (emb_dim != GCWEF_D || edge_dim < 1 || edge_dim > FLOWGNN_MAX_EDGE_DIM) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || l < 0 || (node_graph && !vn)) return FLOWGNN_ERR_ARG;
    if (n_tot <= 0) return 0;
    constexpr int D = GCWEF_D;
    const uint8_t* const lblob = static_cast<const uint8_t*>(blob) + (size_t)l * GwElBlob<D>::layer_stride(edge_dim);
    const int grid = (int)ceil_div_ll(n_tot, GW_ROWS);
    if (node_graph)
        gcw_layer_vn_el_f16_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(x, xout, row_ptr, src, eid, ef, lblob, edge_dim, esc, out_deg, tab, wchunks16, tailp,
                                                                     n_tot, range_flag, GcwVnArgs{node_graph, vn, part});
    else
        gcw_layer_el_f16_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(x, xout, row_ptr, src, eid, ef, lblob, edge_dim, esc, out_deg, tab, wchunks16, tailp, n_tot,
                                                                  range_flag);
    return 0;
}

}  // namespace fg
