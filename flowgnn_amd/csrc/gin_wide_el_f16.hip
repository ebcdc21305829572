// GIN at OGB's default width with OGB's linear edge encoder in the walk and the f16 node MLP behind it: the layer of ogbg-ppa and
// ogbg-code2 in its throughput mode (flowgnn_set_edge_linear_numeric).
//   a[v] = fma(h[v], s_l, sum over v's in-edges (u, v) of relu(h[u] + W_e e_uv + b_e))      fp32, CSR order: gw_el_walk, unchanged
//   hout[v] = W2 r(relu(W1 r(a[v]) + b1)) + b2                                              r: to f16, nearest even (section 4.22)
//
// gw_layer_el_f16_kernel<D> / gw_layer_vn_el_f16_kernel<D>.  A wave owns one 16-node column tile.  The walk is gin_wide_el.hip's own
// function (gin_wide_el_walk.h): per trip one B operand out of the 16 rows' edges, T2 = 19 fragment reads and 19 MFMAs whose split
// K slots keep the encoder fp32-accurate.  What follows is gin_wide_f16.hip's: a rounded pair by pair into the B operands of MLP1 (no
// lo registers: `in` is 40 VGPRs, which is what leaves room for the walk's offsets and masks), then per step 2 KS1 + T2 MFMAs on the
// hi-only weight stream (gwf_step, gin_wide_f16_body.h).
//
// LDS, three distinct objects, 99 584 bytes: the layer's T2 encoder fragments (19 456 B, the head of GwElBlob) and the two 40 064-byte
// weight buffers of GwF16Dims.  No edge table.  The fragments, chunk 0 and chunk 1 are requested together in front of ONE
// s_waitcnt vmcnt(0) and ONE barrier; nothing is in flight while the walk runs (a request made there would be drained by the
// compiler's own waits in front of the walk's loads, section 4.22), the fragments are overwritten by nobody and both chunks are
// resident, so there is no barrier between the walk and the MLP: the step loop's first request is chunk 2's, behind the barrier of
// step 0.  Per step one s_waitcnt vmcnt(0) and one workgroup barrier, as in gin_wide_f16.hip.
//
// fp32 and gin_wide.hip's: biases, 1 / (s1 s2), the ReLU, the virtual node's add in the epilogue.  The range flag is raised by a, a
// hidden unit or an edge feature at or beyond 6e4 or not finite; the engine then repeats the pass on the fp32 exact path
// (launch_gw_aggregate_el + launch_gw_mlp_f32).  The body is this file's own copy of gwf_layer_body with the walk in the gather's
// place: sections 4.21 and 4.22 record that a body shared between the wide files moves their register allocation.
#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "gin_wide_el_f16.h"
#include "gin_wide_el_walk.h"   // gw_el_walk (and GwDims, whose Q / KS1 / T2 shape the walk's registers)
#include "gin_wide_f16_body.h"  // GwfDims, gwf_pack_rne and gwf_step
#include "wide_common.h"        // GW_WAVES / GW_ROWS, gw_relu, the LDS-DMA issue
#include "wide_el_pack.h"       // GwElBlob: where the fragments and 1 / scale are in a layer's part of the encoder's blob

namespace fg {
namespace {

template <int D>
struct GwElF16Dims : GwfDims<D> {
    using F = GwfDims<D>;
    static constexpr int FRAG_BYTES = F::T2 * 1024;  // the encoder's A operands, one 1 KiB fragment per 16-column output tile
    static_assert(F::T2 == GwElBlob<D>::T && F::T2 == GwDims<D>::T2 && F::Q == GwDims<D>::Q && F::KS1 == GwDims<D>::KS1,
                  "the walk, the encoder's blob and the f16 stream cut a row into the same tiles");
    static_assert(FRAG_BYTES + 2 * F::CHUNK_BYTES <= 160 * 1024, "the fragments and two weight buffers must fit the CU's LDS");
};

// hout[v] = W2 r(relu(W1 r(a[v]) + b1)) + b2 (ReLU'd if relu_out), a[v] = fma(h[v], self_s, the walk's sum over v's in-edges).
// VN: OGB's virtual node of the NEXT layer added in the epilogue, hout[v] = relu(..) + vn_add[node_graph[v]] (section 4.17).
// lblob: the layer's part of the encoder's blob (GwElBlob); wchunks: the layer's hi-only stream; tailp: the split stream's tail.
template <int D, bool VN>
__device__ __forceinline__ void gwef_layer_body(const float* __restrict__ h, float* __restrict__ hout, const int* __restrict__ row_ptr,
                                                const int* __restrict__ src, const int* __restrict__ eid, const float* __restrict__ ef,
                                                const uint8_t* __restrict__ lblob, int el_f, const uint8_t* __restrict__ wchunks,
                                                const float* __restrict__ tailp, int n_tot, int relu_out, float self_s,
                                                int* __restrict__ range_flag, const int* __restrict__ node_graph,
                                                const float* __restrict__ vn_add) {
    using M = GwElF16Dims<D>;
    // three DISTINCT LDS objects: the DMA into one weight buffer does not alias the reads of the other, nor those of the fragments
    __shared__ __attribute__((aligned(16))) char s_f[M::FRAG_BYTES];   // the encoder's fragments, resident for the whole launch
    __shared__ __attribute__((aligned(16))) char s_a[M::CHUNK_BYTES];  // the odd chunks
    __shared__ __attribute__((aligned(16))) char s_b[M::CHUNK_BYTES];  // the even chunks
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const long long node0 = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;
    const bool valid = node0 < n_tot;
    const long long node = valid ? node0 : (long long)n_tot - 1;

    const int e_cur = row_ptr[node];
    const int e_end = valid ? row_ptr[node + 1] : e_cur;
    const float el_inv = *reinterpret_cast<const float*>(lblob + GwElBlob<D>::INV_OFF);
    gw_issue_pieces<M::T2>(lblob, s_f, M::T2, 64, wave, lane);                                          // the fragments
    gw_issue_pieces<M::PIECES>(wchunks, s_b, M::PIECES, M::LAST_LANES, wave, lane);                     // chunk 0
    gw_issue_pieces<M::PIECES>(wchunks + M::CHUNK_STRIDE, s_a, M::PIECES, M::LAST_LANES, wave, lane);   // chunk 1
    float bq[4 * M::Q];
#pragma unroll
    for (int k = 0; k < 4 * M::Q; k++) bq[k] = 0.0f;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // the fragments and the first two chunks are resident: nothing is in flight while the walk runs

    // ---- the walk: one in-edge per row and trip, in CSR order, the encoder on the matrix pipe; pieces at or beyond column D stay zero
    float vmax = 0.0f;  // (the walk sets it to infinity at a feature beyond the range)
    gw_el_walk<D>(h, src, eid, ef, el_f, el_inv, s_f, e_cur, e_end, lane, bq, vmax);

    // ---- a = fma(h[v], s_l, m): one fp32 rounding (s_l = 1: the bits of the plain sum), then rounded into the B operands of MLP1
    ds_uint4_t in[M::KS1];
    {
        const float* hr = h + (size_t)node * D + 4 * g;
#pragma unroll
        for (int q = 0; q < M::Q; q++)
            if (16 * q + 4 * g < D) {
                const float4 x = *reinterpret_cast<const float4*>(hr + 16 * q);
                bq[4 * q + 0] = __builtin_fmaf(x.x, self_s, bq[4 * q + 0]);
                bq[4 * q + 1] = __builtin_fmaf(x.y, self_s, bq[4 * q + 1]);
                bq[4 * q + 2] = __builtin_fmaf(x.z, self_s, bq[4 * q + 2]);
                bq[4 * q + 3] = __builtin_fmaf(x.w, self_s, bq[4 * q + 3]);
            }
        // a IS the fp32 value: r(a) below rounds it a second time, as the mode defines it and as gin_wide_f16.hip's kernels compute it.
        // Left to itself the compiler contracts the fma and the conversion into v_fma_mixlo_f16, which rounds the exact sum ONCE --
        // another f16 value wherever the fp32 rounding crosses an f16 tie (a few rows in a thousand)
#pragma unroll
        for (int k = 0; k < 4 * M::Q; k++) asm volatile("" : "+v"(bq[k]));
#pragma unroll
        for (int k = 0; k < 4 * M::Q; k += 2) vmax =__builtin_fmaxf(__builtin_fmaxf(vmax, __builtin_fabsf(bq[k])), __builtin_fabsf(bq[k + 1]));
#pragma unroll
        for (int ks = 0; ks < M::KS1; ks++) {
            in[ks].x = gwf_pack_rne(bq[8 * ks + 0], bq[8 * ks + 1]);
            in[ks].y = gwf_pack_rne(bq[8 * ks + 2], bq[8 * ks + 3]);
            in[ks].z = gwf_pack_rne(bq[8 * ks + 4], bq[8 * ks + 5]);
            in[ks].w = gwf_pack_rne(bq[8 * ks + 6], bq[8 * ks + 7]);
        }
    }
    float4_t acc2[M::T2];
#pragma unroll
    for (int t2 = 0; t2 < M::T2; t2++) {
        const float4 b = *reinterpret_cast<const float4*>(tailp + 16 * t2 + 4 * g);
        acc2[t2] = (float4_t){b.x, b.y, b.z, b.w};
    }
    const float oscale = tailp[M::T2 * 16];

    // ---- node MLP, weights streamed through LDS (no barrier in front: the fragments are overwritten by nobody, and chunks 0 and 1
    // have been resident since the first barrier -- the first request of the loop is chunk 2's, behind a barrier of its own)
    ds_uint4_t hb = {0, 0, 0, 0};
#pragma unroll 1
    for (int c = 0; c < M::STEPS; c += 2) {
        if (c > 0) gw_issue_pieces<M::PIECES>(wchunks + (size_t)(c + 1) * M::CHUNK_STRIDE, s_a, M::PIECES, M::LAST_LANES, wave, lane);
        gwf_step<D>(s_b, c, lane, g, in, hb, acc2, vmax);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of chunk c + 1 have landed
        __syncthreads();                                  // everyone's have; everyone is done with s_b
        if (c + 2 < M::STEPS) gw_issue_pieces<M::PIECES>(wchunks + (size_t)(c + 2) * M::CHUNK_STRIDE, s_b, M::PIECES, M::LAST_LANES, wave, lane);
        gwf_step<D>(s_a, c + 1, lane, g, in, hb, acc2, vmax);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    if (valid) {
        float* row = hout + (size_t)node * D;
        const float* vrow = VN ? vn_add + (size_t)node_graph[node] * D : nullptr;  // the lane's node decides the vector, lane by lane
#pragma unroll
        for (int t2 = 0; t2 < M::T2; t2++) {
            const int col = 16 * t2 + 4 * g;
            if (col < D) {
                float4_t r = acc2[t2] * oscale;
                if (relu_out) { r.x = gw_relu(r.x); r.y = gw_relu(r.y); r.z = gw_relu(r.z); r.w = gw_relu(r.w); }
                if (VN) {
                    const float4 a = *reinterpret_cast<const float4*>(vrow + col);
                    r.x += a.x; r.y += a.y; r.z += a.z; r.w += a.w;
                }
                *reinterpret_cast<float4*>(row + col) = make_float4(r.x, r.y, r.z, r.w);
            }
        }
    }
    if (__any(!(vmax < 6.0e4f))) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_layer_el_f16_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                        const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                        const int* __restrict__ eid, const float* __restrict__ ef,
                                                                        const uint8_t* __restrict__ lblob, int el_f,
                                                                        const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                        int n_tot, int relu_out, float self_s, int* __restrict__ range_flag) {
    gwef_layer_body<D, false>(h, hout, row_ptr, src, eid, ef, lblob, el_f, wchunks, tailp, n_tot, relu_out, self_s, range_flag, nullptr, nullptr);
}

// the VN instance: x_{l+1}[v] = relu(layer l of x_l)[v] + vn_{l+1}[node_graph[v]] (always ReLU'd), as gw_layer_vn_el_kernel
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_layer_vn_el_f16_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                           const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                           const int* __restrict__ eid, const float* __restrict__ ef,
                                                                           const uint8_t* __restrict__ lblob, int el_f,
                                                                           const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                           int n_tot, float self_s, int* __restrict__ range_flag,
                                                                           const int* __restrict__ node_graph, const float* __restrict__ vn_add) {
    gwef_layer_body<D, true>(h, hout, row_ptr, src, eid, ef, lblob, el_f, wchunks, tailp, n_tot, 1, self_s, range_flag, node_graph, vn_add);
}

constexpr int GWEF_D = FLOWGNN_EMB_DIM_OGB;  // the launcher's one width: the public constant's

}  // namespace

int launch_gw_layer_el_f16(int emb_dim, const void* blob, int edge_dim, int l, const float* h, float* hout, const int* row_ptr, const int* src,
                           const int* eid, const float* ef, const uint8_t* wchunks, const float* tailp, int n_tot, int relu_out, float self_s,
                           int* range_flag, const int* node_graph, const float* vn_add, hipStream_t s) {
    if (emb_dim != GWEF_D || edge_dim < 1 || edge_dim > FLOWGNN_MAX_EDGE_DIM) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || l < 0) return FLOWGNN_ERR_ARG;
    if (n_tot <= 0) return 0;
    constexpr int D = GWEF_D;
    const uint8_t* const lblob = static_cast<const uint8_t*>(blob) + (size_t)l * GwElBlob<D>::layer_stride(edge_dim);
    const int grid = (int)ceil_div_ll(n_tot, GW_ROWS);
    if (node_graph)
        gw_layer_vn_el_f16_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(h, hout, row_ptr, src, eid, ef, lblob, edge_dim, wchunks, tailp, n_tot, self_s,
                                                                    range_flag, node_graph, vn_add);
    else
        gw_layer_el_f16_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(h, hout, row_ptr, src, eid, ef, lblob, edge_dim, wchunks, tailp, n_tot, relu_out,
                                                                 self_s, range_flag);
    return 0;
}

}  // namespace fg
