// gin_wide_body.h -- the body of GIN's layer kernel at width 300: the weight stream's layout (GwDims), one
// step of the node MLP (gw_step) and gw_layer_body, whose instances are the kernels of two translation units.  gin_wide.hip has the
// three it always had (EXT = false: the layer, its virtual-node instance, the virtual node's update), gin_wide_jk.hip the three with
// OGB's residual=True and JK="sum" in their epilogues (EXT = true; flowgnn_set_jk_residual, section 4.24).  EXT is a compile-time
// constant: with it false the epilogue's extra code does not exist and a kernel is the one it was before this header did.
#pragma once
#include "common.h"
#include "dense_split.h"
#include "wide_common.h"

namespace fg {
namespace {

template <int D>
struct GwDims {
    static_assert(D % 4 == 0, "rows are read as float4 pieces");
    static constexpr int H = 2 * D;
    static constexpr int C = D / 4;               // float4 pieces of a row
    static constexpr int KS1 = (D + 31) / 32;     // K-steps of the first product (K padded to 32 KS1)
    static constexpr int Q = 2 * KS1;             // 16-feature pieces a lane holds four floats of
    static constexpr int KS2 = (H + 31) / 32;     // K-steps of the second product
    static constexpr int T1 = 2 * KS2;            // 16-row tiles of the hidden layer (K of the second product padded to 16 T1)
    static constexpr int T2 = (D + 15) / 16;      // 16-row tiles of the output, the last one masked at column D
    static constexpr int STEPS = KS2 + 1;         // step s: MLP1 of hidden tiles 2s, 2s + 1 (s < KS2) and K-step s - 1 of MLP2 (s > 0)
    static_assert(STEPS % 2 == 0, "the step loop alternates two LDS buffers");
    // chunk s of the weight stream, in 1 KiB fragments (64 lanes x 8 halves):
    //   [0, W2_OFF): W1 of hidden tiles 2s, 2s + 1: fragment ((ks * 2 + tl) * 2 + p), p = 0 hi, 1 lo          (absent for s = KS2)
    //   [W2_OFF, B1_OFF): W2 of K-step s - 1: fragment (t2 * 2 + p)                                          (absent for s = 0)
    //   [B1_OFF, CHUNK_BYTES): b1 of the two hidden tiles, pre-scaled: 2 x 16 floats
    static constexpr int W2_OFF = KS1 * 2 * 2 * 1024;
    static constexpr int B1_OFF = W2_OFF + T2 * 2 * 1024;
    static constexpr int CHUNK_BYTES = B1_OFF + 2 * 16 * 4;
    static constexpr int PIECES = (CHUNK_BYTES + 1023) / 1024;   // DMA pieces of 1 KiB, the last one partial
    static constexpr int LAST_LANES = (CHUNK_BYTES - (PIECES - 1) * 1024) / 16;
    static constexpr int CHUNK_STRIDE = PIECES * 1024;           // in global memory
    static constexpr size_t LAYER_BYTES = (size_t)STEPS * CHUNK_STRIDE;
    static constexpr int ECOMB_BYTES = EDGE_COMBOS * D * 4;      // the layer's 60 combined edge rows: in buffer A until the first odd chunk
    static constexpr int ECOMB_PIECES = (ECOMB_BYTES + 1023) / 1024;
    static constexpr int ECOMB_LAST_LANES = (ECOMB_BYTES - (ECOMB_PIECES - 1) * 1024) / 16;
    static_assert(ECOMB_BYTES <= CHUNK_BYTES && ECOMB_BYTES % 16 == 0, "the combined edge table shares buffer A");
    static_assert(2 * CHUNK_BYTES <= 160 * 1024, "two weight buffers must fit the CU's LDS");
    static constexpr int TAIL_FLOATS = T2 * 16 + 4;  // per layer, read from global memory: b2 pre-scaled and padded, then 1 / (s1 s2)
};

template <int D>
__device__ __forceinline__ void gw_issue(const uint8_t* __restrict__ gsrc, char* lds_buf, int pieces, int last_lanes, int wave, int lane) {
    gw_issue_pieces<GwDims<D>::PIECES>(gsrc, lds_buf, pieces, last_lanes, wave, lane);  // (wide_common.h)
}

// one step from the chunk in `wb`: MLP1 of hidden tiles 2s, 2s + 1 (their ReLU'd, split values become h_hi / h_lo for the next step),
// and K-step s - 1 of MLP2 from the h_hi / h_lo the previous step left
template <int D>
__device__ __forceinline__ void gw_step(const char* wb, int s, int lane, int g, const ds_uint4_t (&in_hi)[GwDims<D>::KS1],
                                        const ds_uint4_t (&in_lo)[GwDims<D>::KS1], ds_uint4_t& h_hi, ds_uint4_t& h_lo,
                                        float4_t (&acc2)[GwDims<D>::T2], float& vmax) {
    using M = GwDims<D>;
    ds_uint4_t n_hi = {0, 0, 0, 0}, n_lo = {0, 0, 0, 0};
    if (s < M::KS2) {
        float4_t acc1[2];
#pragma unroll
        for (int tl = 0; tl < 2; tl++) {
            const float4 b = *reinterpret_cast<const float4*>(wb + M::B1_OFF + tl * 64 + g * 16);
            acc1[tl] = (float4_t){b.x, b.y, b.z, b.w};
        }
#pragma unroll
        for (int ks = 0; ks < M::KS1; ks++) {
            ds_uint4_t a[2][2];
#pragma unroll
            for (int tl = 0; tl < 2; tl++)
#pragma unroll
                for (int p = 0; p < 2; p++) a[tl][p] = *reinterpret_cast<const ds_uint4_t*>(wb + ((ks * 2 + tl) * 2 + p) * 1024 + lane * 16);
#pragma unroll
            for (int tl = 0; tl < 2; tl++) acc1[tl] = DS_MFMA16(a[tl][0], in_hi[ks], acc1[tl]);
#pragma unroll
            for (int tl = 0; tl < 2; tl++) acc1[tl] = DS_MFMA16(a[tl][0], in_lo[ks], acc1[tl]);
#pragma unroll
            for (int tl = 0; tl < 2; tl++) acc1[tl] = DS_MFMA16(a[tl][1], in_hi[ks], acc1[tl]);
        }
        float4_t r0 = acc1[0], r1 = acc1[1];
        r0.x = gw_relu(r0.x); r0.y = gw_relu(r0.y); r0.z = gw_relu(r0.z); r0.w = gw_relu(r0.w);
        r1.x = gw_relu(r1.x); r1.y = gw_relu(r1.y); r1.z = gw_relu(r1.z); r1.w = gw_relu(r1.w);
        vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, r0.x), r0.y);
        vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, r0.z), r0.w);
        vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, r1.x), r1.y);
        vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, r1.z), r1.w);
        asm volatile("" : "+v"(vmax));
        DS_SPLIT2(r0.x, r0.y, n_hi.x, n_lo.x);
        DS_SPLIT2(r0.z, r0.w, n_hi.y, n_lo.y);
        DS_SPLIT2(r1.x, r1.y, n_hi.z, n_lo.z);
        DS_SPLIT2(r1.z, r1.w, n_hi.w, n_lo.w);
    }
    if (s > 0) {
#pragma unroll
        for (int t2 = 0; t2 < M::T2; t2++) {
            const ds_uint4_t a_hi = *reinterpret_cast<const ds_uint4_t*>(wb + M::W2_OFF + (t2 * 2 + 0) * 1024 + lane * 16);
            const ds_uint4_t a_lo = *reinterpret_cast<const ds_uint4_t*>(wb + M::W2_OFF + (t2 * 2 + 1) * 1024 + lane * 16);
            acc2[t2] = DS_MFMA16(a_hi, h_hi, acc2[t2]);
            acc2[t2] = DS_MFMA16(a_hi, h_lo, acc2[t2]);
            acc2[t2] = DS_MFMA16(a_lo, h_hi, acc2[t2]);
        }
    }
    h_hi = n_hi;
    h_lo = n_lo;
}

// hout[v] = W2 relu(W1 a[v] + b1) + b2 (ReLU'd if relu_out), a[v] = fma(h[v], self_s, sum over v's in-edges, in CSR order)
// The body of the layer's kernels; MODE and EXT are compile-time constants in each, and GW_PLAIN without EXT compiles to what the one
// kernel was before the others existed.
//   GW_PLAIN   the layer
//   GW_VN      the layer, and OGB's virtual node of the NEXT layer added in the epilogue: hout[v] = relu(..) + vn_add[node_graph[v]],
//              one fp32 add just before the store (section 4.17) -- the 16 rows of a tile may belong to 16 different graphs
//   GW_UPDATE  the virtual node's update MLP: the "rows" are the per-graph sums t, nothing has in-edges (no gather, no edge table)
// EXT (section 4.24), every add fp32, in this order, on the lane's own float4 pieces:
//   xres non-null   OGB's residual=True: r += xres[node * xres_stride], after the scale and the ReLU and before the virtual node's add.
//                   A layer passes its input rows h (stride D), the update the previous vector vn_l (stride D; E with stride 0 for l = 0)
//   jk_out non-null OGB's JK="sum": jk_out[node] = jk_in[node] + (what the layer stores).  Layer 0 passes its input rows x_0 as jk_in,
//                   layers 1..4 the running sum; jk_in may be jk_out -- a lane reads its pieces before it writes them, and no other lane
//                   or workgroup touches them
enum { GW_PLAIN = 0, GW_VN = 1, GW_UPDATE = 2 };

template <int D, int MODE, bool EXT = false>
__device__ __forceinline__ void gw_layer_body(const float* __restrict__ h, float* __restrict__ hout, const int* __restrict__ row_ptr,
                                              const int* __restrict__ src, const uint8_t* __restrict__ ecode, const float* __restrict__ ecomb,
                                              const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp, int n_tot, int relu_out,
                                              float self_s, int* __restrict__ range_flag, const int* __restrict__ node_graph,
                                              const float* __restrict__ vn_add, const float* __restrict__ xres = nullptr,
                                              int xres_stride = 0, const float* jk_in = nullptr, float* jk_out = nullptr) {
    using M = GwDims<D>;
    // two DISTINCT LDS objects, as in gin_layer_split_kernel: the DMA into one does not alias the reads of the other
    __shared__ __attribute__((aligned(16))) char s_a[M::CHUNK_BYTES];  // the combined edge table, then the odd chunks
    __shared__ __attribute__((aligned(16))) char s_b[M::CHUNK_BYTES];  // the even chunks
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const long long node0 = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;
    const bool valid = node0 < n_tot;
    const long long node = valid ? node0 : (long long)n_tot - 1;

    int e_cur = MODE == GW_UPDATE ? 0 : row_ptr[node];
    const int e_end = MODE == GW_UPDATE ? 0 : (valid ? row_ptr[node + 1] : e_cur);
    gw_issue<D>(wchunks, s_b, M::PIECES, M::LAST_LANES, wave, lane);                                                  // chunk 0
    if (MODE != GW_UPDATE)
        gw_issue<D>(reinterpret_cast<const uint8_t*>(ecomb), s_a, M::ECOMB_PIECES, M::ECOMB_LAST_LANES, wave, lane);  // the edge table
    float bq[4 * M::Q];
#pragma unroll
    for (int k = 0; k < 4 * M::Q; k++) bq[k] = 0.0f;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const float* s_ecomb = reinterpret_cast<const float*>(s_a);

    // ---- gather: one in-edge per trip, in CSR order (a row's sum depends on the row alone); pieces at or beyond column D stay zero
    while (MODE != GW_UPDATE && __any(e_cur < e_end)) {
        if (e_cur < e_end) {
            const int u = src[e_cur];
            const int code = ecode[e_cur];
            e_cur++;
            const float* hr = h + (size_t)u * D + 4 * g;
            const float* er = s_ecomb + code * D + 4 * g;
#pragma unroll
            for (int q0 = 0; q0 < M::Q; q0 += M::KS1) {
                float4 x[M::KS1];
#pragma unroll
                for (int q = 0; q < M::KS1; q++)
                    if (16 * (q0 + q) + 4 * g < D) x[q] = *reinterpret_cast<const float4*>(hr + 16 * (q0 + q));
#pragma unroll
                for (int q = 0; q < M::KS1; q++)
                    if (16 * (q0 + q) + 4 * g < D) {
                        const float4 w = *reinterpret_cast<const float4*>(er + 16 * (q0 + q));
                        bq[4 * (q0 + q) + 0] += relu1(w.x + x[q].x);
                        bq[4 * (q0 + q) + 1] += relu1(w.y + x[q].y);
                        bq[4 * (q0 + q) + 2] += relu1(w.z + x[q].z);
                        bq[4 * (q0 + q) + 3] += relu1(w.w + x[q].w);
                    }
            }
        }
    }
    // ---- a = fma(h[v], s_l, m): one fp32 rounding (s_l = 1: the bits of the plain sum), then split into the B operands of MLP1
    float vmax = 0.0f;
    ds_uint4_t in_hi[M::KS1], in_lo[M::KS1];
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
#pragma unroll
        for (int k = 0; k < 4 * M::Q; k += 2) vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, __builtin_fabsf(bq[k])), __builtin_fabsf(bq[k + 1]));
#pragma unroll
        for (int ks = 0; ks < M::KS1; ks++) {
            DS_SPLIT2(bq[8 * ks + 0], bq[8 * ks + 1], in_hi[ks].x, in_lo[ks].x);
            DS_SPLIT2(bq[8 * ks + 2], bq[8 * ks + 3], in_hi[ks].y, in_lo[ks].y);
            DS_SPLIT2(bq[8 * ks + 4], bq[8 * ks + 5], in_hi[ks].z, in_lo[ks].z);
            DS_SPLIT2(bq[8 * ks + 6], bq[8 * ks + 7], in_hi[ks].w, in_lo[ks].w);
        }
    }
    float4_t acc2[M::T2];
#pragma unroll
    for (int t2 = 0; t2 < M::T2; t2++) {
        const float4 b = *reinterpret_cast<const float4*>(tailp + 16 * t2 + 4 * g);
        acc2[t2] = (float4_t){b.x, b.y, b.z, b.w};
    }
    const float oscale = tailp[M::T2 * 16];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // every wave is done with the edge table: s_a may be overwritten (chunk 0 has been resident since the first barrier)

    // ---- node MLP, weights streamed through LDS
    ds_uint4_t h_hi = {0, 0, 0, 0}, h_lo = {0, 0, 0, 0};
#pragma unroll 1
    for (int c = 0; c < M::STEPS; c += 2) {
        gw_issue<D>(wchunks + (size_t)(c + 1) * M::CHUNK_STRIDE, s_a, M::PIECES, M::LAST_LANES, wave, lane);
        gw_step<D>(s_b, c, lane, g, in_hi, in_lo, h_hi, h_lo, acc2, vmax);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of chunk c + 1 have landed
        __syncthreads();                                  // everyone's have; everyone is done with s_b
        if (c + 2 < M::STEPS) gw_issue<D>(wchunks + (size_t)(c + 2) * M::CHUNK_STRIDE, s_b, M::PIECES, M::LAST_LANES, wave, lane);
        gw_step<D>(s_a, c + 1, lane, g, in_hi, in_lo, h_hi, h_lo, acc2, vmax);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    if (valid) {
        float* row = hout + (size_t)node * D;
        // (GW_VN: in_hi / in_lo are dead here; the lane's node decides the vector, lane by lane)
        const float* vrow = MODE == GW_VN ? vn_add + (size_t)node_graph[node] * D : nullptr;
        const float* xrow = EXT && xres ? xres + (size_t)node * xres_stride : nullptr;
        const float* jrow = EXT && jk_out ? jk_in + (size_t)node * D : nullptr;
        float* jout = EXT && jk_out ? jk_out + (size_t)node * D : nullptr;
#pragma unroll
        for (int t2 = 0; t2 < M::T2; t2++) {
            const int col = 16 * t2 + 4 * g;
            if (col < D) {
                float4_t r = acc2[t2] * oscale;
                if (relu_out) { r.x = gw_relu(r.x); r.y = gw_relu(r.y); r.z = gw_relu(r.z); r.w = gw_relu(r.w); }
                if (EXT && xrow) {
                    const float4 a = *reinterpret_cast<const float4*>(xrow + col);
                    r.x += a.x; r.y += a.y; r.z += a.z; r.w += a.w;
                }
                if (MODE == GW_VN) {
                    const float4 a = *reinterpret_cast<const float4*>(vrow + col);
                    r.x += a.x; r.y += a.y; r.z += a.z; r.w += a.w;
                }
                *reinterpret_cast<float4*>(row + col) = make_float4(r.x, r.y, r.z, r.w);
                if (EXT && jout) {
                    const float4 a = *reinterpret_cast<const float4*>(jrow + col);
                    *reinterpret_cast<float4*>(jout + col) = make_float4(a.x + r.x, a.y + r.y, a.z + r.z, a.w + r.w);
                }
            }
        }
    }
    if (__any(!(vmax < 6.0e4f))) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

}  // namespace
}  // namespace fg
