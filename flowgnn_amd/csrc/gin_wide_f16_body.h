// gin_wide_f16_body.h -- the body of GIN's layer kernel at width 300 in FLOWGNN_NUMERIC_F16: GwfDims, one step
// of the node MLP (gwf_step) and gwf_layer_body, whose instances are the kernels of two translation units.  gin_wide_f16.hip has the
// two it always had (EXT = false), gin_wide_jk.hip the two with OGB's residual=True and JK="sum" in their epilogues (EXT = true;
// flowgnn_set_jk_residual, section 4.24: gin_wide_body.h states the epilogue's contract).  EXT is a compile-time constant: with it
// false the epilogue's extra code does not exist and a kernel is the one it was before this header did.
#pragma once
#include "common.h"
#include "dense_split.h"
#include "gin_wide_f16.h"
#include "wide_common.h"

namespace fg {
namespace {

template <int D>
struct GwfDims : GwF16Dims<D> {
    static_assert(D % 4 == 0, "rows are read as float4 pieces");
    using F = GwF16Dims<D>;
    static constexpr int Q = 2 * F::KS1;  // 16-feature pieces a lane holds four floats of
    static_assert(F::STEPS % 2 == 0, "the step loop alternates two LDS buffers");
    static constexpr int ECOMB_BYTES = EDGE_COMBOS * D * 4;  // the layer's 60 combined edge rows
    static constexpr int ECOMB_PIECES = (ECOMB_BYTES + 1023) / 1024;
    static constexpr int ECOMB_LAST_LANES = (ECOMB_BYTES - (ECOMB_PIECES - 1) * 1024) / 16;
    static_assert(ECOMB_BYTES % 16 == 0 && F::CHUNK_BYTES % 16 == 0, "LDS-DMA moves 16 bytes per lane");
    static_assert(ECOMB_BYTES + 2 * F::CHUNK_BYTES <= 160 * 1024, "the edge table and two weight buffers must fit the CU's LDS");
};

typedef _Float16 gwf_half2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t gwf_pack_rne(float a, float b) {  // to nearest even: one v_cvt_pk_f16_f32
    return __builtin_bit_cast(uint32_t, (gwf_half2_t){(_Float16)a, (_Float16)b});
}

// one step from the chunk in `wb`: MLP1 of hidden tiles 2s, 2s + 1 (their ReLU'd, rounded values become hb for the next step), and
// K-step s - 1 of MLP2 from the hb the previous step left
template <int D>
__device__ __forceinline__ void gwf_step(const char* wb, int s, int lane, int g, const ds_uint4_t (&in)[GwfDims<D>::KS1], ds_uint4_t& hb,
                                         float4_t (&acc2)[GwfDims<D>::T2], float& vmax) {
    using M = GwfDims<D>;
    ds_uint4_t nb = {0, 0, 0, 0};
    if (s < M::KS2) {
        float4_t acc1[2];
#pragma unroll
        for (int tl = 0; tl < 2; tl++) {
            const float4 b = *reinterpret_cast<const float4*>(wb + M::B1_OFF + tl * 64 + g * 16);
            acc1[tl] = (float4_t){b.x, b.y, b.z, b.w};
        }
#pragma unroll
        for (int ks = 0; ks < M::KS1; ks++) {
            ds_uint4_t a[2];
#pragma unroll
            for (int tl = 0; tl < 2; tl++) a[tl] = *reinterpret_cast<const ds_uint4_t*>(wb + (ks * 2 + tl) * 1024 + lane * 16);
#pragma unroll
            for (int tl = 0; tl < 2; tl++) acc1[tl] = DS_MFMA16(a[tl], in[ks], acc1[tl]);
        }
        float4_t r0 = acc1[0], r1 = acc1[1];
        r0.x = gw_relu(r0.x); r0.y = gw_relu(r0.y); r0.z = gw_relu(r0.z); r0.w = gw_relu(r0.w);
        r1.x = gw_relu(r1.x); r1.y = gw_relu(r1.y); r1.z = gw_relu(r1.z); r1.w = gw_relu(r1.w);
        vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, r0.x), r0.y);
        vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, r0.z), r0.w);
        vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, r1.x), r1.y);
        vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, r1.z), r1.w);
        asm volatile("" : "+v"(vmax));
        nb.x = gwf_pack_rne(r0.x, r0.y);
        nb.y = gwf_pack_rne(r0.z, r0.w);
        nb.z = gwf_pack_rne(r1.x, r1.y);
        nb.w = gwf_pack_rne(r1.z, r1.w);
    }
    if (s > 0) {
#pragma unroll
        for (int t2 = 0; t2 < M::T2; t2++) {
            const ds_uint4_t a = *reinterpret_cast<const ds_uint4_t*>(wb + M::W2_OFF + t2 * 1024 + lane * 16);
            acc2[t2] = DS_MFMA16(a, hb, acc2[t2]);
        }
    }
    hb = nb;
}

// hout[v] = W2 r(relu(W1 r(a[v]) + b1)) + b2 (ReLU'd if relu_out), a[v] = fma(h[v], self_s, sum over v's in-edges, in CSR order).
// VN: OGB's virtual node of the NEXT layer added in the epilogue, hout[v] = relu(..) + vn_add[node_graph[v]] (section 4.17).
template <int D, bool VN, bool EXT = false>
__device__ __forceinline__ void gwf_layer_body(const float* __restrict__ h, float* __restrict__ hout, const int* __restrict__ row_ptr,
                                               const int* __restrict__ src, const uint8_t* __restrict__ ecode, const float* __restrict__ ecomb,
                                               const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp, int n_tot, int relu_out,
                                               float self_s, int* __restrict__ range_flag, const int* __restrict__ node_graph,
                                               const float* __restrict__ vn_add, const float* __restrict__ xres = nullptr,
                                               const float* jk_in = nullptr, float* jk_out = nullptr) {
    using M = GwfDims<D>;
    // three DISTINCT LDS objects: the DMA into one weight buffer does not alias the reads of the other, nor those of the edge table
    __shared__ __attribute__((aligned(16))) char s_e[M::ECOMB_BYTES];  // the combined edge table
    __shared__ __attribute__((aligned(16))) char s_a[M::CHUNK_BYTES];  // the odd chunks
    __shared__ __attribute__((aligned(16))) char s_b[M::CHUNK_BYTES];  // the even chunks
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const long long node0 = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;
    const bool valid = node0 < n_tot;
    const long long node = valid ? node0 : (long long)n_tot - 1;

    int e_cur = row_ptr[node];
    const int e_end = valid ? row_ptr[node + 1] : e_cur;
    gw_issue_pieces<M::PIECES>(wchunks, s_b, M::PIECES, M::LAST_LANES, wave, lane);                                                      // chunk 0
    gw_issue_pieces<M::PIECES>(wchunks + M::CHUNK_STRIDE, s_a, M::PIECES, M::LAST_LANES, wave, lane);                                    // chunk 1
    gw_issue_pieces<M::ECOMB_PIECES>(reinterpret_cast<const uint8_t*>(ecomb), s_e, M::ECOMB_PIECES, M::ECOMB_LAST_LANES, wave, lane);  // the edge table
    float bq[4 * M::Q];
#pragma unroll
    for (int k = 0; k < 4 * M::Q; k++) bq[k] = 0.0f;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // the table and the first two chunks are resident: nothing is in flight while the gather runs
    const float* s_ecomb = reinterpret_cast<const float*>(s_e);

    // ---- gather: one in-edge per trip, in CSR order (a row's sum depends on the row alone); pieces at or beyond column D stay zero
    while (__any(e_cur < e_end)) {
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
    // ---- a = fma(h[v], s_l, m): one fp32 rounding (s_l = 1: the bits of the plain sum), then rounded into the B operands of MLP1
    float vmax = 0.0f;
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
#pragma unroll
        for (int k = 0; k < 4 * M::Q; k += 2) vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, __builtin_fabsf(bq[k])), __builtin_fabsf(bq[k + 1]));
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

    // ---- node MLP, weights streamed through LDS (no barrier in front: the edge table is overwritten by nobody, and chunks 0 and 1
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
        const float* xrow = EXT && xres ? xres + (size_t)node * D : nullptr;  // (EXT: gin_wide_body.h's contract, the residual's rows D apart)
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
                if (VN) {
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
