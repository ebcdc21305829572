// OGB's graph_pooling="attention" readout at width 300 (flowgnn_set_attention_pooling), for gin_wide.hip and
// gcn_wide.hip alike: their one readout (GwReadout, wide_common.h) calls the two launch functions of wide_attn.h in place of its
// gw_pool_rows_kernel launch.  The gate's stream is packed with wide_common.h's gw_pack_tile, as the layers' streams are.
//   s[v]      = w2 . relu(W1 r[v] + b1)            W1 [H][D], b1 [H], w2 [H], H = 2 D (the gate's BatchNorm folded in by the exporter)
//   pooled[g] = (sum_v e[v] r[v]) / (sum_v e[v]),  e[v] = exp(s[v] - max_{u in g} s[u]), both sums in node order
//
// attn_gate_kernel<D>: the scheme of gin_wide.hip's gw_layer_body, GW_UPDATE instance, with the second product taken out -- a wave owns
// 16 rows, reads them straight into the B-operand layout of the f16 matrix pipe and splits them (DS_SPLIT2); per step it runs MLP1 of
// two hidden tiles as three f16 MFMAs per K-step (w_hi x_hi + w_hi x_lo + w_lo x_hi, fp32 accumulate, W1 pre-scaled by a power of two
// and split on the host), and the H -> 1 product follows in fp32 on the VALU: the lane's eight ReLU'd hidden values of the step times
// the matching w2 entries (pre-divided by the scale, an exact division), one fma chain per lane.  The W1 stream goes L2 -> LDS by LDS-DMA
// into two distinct LDS objects, shared by the eight waves of a 128-row workgroup; s_waitcnt vmcnt(0) + one barrier per step.
//   lane (j = lane & 15, g = lane >> 4): row j of the wave's tile; B operand of K-step ks, slot e: feature 16 (2 ks + (e >> 2)) + 4 g + (e & 3);
//   C layout of hidden tile t, slot r: hidden unit 16 t + 4 g + r -- the four lane groups g of a row are summed once, at the end.
// attn_pool_rows_kernel<D>: the shape of gw_pool_rows_kernel (wide_common.h), one wavefront per graph, no atomics.
#include "../../include/flowgnn.h"
#include "wide_common.h"  // (common.h, dense_split.h, wide_attn.h)

namespace fg {
namespace {

template <int D>
struct AgDims {
    static_assert(D % 4 == 0, "rows are read as float4 pieces");
    static constexpr int H = 2 * D;
    static constexpr int C = D / 4;
    static constexpr int KS1 = (D + 31) / 32;  // K-steps of the product (K padded to 32 KS1 with zero weights)
    static constexpr int Q = 2 * KS1;          // 16-feature pieces a lane holds four floats of
    static constexpr int STEPS = (H + 31) / 32;  // step s: hidden tiles 2s, 2s + 1 (H padded to 32 STEPS with zero weights)
    // chunk s of the weight stream, in 1 KiB fragments (64 lanes x 8 halves):
    //   [0, B1_OFF): W1 of hidden tiles 2s, 2s + 1: fragment ((ks * 2 + tl) * 2 + p), p = 0 hi, 1 lo
    //   [B1_OFF, W2_OFF): b1 of the two tiles, pre-scaled: 2 x 16 floats
    //   [W2_OFF, CHUNK_BYTES): w2 of the two tiles, pre-divided by the scale: 2 x 16 floats
    static constexpr int B1_OFF = KS1 * 2 * 2 * 1024;
    static constexpr int W2_OFF = B1_OFF + 2 * 16 * 4;
    static constexpr int CHUNK_BYTES = W2_OFF + 2 * 16 * 4;
    static constexpr int PIECES = (CHUNK_BYTES + 1023) / 1024;  // DMA pieces of 1 KiB, the last one partial
    static constexpr int LAST_LANES = (CHUNK_BYTES - (PIECES - 1) * 1024) / 16;
    static constexpr int CHUNK_STRIDE = PIECES * 1024;  // in global memory
    static constexpr size_t STREAM_BYTES = (size_t)STEPS * CHUNK_STRIDE;
    static_assert(2 * CHUNK_BYTES <= 160 * 1024, "two weight buffers must fit the CU's LDS");
    // the blob: the stream | W1^T [D][H] | b1 [H] | w2 [H]   (the three fp32 parts: the exact form)
    static constexpr size_t W1T_OFF = STREAM_BYTES;
    static constexpr size_t B1F_OFF = W1T_OFF + (size_t)D * H * 4;
    static constexpr size_t W2F_OFF = B1F_OFF + (size_t)H * 4;
    static constexpr size_t BYTES = W2F_OFF + (size_t)H * 4;
    static_assert(W1T_OFF % 16 == 0 && B1F_OFF % 16 == 0 && W2F_OFF % 16 == 0, "the parts are read in 16-byte pieces");
};

// one step from the chunk in `wb`: MLP1 of two hidden tiles, ReLU, and the lane's eight terms of w2 . hidden
template <int D>
__device__ __forceinline__ void ag_step(const char* wb, int lane, int g, const ds_uint4_t (&in_hi)[AgDims<D>::KS1],
                                        const ds_uint4_t (&in_lo)[AgDims<D>::KS1], float& part, float& vmax) {
    using M = AgDims<D>;
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
#pragma unroll
    for (int tl = 0; tl < 2; tl++) {
        float4_t r = acc1[tl];
        r.x = gw_relu(r.x); r.y = gw_relu(r.y); r.z = gw_relu(r.z); r.w = gw_relu(r.w);
        vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, r.x), r.y);
        vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, r.z), r.w);
        const float4 w = *reinterpret_cast<const float4*>(wb + M::W2_OFF + tl * 64 + g * 16);
        part = __builtin_fmaf(r.x, w.x, part);
        part = __builtin_fmaf(r.y, w.y, part);
        part = __builtin_fmaf(r.z, w.z, part);
        part = __builtin_fmaf(r.w, w.w, part);
    }
}

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void attn_gate_kernel(const float* __restrict__ rows, float* __restrict__ s_out,
                                                                  const uint8_t* __restrict__ wchunks, int n_tot,
                                                                  int* __restrict__ range_flag) {
    using M = AgDims<D>;
    // two DISTINCT LDS objects, as in gw_layer_body: the DMA into one does not alias the reads of the other
    __shared__ __attribute__((aligned(16))) char s_a[M::CHUNK_BYTES];  // the odd chunks
    __shared__ __attribute__((aligned(16))) char s_b[M::CHUNK_BYTES];  // the even chunks
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const long long node0 = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;
    const bool valid = node0 < n_tot;
    const long long node = valid ? node0 : (long long)n_tot - 1;

    gw_issue_pieces<M::PIECES>(wchunks, s_b, M::PIECES, M::LAST_LANES, wave, lane);  // chunk 0
    // ---- the row, straight into the B operands; pieces at or beyond column D are zero
    float vmax = 0.0f;
    ds_uint4_t in_hi[M::KS1], in_lo[M::KS1];
    {
        const float* hr = rows + (size_t)node * D + 4 * g;
        float4 x[M::Q];
#pragma unroll
        for (int q = 0; q < M::Q; q++) x[q] = 16 * q + 4 * g < D ? *reinterpret_cast<const float4*>(hr + 16 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int q = 0; q < M::Q; q++) {
            vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, __builtin_fabsf(x[q].x)), __builtin_fabsf(x[q].y));
            vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, __builtin_fabsf(x[q].z)), __builtin_fabsf(x[q].w));
        }
#pragma unroll
        for (int ks = 0; ks < M::KS1; ks++) {
            DS_SPLIT2(x[2 * ks].x, x[2 * ks].y, in_hi[ks].x, in_lo[ks].x);
            DS_SPLIT2(x[2 * ks].z, x[2 * ks].w, in_hi[ks].y, in_lo[ks].y);
            DS_SPLIT2(x[2 * ks + 1].x, x[2 * ks + 1].y, in_hi[ks].z, in_lo[ks].z);
            DS_SPLIT2(x[2 * ks + 1].z, x[2 * ks + 1].w, in_hi[ks].w, in_lo[ks].w);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // chunk 0 is resident

    float part = 0.0f;
#pragma unroll 1
    for (int c = 0; c < M::STEPS; c += 2) {
        if (c + 1 < M::STEPS) gw_issue_pieces<M::PIECES>(wchunks + (size_t)(c + 1) * M::CHUNK_STRIDE, s_a, M::PIECES, M::LAST_LANES, wave, lane);
        ag_step<D>(s_b, lane, g, in_hi, in_lo, part, vmax);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of chunk c + 1 have landed
        __syncthreads();                                  // everyone's have; everyone is done with s_b
        if (c + 1 < M::STEPS) {
            if (c + 2 < M::STEPS) gw_issue_pieces<M::PIECES>(wchunks + (size_t)(c + 2) * M::CHUNK_STRIDE, s_b, M::PIECES, M::LAST_LANES, wave, lane);
            ag_step<D>(s_a, lane, g, in_hi, in_lo, part, vmax);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
    // ---- the four lane groups of a row, in a fixed order
    const float p0 = __shfl(part, j, 64), p1 = __shfl(part, j + 16, 64), p2 = __shfl(part, j + 32, 64), p3 = __shfl(part, j + 48, 64);
    if (valid && g == 0) s_out[node] = ((p0 + p1) + p2) + p3;
    if (__any(!(vmax < 6.0e4f))) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

// the exact form's H -> 1 product: s[v] = hid[v] . w2 in fp32.  One 16-lane group per row, the float4 pieces j, j + 16, ... in that
// order, then a fixed xor tree (node_logits_rows_kernel's shape)
template <int H>
__global__ __launch_bounds__(256) void attn_dot_kernel(const float* __restrict__ hid, const float* __restrict__ w2, float* __restrict__ s_out,
                                                       int n_tot) {
    constexpr int C = H / 4, K = (C + 15) / 16;
    const int j = threadIdx.x & 15;
    const long long v = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = v < n_tot;  // (no early return: the shuffles below are wave-wide)
    float part = 0.0f;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int c = j + 16 * k;
        if (live && c < C) {
            const float4 x = reinterpret_cast<const float4*>(hid)[(size_t)v * C + c];
            const float4 w = reinterpret_cast<const float4*>(w2)[c];
            part = __builtin_fmaf(x.x, w.x, part); part = __builtin_fmaf(x.y, w.y, part);
            part = __builtin_fmaf(x.z, w.z, part); part = __builtin_fmaf(x.w, w.w, part);
        }
    }
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
    if (live && j == 0) s_out[v] = part;
}

// pooled[g][:] = sum_v alpha[v] rows[v][:], alpha the softmax of the gates over graph g: one wavefront per graph, a lane owns the float4
// pieces lane, lane + 64, ...; every lane computes the same e[v] and Z, every column is one fma chain in node order -- the value depends
// on the graph alone.  A one-node graph: e = 1, Z = 1, pooled = the row exactly.
template <int D>
__global__ __launch_bounds__(256) void attn_pool_rows_kernel(const float* __restrict__ rows, const float* __restrict__ gate,
                                                             const int* __restrict__ node_off, float* __restrict__ pooled, int num_graphs) {
    constexpr int C = D / 4, K = (C + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int gi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gi >= num_graphs) return;
    const int n0 = node_off[gi], n1 = node_off[gi + 1];
    float m = -INFINITY;
    for (int v = n0 + lane; v < n1; v += 64) m = __builtin_fmaxf(m, gate[v]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, d, 64));
    float4 acc[K];
#pragma unroll
    for (int k = 0; k < K; k++) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    float z = 0.0f;
#pragma unroll 4
    for (int v = n0; v < n1; v++) {
        const float e = expf(gate[v] - m);
        z += e;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int c = lane + 64 * k;
            if (c < C) {
                const float4 x = reinterpret_cast<const float4*>(rows)[(size_t)v * C + c];
                acc[k].x = __builtin_fmaf(e, x.x, acc[k].x); acc[k].y = __builtin_fmaf(e, x.y, acc[k].y);
                acc[k].z = __builtin_fmaf(e, x.z, acc[k].z); acc[k].w = __builtin_fmaf(e, x.w, acc[k].w);
            }
        }
    }
    const bool any = n1 > n0;  // (a graph without nodes: zeros)
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int c = lane + 64 * k;
        if (c < C)
            reinterpret_cast<float4*>(pooled)[(size_t)gi * C + c] =
                any ? make_float4(acc[k].x / z, acc[k].y / z, acc[k].z / z, acc[k].w / z) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// w1 [H][D], b1 [H], w2 [H] (row-major, host) -> AgDims<D>::BYTES bytes
template <int D>
void ag_pack(const float* w1, const float* b1, const float* w2, uint8_t* out) {
    using M = AgDims<D>;
    constexpr int H = M::H;
    std::memset(out, 0, M::BYTES);
    const float s1 = gw_pow2_scale(w1, (size_t)H * D);
    for (int s = 0; s < M::STEPS; s++) {
        uint8_t* ck = out + (size_t)s * M::CHUNK_STRIDE;
        for (int tl = 0; tl < 2; tl++) {
            const int t = 2 * s + tl;
            gw_pack_tile(w1, H, D, 16 * t, s1, 0, M::KS1, ck + tl * 2048, 4096);
            for (int x = 0; x < 16; x++) {
                const int o = 16 * t + x;
                const float b = o < H ? b1[o] * s1 : 0.0f;
                const float w = o < H ? w2[o] / s1 : 0.0f;  // (a power of two: the product with the pre-scaled hidden value is the un-scaled one's)
                std::memcpy(ck + M::B1_OFF + tl * 64 + x * 4, &b, 4);
                std::memcpy(ck + M::W2_OFF + tl * 64 + x * 4, &w, 4);
            }
        }
    }
    gw_transpose(w1, H, D, reinterpret_cast<float*>(out + M::W1T_OFF));
    std::memcpy(out + M::B1F_OFF, b1, (size_t)H * 4);
    std::memcpy(out + M::W2F_OFF, w2, (size_t)H * 4);
}

constexpr int AG_D = FLOWGNN_EMB_DIM_OGB;  // the one instantiation

}  // namespace

size_t attn_pool_blob_bytes(int emb_dim) { return emb_dim == AG_D ? AgDims<AG_D>::BYTES : 0; }

void attn_pool_blob_pack(int emb_dim, const float* w1, const float* b1, const float* w2, void* out) {
    if (emb_dim == AG_D) ag_pack<AG_D>(w1, b1, w2, static_cast<uint8_t*>(out));
}

int launch_attn_gate(int emb_dim, const void* blob, const float* rows, float* s_out, float* hid, int n_tot, bool exact, int* range_flag,
                     hipStream_t s) {
    if (emb_dim != AG_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (n_tot <= 0) return 0;
    constexpr int D = AG_D, H = 2 * D;
    using M = AgDims<D>;
    const uint8_t* const b = static_cast<const uint8_t*>(blob);
    if (!exact) {
        attn_gate_kernel<D><<<(int)ceil_div_ll(n_tot, GW_ROWS), GW_WAVES * 64, 0, s>>>(rows, s_out, b, n_tot, range_flag);
    } else {
        launch_gw_dense_f32<D, H>(rows, reinterpret_cast<const float*>(b + M::W1T_OFF), reinterpret_cast<const float*>(b + M::B1F_OFF), hid, n_tot, 1, s);
        attn_dot_kernel<H><<<(int)ceil_div_ll(n_tot, 16), 256, 0, s>>>(hid, reinterpret_cast<const float*>(b + M::W2F_OFF), s_out, n_tot);
    }
    return 0;
}

int launch_attn_pool_rows(int emb_dim, const float* rows, const float* gate, const int* node_off, float* pooled, int num_graphs,
                          hipStream_t s) {
    if (emb_dim != AG_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (num_graphs <= 0) return 0;
    attn_pool_rows_kernel<AG_D><<<(num_graphs + 3) / 4, 256, 0, s>>>(rows, gate, node_off, pooled, num_graphs);
    return 0;
}

}  // namespace fg
