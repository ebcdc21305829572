// OGB's graph_pooling="set2set" readout at width 300 (flowgnn_set_set2set_pooling), for gin_wide.hip and
// gcn_wide.hip alike: their one readout (GwReadout, wide_common.h) calls the launch functions of wide_s2s.h, and wide_attn.h's
// launch_attn_pool_rows for the softmax-weighted sum, in place of its pool and head launches.  Per step t = 1 .. steps:
//   z        = W q*_{t-1} + b        W [4D][2D] = W_ih with W_hh added to its first D columns, b = b_ih + b_hh (q*'s first half is h_{t-1};
//                                     both folds in float64 on the host, rounded once);  z = (z_i, z_f, z_g, z_o)
//   c_t      = sigmoid(z_f) c_{t-1} + sigmoid(z_i) tanh(z_g);  h_t = sigmoid(z_o) tanh(c_t)
//   e[v]     = r[v] . h_t[g(v)];  r_t[g] = (sum_v a[v] r[v]) / (sum_v a[v]),  a[v] = exp(e[v] - max_{u in g} e[u])   (attn_pool_rows_kernel)
//   q*_t     = [h_t, r_t]
// and logit[g][k] = head_b[k] + head_W[k] . q*_steps[g].
//
// s2s_lstm_kernel<D>: one row per graph, the scheme of attn_gate_kernel -- a wave owns 16 rows and holds both halves of q* (h, r) in the
// B-operand layout of the f16 matrix pipe, split (DS_SPLIT2); an output step is one tile of 16 hidden units with its four gate tiles
// (i, f, g, o), so the cell runs in registers and z never goes to HBM.  K = 600 is cut into four quarters of five K-steps (h: K-steps
// 0..4, 5..9; r: the same), one chunk of the weight stream each: three f16 MFMAs per K-step and gate tile (w_hi x_hi + w_hi x_lo +
// w_lo x_hi, fp32 accumulate, W pre-scaled by a power of two and split on the host).  The stream goes L2 -> LDS by LDS-DMA into two
// distinct LDS objects, shared by the four waves of a 64-row workgroup (S2S_WAVES below says why four); s_waitcnt vmcnt(0) + one barrier
// per chunk.  Step 1 is s2s_cell_kernel alone: q*_0 = 0, so z is the bias.
//   lane (j = lane & 15, g = lane >> 4): row j of the wave's tile; B operand of K-step ks, slot e: feature 16 (2 ks + (e >> 2)) + 4 g + (e & 3);
//   C layout of unit tile t, gate tile gt, slot r: z_gt of hidden unit 16 t + 4 g + r.
// s2s_dot_rows_kernel<D>, s2s_head_kernel<D>: one wavefront per graph, gw_pool_rows_kernel's lane -> float4-piece ownership, no atomics.
#include "../../include/flowgnn.h"
#include "wide_common.h"  // (common.h, dense_split.h, wide_attn.h, wide_s2s.h)

namespace fg {
namespace {

template <int D>
struct S2sDims {
    static_assert(D % 4 == 0, "rows are read as float4 pieces");
    static constexpr int C = D / 4;
    static constexpr int KS = (D + 31) / 32;  // K-steps of one half of q* (K padded to 32 KS with zero weights)
    static_assert(KS % 2 == 0, "a half of q* is two chunks of KS / 2 K-steps");
    static constexpr int QK = KS / 2;           // K-steps of a chunk
    static constexpr int Q = 2 * KS;            // 16-feature pieces of a half a lane holds four floats of
    static constexpr int TILES = (D + 15) / 16;  // unit tiles (D padded to 16 TILES with zero weights)
    static constexpr int CHUNKS = 4 * TILES;    // chunk 4 t + q: unit tile t, quarter q (0, 1: h; 2, 3: r)
    // a chunk, in 1 KiB fragments (64 lanes x 8 halves): fragment ((kq * 4 + gt) * 2 + p), kq the K-step in the quarter, gt the gate, p = 0 hi, 1 lo
    static constexpr int CHUNK_BYTES = QK * 4 * 2 * 1024;
    static constexpr int PIECES = CHUNK_BYTES / 1024;
    static_assert(2 * CHUNK_BYTES <= 160 * 1024, "two weight buffers must fit the CU's LDS");
    // the blob: the stream | b pre-scaled [TILES][4][16] | 1 / scale (one float, padded to 16 bytes) | W^T [2D][4D] | b [4D] | head_w [T][2D] | head_b [T]
    static constexpr size_t STREAM_BYTES = (size_t)CHUNKS * CHUNK_BYTES;
    static constexpr size_t BIAS_OFF = STREAM_BYTES;
    static constexpr size_t SCALE_OFF = BIAS_OFF + (size_t)TILES * 4 * 16 * 4;
    static constexpr size_t WT_OFF = SCALE_OFF + 16;
    static constexpr size_t BF_OFF = WT_OFF + (size_t)2 * D * 4 * D * 4;
    static constexpr size_t HEADW_OFF = BF_OFF + (size_t)4 * D * 4;
    static constexpr size_t headb_off(int T) { return HEADW_OFF + (size_t)T * 2 * D * 4; }
    static constexpr size_t bytes(int T) { return (headb_off(T) + (size_t)T * 4 + 15) / 16 * 16; }
    static_assert(BIAS_OFF % 16 == 0 && WT_OFF % 16 == 0 && BF_OFF % 16 == 0 && HEADW_OFF % 16 == 0, "the parts are read in 16-byte pieces");
};

// The LSTM kernel's workgroup: four waves of 16 rows, one per SIMD, so that a wave may hold both halves of q* as split operands (160
// VGPRs) beside its accumulators and weight fragments without scratch -- eight waves of 256 registers do not allow it (section 4.23)
constexpr int S2S_WAVES = 4;
constexpr int S2S_ROWS = S2S_WAVES * 16;

// LDS-DMA of a chunk of PIECES whole 1 KiB pieces (64 lanes x 16 bytes) from gsrc to lds_buf, dealt round robin to the workgroup's
// waves (gw_issue_pieces for this workgroup size).  Nothing is waited for here.
template <int PIECES>
__device__ __forceinline__ void s2s_issue_chunk(const uint8_t* __restrict__ gsrc, char* lds_buf, int wave, int lane) {
    static_assert(PIECES % S2S_WAVES == 0, "every wave issues the same number of pieces");
#pragma unroll
    for (int p = 0; p < PIECES / S2S_WAVES; p++) {
        const int piece = wave + S2S_WAVES * p;
        const uint8_t* g = gsrc + piece * 1024 + lane * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                         (__attribute__((address_space(3))) void*)(lds_buf + piece * 1024), 16, 0, 0);
    }
}

// safe at saturation: expf gives 0 or inf there, never inf - inf
__device__ __forceinline__ float s2s_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float s2s_tanh(float x) { return 1.0f - 2.0f / (expf(2.0f * x) + 1.0f); }

__device__ __forceinline__ void s2s_cell(float zi, float zf, float zg, float zo, float c_prev, float& h, float& c) {
    c = __builtin_fmaf(s2s_sigmoid(zf), c_prev, s2s_sigmoid(zi) * s2s_tanh(zg));
    h = s2s_sigmoid(zo) * s2s_tanh(c);
}

// the cell on a lane's four units of a tile: acc = scale * z of the four gates
__device__ __forceinline__ void s2s_cell4(const float4_t (&acc)[4], float inv_s, const float4& cp, float4& hn, float4& cn) {
    s2s_cell(acc[0].x * inv_s, acc[1].x * inv_s, acc[2].x * inv_s, acc[3].x * inv_s, cp.x, hn.x, cn.x);
    s2s_cell(acc[0].y * inv_s, acc[1].y * inv_s, acc[2].y * inv_s, acc[3].y * inv_s, cp.y, hn.y, cn.y);
    s2s_cell(acc[0].z * inv_s, acc[1].z * inv_s, acc[2].z * inv_s, acc[3].z * inv_s, cp.z, hn.z, cn.z);
    s2s_cell(acc[0].w * inv_s, acc[1].w * inv_s, acc[2].w * inv_s, acc[3].w * inv_s, cp.w, hn.w, cn.w);
}

// K-steps K0 .. K0 + QK - 1 of a half of q* of the lane's row, straight into the B operands; pieces at or beyond column D are zero.
template <int D, int K0>
__device__ __forceinline__ void s2s_load_quarter(const float* hr, int g, ds_uint4_t (&hi)[S2sDims<D>::KS], ds_uint4_t (&lo)[S2sDims<D>::KS], float& vmax) {
    using M = S2sDims<D>;
    float4 x[2 * M::QK];
#pragma unroll
    for (int q = 0; q < 2 * M::QK; q++)
        x[q] = 16 * (2 * K0 + q) + 4 * g < D ? *reinterpret_cast<const float4*>(hr + 16 * (2 * K0 + q)) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < 2 * M::QK; q++) {
        vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, __builtin_fabsf(x[q].x)), __builtin_fabsf(x[q].y));
        vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, __builtin_fabsf(x[q].z)), __builtin_fabsf(x[q].w));
    }
#pragma unroll
    for (int k = 0; k < M::QK; k++) {
        DS_SPLIT2(x[2 * k].x, x[2 * k].y, hi[K0 + k].x, lo[K0 + k].x);
        DS_SPLIT2(x[2 * k].z, x[2 * k].w, hi[K0 + k].y, lo[K0 + k].y);
        DS_SPLIT2(x[2 * k + 1].x, x[2 * k + 1].y, hi[K0 + k].z, lo[K0 + k].z);
        DS_SPLIT2(x[2 * k + 1].z, x[2 * k + 1].w, hi[K0 + k].w, lo[K0 + k].w);
    }
}

// one chunk from `wb`: K-steps K0 .. K0 + QK - 1 of a half, the four gate tiles
template <int D, int K0>
__device__ __forceinline__ void s2s_step(const char* wb, int lane, const ds_uint4_t (&hi)[S2sDims<D>::KS], const ds_uint4_t (&lo)[S2sDims<D>::KS],
                                         float4_t (&acc)[4]) {
    using M = S2sDims<D>;
#pragma unroll
    for (int kq = 0; kq < M::QK; kq++) {
        ds_uint4_t a[4][2];
#pragma unroll
        for (int gt = 0; gt < 4; gt++)
#pragma unroll
            for (int p = 0; p < 2; p++) a[gt][p] = *reinterpret_cast<const ds_uint4_t*>(wb + ((kq * 4 + gt) * 2 + p) * 1024 + lane * 16);
#pragma unroll
        for (int gt = 0; gt < 4; gt++) acc[gt] = DS_MFMA16(a[gt][0], hi[K0 + kq], acc[gt]);
#pragma unroll
        for (int gt = 0; gt < 4; gt++) acc[gt] = DS_MFMA16(a[gt][0], lo[K0 + kq], acc[gt]);
#pragma unroll
        for (int gt = 0; gt < 4; gt++) acc[gt] = DS_MFMA16(a[gt][1], hi[K0 + kq], acc[gt]);
    }
}

template <int D>
__global__ __launch_bounds__(S2S_WAVES * 64) void s2s_lstm_kernel(float* h, float* c, const float* __restrict__ r, const uint8_t* __restrict__ blob,
                                                                 int num_graphs, int* __restrict__ range_flag) {
    using M = S2sDims<D>;
    // two DISTINCT LDS objects, as in attn_gate_kernel: the DMA into one does not alias the reads of the other
    __shared__ __attribute__((aligned(16))) char s_a[M::CHUNK_BYTES];  // the odd chunks
    __shared__ __attribute__((aligned(16))) char s_b[M::CHUNK_BYTES];  // the even chunks
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const long long row0 = (long long)blockIdx.x * S2S_ROWS + wave * 16 + j;
    const bool valid = row0 < num_graphs;
    const long long row = valid ? row0 : (long long)num_graphs - 1;
    const float* const bias = reinterpret_cast<const float*>(blob + M::BIAS_OFF);
    const float inv_s = *reinterpret_cast<const float*>(blob + M::SCALE_OFF);

    const uint8_t* const wchunks = blob;
    s2s_issue_chunk<M::PIECES>(wchunks, s_b, wave, lane);  // chunk 0
    float vmax = 0.0f;
    ds_uint4_t h_hi[M::KS], h_lo[M::KS], r_hi[M::KS], r_lo[M::KS];
    s2s_load_quarter<D, 0>(h + (size_t)row * D + 4 * g, g, h_hi, h_lo, vmax);
    s2s_load_quarter<D, M::QK>(h + (size_t)row * D + 4 * g, g, h_hi, h_lo, vmax);
    s2s_load_quarter<D, 0>(r + (size_t)row * D + 4 * g, g, r_hi, r_lo, vmax);
    s2s_load_quarter<D, M::QK>(r + (size_t)row * D + 4 * g, g, r_hi, r_lo, vmax);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // chunk 0 is resident; every row of h this workgroup rewrites has been read

#pragma unroll 1
    for (int t = 0; t < M::TILES; t++) {
        const uint8_t* const wt = wchunks + (size_t)(4 * t) * M::CHUNK_BYTES;
        const int u = 16 * t + 4 * g;
        const bool live = valid && u < D;
        float4_t acc[4];
#pragma unroll
        for (int gt = 0; gt < 4; gt++) {
            const float4 b = *reinterpret_cast<const float4*>(bias + (t * 4 + gt) * 16 + g * 4);
            acc[gt] = (float4_t){b.x, b.y, b.z, b.w};
        }
        const float4 cp = live ? *reinterpret_cast<const float4*>(c + (size_t)row * D + u) : make_float4(0.f, 0.f, 0.f, 0.f);
        // quarter 0 (h, K-steps 0 ..) from s_b
        s2s_issue_chunk<M::PIECES>(wt + 1 * M::CHUNK_BYTES, s_a, wave, lane);
        s2s_step<D, 0>(s_b, lane, h_hi, h_lo, acc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of the next chunk have landed
        __syncthreads();                                  // everyone's have; everyone is done with s_b
        // quarter 1 (h, K-steps QK ..) from s_a
        s2s_issue_chunk<M::PIECES>(wt + 2 * M::CHUNK_BYTES, s_b, wave, lane);
        s2s_step<D, M::QK>(s_a, lane, h_hi, h_lo, acc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // quarter 2 (r, K-steps 0 ..) from s_b
        s2s_issue_chunk<M::PIECES>(wt + 3 * M::CHUNK_BYTES, s_a, wave, lane);
        s2s_step<D, 0>(s_b, lane, r_hi, r_lo, acc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // quarter 3 (r, K-steps QK ..) from s_a
        if (t + 1 < M::TILES) s2s_issue_chunk<M::PIECES>(wt + 4 * M::CHUNK_BYTES, s_b, wave, lane);
        s2s_step<D, M::QK>(s_a, lane, r_hi, r_lo, acc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        float4 hn, cn;
        s2s_cell4(acc, inv_s, cp, hn, cn);
        if (live) {
            *reinterpret_cast<float4*>(h + (size_t)row * D + u) = hn;
            *reinterpret_cast<float4*>(c + (size_t)row * D + u) = cn;
        }
    }
    if (__any(!(vmax < 6.0e4f))) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

// the exact form: q [G][2D] = [h, r], the input of gw_dense_f32_kernel<2D, 4D>
template <int D>
__global__ __launch_bounds__(256) void s2s_concat_kernel(const float* __restrict__ h, const float* __restrict__ r, float* __restrict__ q,
                                                         int num_graphs) {
    constexpr int C = D / 4;
    const long long items = (long long)num_graphs * 2 * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const long long gi = i / (2 * C);
        const int p = (int)(i - gi * 2 * C);
        reinterpret_cast<float4*>(q)[i] = p < C ? reinterpret_cast<const float4*>(h)[gi * C + p] : reinterpret_cast<const float4*>(r)[gi * C + p - C];
    }
}

// the cell alone: the first step of both forms (z null: q*_0 = 0 and h_0 = c_0 = 0, so z is bf [4D] for every graph and nothing else is
// read) and the exact form's later steps (z [G][4D], bias included)
template <int D>
__global__ __launch_bounds__(256) void s2s_cell_kernel(const float* __restrict__ z, const float* __restrict__ bf, float* __restrict__ h,
                                                       float* __restrict__ c, int num_graphs) {
    const long long items = (long long)num_graphs * D;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const long long gi = i / D;
        const int u = (int)(i - gi * D);
        const float* const zr = z ? z + (size_t)gi * 4 * D : bf;
        float hn, cn;
        s2s_cell(zr[u], zr[D + u], zr[2 * D + u], zr[3 * D + u], z ? c[i] : 0.0f, hn, cn);
        h[i] = hn;
        c[i] = cn;
    }
}

// e[v] = rows[v] . h[g(v)]: one wavefront per graph, a lane owns the float4 pieces lane, lane + 64 of the row and of h (loaded once per
// graph); per node one fma chain per lane over its pieces in ascending order (x, y, z, w of each), then a fixed xor tree over the 64 lanes,
// distances 32, 16, 8, 4, 2, 1 -- the value depends on the row and the graph's h alone
template <int D>
__global__ __launch_bounds__(256) void s2s_dot_rows_kernel(const float* __restrict__ rows, const float* __restrict__ h, const int* __restrict__ node_off,
                                                           float* __restrict__ e, int num_graphs) {
    constexpr int C = D / 4, K = (C + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int gi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gi >= num_graphs) return;  // (a whole wavefront: the shuffles below stay wave-wide)
    const int n0 = node_off[gi], n1 = node_off[gi + 1];
    float4 hp[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int cc = lane + 64 * k;
        hp[k] = cc < C ? reinterpret_cast<const float4*>(h)[(size_t)gi * C + cc] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int v = n0; v < n1; v++) {
        float part = 0.0f;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int cc = lane + 64 * k;
            if (cc < C) {
                const float4 x = reinterpret_cast<const float4*>(rows)[(size_t)v * C + cc];
                part = __builtin_fmaf(x.x, hp[k].x, part); part = __builtin_fmaf(x.y, hp[k].y, part);
                part = __builtin_fmaf(x.z, hp[k].z, part); part = __builtin_fmaf(x.w, hp[k].w, part);
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
        if (lane == 0) e[v] = part;
    }
}

// out[g][k] = head_b[k] + head_w[k] . [h[g], r[g]]: one wavefront per graph, the same ownership; per task one fma chain per lane (its
// pieces of h, then of r), then the same xor tree
template <int D>
__global__ __launch_bounds__(256) void s2s_head_kernel(const float* __restrict__ h, const float* __restrict__ r, const float* __restrict__ hw,
                                                       const float* __restrict__ hb, float* __restrict__ out, int num_graphs, int num_tasks) {
    constexpr int C = D / 4, K = (C + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int gi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gi >= num_graphs) return;
    float4 hp[K], rp[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int cc = lane + 64 * k;
        hp[k] = cc < C ? reinterpret_cast<const float4*>(h)[(size_t)gi * C + cc] : make_float4(0.f, 0.f, 0.f, 0.f);
        rp[k] = cc < C ? reinterpret_cast<const float4*>(r)[(size_t)gi * C + cc] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int t = 0; t < num_tasks; t++) {
        const float4* const w = reinterpret_cast<const float4*>(hw) + (size_t)t * 2 * C;
        float part = 0.0f;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int cc = lane + 64 * k;
            if (cc < C) {
                const float4 x = w[cc];
                part = __builtin_fmaf(hp[k].x, x.x, part); part = __builtin_fmaf(hp[k].y, x.y, part);
                part = __builtin_fmaf(hp[k].z, x.z, part); part = __builtin_fmaf(hp[k].w, x.w, part);
            }
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int cc = lane + 64 * k;
            if (cc < C) {
                const float4 x = w[C + cc];
                part = __builtin_fmaf(rp[k].x, x.x, part); part = __builtin_fmaf(rp[k].y, x.y, part);
                part = __builtin_fmaf(rp[k].z, x.z, part); part = __builtin_fmaf(rp[k].w, x.w, part);
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
        if (lane == 0) out[(size_t)gi * num_tasks + t] = hb[t] + part;
    }
}

// the six host tensors (row-major) -> S2sDims<D>::bytes(T) bytes
template <int D>
void s2s_pack(int T, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* head_w, const float* head_b,
              uint8_t* out) {
    using M = S2sDims<D>;
    constexpr int O = 4 * D, K = 2 * D;
    std::memset(out, 0, M::bytes(T));
    // the fold: q*_{t-1}'s first half is h_{t-1}, so W_hh goes into W_ih's first D columns and the biases into one -- float64, rounded once
    std::vector<float> w((size_t)O * K), b(O);
    for (int o = 0; o < O; o++) {
        for (int k = 0; k < K; k++)
            w[(size_t)o * K + k] = k < D ? (float)((double)w_ih[(size_t)o * K + k] + (double)w_hh[(size_t)o * D + k]) : w_ih[(size_t)o * K + k];
        b[o] = (float)((double)b_ih[o] + (double)b_hh[o]);
    }
    const float s1 = gw_pow2_scale(w.data(), w.size());
    std::vector<float> sub((size_t)D * D);  // gate gt's rows, one half's columns: what gw_pack_tile pads with zeros is outside THIS matrix
    for (int gt = 0; gt < 4; gt++)
        for (int half = 0; half < 2; half++) {
            for (int o = 0; o < D; o++)
                std::memcpy(&sub[(size_t)o * D], &w[(size_t)(gt * D + o) * K + half * D], sizeof(float) * D);
            for (int t = 0; t < M::TILES; t++)
                for (int qq = 0; qq < 2; qq++)
                    gw_pack_tile(sub.data(), D, D, 16 * t, s1, qq * M::QK, M::QK, out + (size_t)(4 * t + 2 * half + qq) * M::CHUNK_BYTES + gt * 2048,
                                 4 * 2048);
        }
    float* const bias = reinterpret_cast<float*>(out + M::BIAS_OFF);
    for (int t = 0; t < M::TILES; t++)
        for (int gt = 0; gt < 4; gt++)
            for (int x = 0; x < 16; x++) bias[(t * 4 + gt) * 16 + x] = 16 * t + x < D ? b[gt * D + 16 * t + x] * s1 : 0.0f;
    const float inv = 1.0f / s1;  // (a power of two: the product with the pre-scaled accumulator is the un-scaled one's)
    std::memcpy(out + M::SCALE_OFF, &inv, 4);
    gw_transpose(w.data(), O, K, reinterpret_cast<float*>(out + M::WT_OFF));
    std::memcpy(out + M::BF_OFF, b.data(), sizeof(float) * O);
    std::memcpy(out + M::HEADW_OFF, head_w, sizeof(float) * (size_t)T * K);
    std::memcpy(out + M::headb_off(T), head_b, sizeof(float) * T);
}

constexpr int S2S_D = FLOWGNN_EMB_DIM_OGB;  // the one instantiation

}  // namespace

size_t s2s_blob_bytes(int emb_dim, int num_tasks) { return emb_dim == S2S_D && num_tasks >= 1 ? S2sDims<S2S_D>::bytes(num_tasks) : 0; }

void s2s_blob_pack(int emb_dim, int num_tasks, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* head_w,
                   const float* head_b, void* out) {
    if (emb_dim == S2S_D) s2s_pack<S2S_D>(num_tasks, w_ih, w_hh, b_ih, b_hh, head_w, head_b, static_cast<uint8_t*>(out));
}

int launch_s2s_lstm(int emb_dim, const void* blob, float* h, float* c, const float* r, float* q, float* z, int num_graphs, bool first,
                    bool exact, int* range_flag, hipStream_t s) {
    if (emb_dim != S2S_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (num_graphs <= 0) return 0;
    constexpr int D = S2S_D;
    using M = S2sDims<D>;
    const uint8_t* const b = static_cast<const uint8_t*>(blob);
    const float* const bf = reinterpret_cast<const float*>(b + M::BF_OFF);
    if (!exact && !first) {
        s2s_lstm_kernel<D><<<(int)ceil_div_ll(num_graphs, S2S_ROWS), S2S_WAVES * 64, 0, s>>>(h, c, r, b, num_graphs, range_flag);
        return 0;
    }
    if (!first) {
        s2s_concat_kernel<D><<<grid_for((long long)num_graphs * 2 * M::C, 256, 256 * 8), 256, 0, s>>>(h, r, q, num_graphs);
        launch_gw_dense_f32<2 * D, 4 * D>(q, reinterpret_cast<const float*>(b + M::WT_OFF), bf, z, num_graphs, 0, s);
    }
    s2s_cell_kernel<D><<<grid_for((long long)num_graphs * D, 256, 256 * 8), 256, 0, s>>>(first ? nullptr : z, bf, h, c, num_graphs);
    return 0;
}

int launch_s2s_dot_rows(int emb_dim, const float* rows, const float* h, const int* node_off, float* e, int num_graphs, hipStream_t s) {
    if (emb_dim != S2S_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (num_graphs <= 0) return 0;
    s2s_dot_rows_kernel<S2S_D><<<(num_graphs + 3) / 4, 256, 0, s>>>(rows, h, node_off, e, num_graphs);
    return 0;
}

int launch_s2s_head(int emb_dim, const void* blob, const float* h, const float* r, float* out, int num_graphs, int num_tasks, hipStream_t s) {
    if (emb_dim != S2S_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (num_graphs <= 0) return 0;
    using M = S2sDims<S2S_D>;
    const uint8_t* const b = static_cast<const uint8_t*>(blob);
    s2s_head_kernel<S2S_D><<<(num_graphs + 3) / 4, 256, 0, s>>>(h, r, reinterpret_cast<const float*>(b + M::HEADW_OFF),
                                                                reinterpret_cast<const float*>(b + M::headb_off(num_tasks)), out, num_graphs, num_tasks);
    return 0;
}

}  // namespace fg
