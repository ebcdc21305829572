// wide_common.h -- device code shared by the per-layer models of OGB's default width: gin_wide.hip (DESIGN.md sections 4.16, 4.17)
// and gcn_wide.hip (section 4.18).  Templates on the width D; every kernel here has internal linkage, so each of the two translation
// units compiles the instances it launches and nothing else.
#pragma once
#include "common.h"
#include "dense_split.h"

namespace fg {
namespace {

constexpr int GW_WAVES = 8;
constexpr int GW_ROWS = GW_WAVES * 16;  // rows of a workgroup

__device__ __forceinline__ float gw_relu(float x) {  // max(x, 0) as one integer max (gin_split.hip: gs_relu)
    const int b = __builtin_bit_cast(int, x);
    return __builtin_bit_cast(float, b > 0 ? b : 0);
}

// LDS-DMA of `pieces` 1 KiB pieces (64 lanes x 16 bytes; the last one `last_lanes` lanes wide) from gsrc to lds_buf, dealt round robin
// to the GW_WAVES waves of the workgroup.  MAXP: the largest `pieces` of the caller (the trip count).  Nothing is waited for here.
template <int MAXP>
__device__ __forceinline__ void gw_issue_pieces(const uint8_t* __restrict__ gsrc, char* lds_buf, int pieces, int last_lanes, int wave, int lane) {
#pragma unroll
    for (int p = 0; p < (MAXP + GW_WAVES - 1) / GW_WAVES; p++) {
        const int piece = wave + GW_WAVES * p;
        if (piece < pieces - 1 || (piece == pieces - 1 && lane < last_lanes)) {
            const uint8_t* g = gsrc + piece * 1024 + lane * 16;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)(lds_buf + piece * 1024), 16, 0, 0);
        }
    }
}

// out[v][o] = act(b[o] + sum_k in[v][k] wt[k][o]), k ascending; eight rows per workgroup staged in LDS, a thread owns output columns
template <int K, int O>
__global__ __launch_bounds__(256) void gw_dense_f32_kernel(const float* __restrict__ in, const float* __restrict__ wt, const float* __restrict__ b,
                                                           float* __restrict__ out, int n_tot, int relu_out) {
    constexpr int RB = 8;
    __shared__ float s_in[RB][K];
    const long long v0 = (long long)blockIdx.x * RB;
    for (int i = threadIdx.x; i < RB * K; i += 256) {
        const int r = i / K, k = i - r * K;
        s_in[r][k] = v0 + r < n_tot ? in[(size_t)(v0 + r) * K + k] : 0.0f;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < O; o += 256) {
        float acc[RB];
        const float bo = b[o];
#pragma unroll
        for (int r = 0; r < RB; r++) acc[r] = bo;
        for (int k = 0; k < K; k++) {
            const float w = wt[(size_t)k * O + o];
#pragma unroll
            for (int r = 0; r < RB; r++) acc[r] = __builtin_fmaf(s_in[r][k], w, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < RB; r++)
            if (v0 + r < n_tot) out[(size_t)(v0 + r) * O + o] = relu_out ? relu1(acc[r]) : acc[r];
    }
}

// ---------------------------------------------------------------- atom encoder and pooling at this width
// (atom_encoder_kernel<D> stages the 173-row table in LDS, and the readout kernels of device_common.h hold a row in half a wavefront:
// neither fits 75 float4 pieces.)  One lane per (node, float4 piece), the table read through the caches; summation order k = 0..8.
// VN: a tenth row, vn_e's piece, added after the nine table rows -- the bits of a separate add (GIN: x_0 = h_0 + E, section 4.17;
// GCN: x_0 = sum of nine projected rows + b_0, section 4.18)
template <int D, bool VN>
__device__ __forceinline__ void gw_atom_encoder_body(const int* __restrict__ node_feature, const float* __restrict__ table,
                                                     float* __restrict__ h, int n_tot, int* __restrict__ err, const float* __restrict__ vn_e) {
    constexpr int C = D / 4;
    const long long items = (long long)n_tot * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const long long v = i / C;
        const int c = (int)(i - v * C);
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < ND_FEATURE; k++) {
            int f = node_feature[v * ND_FEATURE + k];
            if (f < 0 || f >= c_nd_card[k]) {
                atomicMax(err, ERR_NODE_FEAT);
                f = 0;
            }
            const float4 w = reinterpret_cast<const float4*>(table)[(size_t)(c_nd_off[k] + f) * C + c];
            s.x += w.x; s.y += w.y; s.z += w.z; s.w += w.w;
        }
        if (VN) {
            const float4 w = reinterpret_cast<const float4*>(vn_e)[c];
            s.x += w.x; s.y += w.y; s.z += w.z; s.w += w.w;
        }
        reinterpret_cast<float4*>(h)[i] = s;
    }
}

template <int D>
__global__ __launch_bounds__(256) void gw_atom_encoder_kernel(const int* __restrict__ node_feature, const float* __restrict__ table,
                                                              float* __restrict__ h, int n_tot, int* __restrict__ err) {
    gw_atom_encoder_body<D, false>(node_feature, table, h, n_tot, err, nullptr);
}

template <int D>
__global__ __launch_bounds__(256) void gw_atom_encoder_vn_kernel(const int* __restrict__ node_feature, const float* __restrict__ table,
                                                                 float* __restrict__ h, int n_tot, int* __restrict__ err,
                                                                 const float* __restrict__ vn_e) {
    gw_atom_encoder_body<D, true>(node_feature, table, h, n_tot, err, vn_e);
}

// emb[g][:] = pool over the rows of graph g, in node order: one wavefront per graph, a lane owns the float4 pieces lane, lane + 64, ...
// -- every column is one chain in node order, so the value depends on the graph alone
template <int D, int OP>
__global__ __launch_bounds__(256) void gw_pool_rows_kernel(const float* __restrict__ rows, const int* __restrict__ node_off, float* __restrict__ emb,
                                                           int num_graphs) {
    constexpr int C = D / 4;
    const int lane = threadIdx.x & 63;
    const int gi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gi >= num_graphs) return;
    const int n0 = node_off[gi], n1 = node_off[gi + 1];
    const float n = (float)(n1 - n0);
    for (int c = lane; c < C; c += 64) {
        float4 acc = make_float4(pool_init<OP>(), pool_init<OP>(), pool_init<OP>(), pool_init<OP>());
        for (int v = n0; v < n1; v++) pool_fold4<OP>(acc, reinterpret_cast<const float4*>(rows)[(size_t)v * C + c]);
        reinterpret_cast<float4*>(emb)[(size_t)gi * C + c] =
            make_float4(pool_finish<OP>(acc.x, n), pool_finish<OP>(acc.y, n), pool_finish<OP>(acc.z, n), pool_finish<OP>(acc.w, n));
    }
}

inline float gw_pow2_scale(const float* w, size_t n) {
    float m = 0.0f;
    for (size_t i = 0; i < n; i++) m = std::fmax(m, std::fabs(w[i]));
    if (!(m > 0.0f) || !std::isfinite(m)) return 1.0f;
    return std::ldexp(1.0f, -std::ilogb(m));  // m * scale in [1, 2)
}

inline void gw_put_split(uint8_t* frag, int lane, int e, float v) {
    const _Float16 hi = (_Float16)v;  // to nearest even
    const _Float16 lo = (_Float16)(v - (float)hi);
    std::memcpy(frag + lane * 16 + e * 2, &hi, 2);
    std::memcpy(frag + 1024 + lane * 16 + e * 2, &lo, 2);
}

}  // namespace
}  // namespace fg
