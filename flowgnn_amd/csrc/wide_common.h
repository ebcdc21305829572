// wide_common.h -- what the per-layer models of OGB's default width share: gin_wide.hip (DESIGN.md sections 4.16, 4.17), gcn_wide.hip
// (sections 4.18, 4.19), wide_attn.hip (section 4.20) and wide_s2s.hip (section 4.23).  Device side: the LDS-DMA issue, the fp32 dense kernel, the atom encoder and
// the pooling kernel.  Host side: the fp32 launches, the split-f16 fragment packer, the transpose and the edge table of set_weights,
// and the readout (GwReadout).  Templates on the width D; every kernel here has internal linkage, so each translation unit compiles
// the instances it launches and nothing else.  The layer kernels' own bodies are NOT shared: section 4.21 says why.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "dense_split.h"
#include "wide_attn.h"  // the attention readout's two launches
#include "wide_s2s.h"   // the set2set readout's launches

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

// ---------------------------------------------------------------- host side: launches, packing, the readout
template <int K, int O>
inline void launch_gw_dense_f32(const float* in, const float* wt, const float* b, float* out, int rows, int relu_out, hipStream_t s) {
    gw_dense_f32_kernel<K, O><<<(int)ceil_div_ll(rows, 8), 256, 0, s>>>(in, wt, b, out, rows, relu_out);
}

// the fp32 MLP of the exact forms: out = act(W2 relu(W1 in + b1) + b2), D -> 2 D -> D, through hid [rows][2 D]; w1t / w2t are [K][O]
template <int D>
inline void launch_gw_mlp_f32(const float* in, const float* w1t, const float* b1, const float* w2t, const float* b2, float* hid, float* out,
                              int rows, int relu_out, hipStream_t s) {
    launch_gw_dense_f32<D, 2 * D>(in, w1t, b1, hid, rows, 1, s);
    launch_gw_dense_f32<2 * D, D>(hid, w2t, b2, out, rows, relu_out, s);
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

// The A operand of the split-f16 products: rows row0 .. row0 + 15 of the row-major w [rows][cols], times `scale`, as `nks` hi/lo
// fragment pairs (2 KiB each; K-steps ks0 .. ks0 + nks - 1) `stride` bytes apart from `base`.  Lane (i = lane & 15, gk = lane >> 4),
// slot e of K-step ks holds w[row0 + i][16 (2 ks + (e >> 2)) + 4 gk + (e & 3)]; what lies outside the matrix is zero.
inline void gw_pack_tile(const float* w, int rows, int cols, int row0, float scale, int ks0, int nks, uint8_t* base, size_t stride) {
    for (int lane = 0; lane < 64; lane++) {
        const int o = row0 + (lane & 15), gk = lane >> 4;
        for (int ks = ks0; ks < ks0 + nks; ks++)
            for (int e = 0; e < 8; e++) {
                const int k = 16 * (2 * ks + (e >> 2)) + 4 * gk + (e & 3);
                gw_put_split(base + (size_t)(ks - ks0) * stride, lane, e, (o < rows && k < cols) ? w[(size_t)o * cols + k] * scale : 0.0f);
            }
    }
}

// wt [K][O] = w [O][K] transposed: the exact forms read a weight row per k
inline void gw_transpose(const float* w, int O, int K, float* wt) {
    for (int o = 0; o < O; o++)
        for (int k = 0; k < K; k++) wt[(size_t)k * O + o] = w[(size_t)o * K + k];
}

// out [60][d]: a layer's combined edge rows, row (a0 * 6 + a1) * 2 + a2 = E[a0] + E[5 + a1] + E[11 + a2] of its 13 edge rows E
inline void gw_edge_combos(const float* E, int d, float* out) {
    static const int ed_off[3] = {0, 5, 11};
    for (int a0 = 0; a0 < 5; a0++)
        for (int a1 = 0; a1 < 6; a1++)
            for (int a2 = 0; a2 < 2; a2++)
                for (int k = 0; k < d; k++) {
                    float s = 0.0f;  // the order of GinModel::set_weights (GcnModel's is the same)
                    s += E[(ed_off[0] + a0) * d + k];
                    s += E[(ed_off[1] + a1) * d + k];
                    s += E[(ed_off[2] + a2) * d + k];
                    out[(size_t)((a0 * 6 + a1) * 2 + a2) * d + k] = s;
                }
}

// The readout of both models: the pooled rows (the caller's graph embeddings when they are on), then the head on them -- every
// NUM_TASK, every pooling -- and the per-node logit terms; or, in its place, the set2set readout with its own head (section 4.23).
// Owns the head's weights and the readouts' buffers; a member of the model.
template <int D>
struct GwReadout {
    int num_tasks = 1;
    float *d_pw = nullptr, *d_pb = nullptr;  // graph_pred_weights [NUM_TASK][D], bias [NUM_TASK]
    GrowBuf pooled;                          // the pooled rows [G][D] when graph embeddings are off
    GrowBuf attn_s;                          // the attention readout's gates [N] (section 4.20)
    GrowBuf s2s_h, s2s_c, s2s_r, s2s_e;      // the set2set readout's h_t, c_t, r_t [G][D] and dots e [N] (section 4.23)
    GrowBuf s2s_q, s2s_z;                    // ... and its exact form's q* [G][2 D] and z [G][4 D]

    int set_num_tasks(int t, bool& ready) {
        if (t < 1) return 8;
        if (t != num_tasks) ready = false;  // graph_pred_weights / bias change shape: set the weights again
        num_tasks = t;
        return 0;
    }
    int upload_head(const float* pw, const float* pb) {
        if (int rc = upload(&d_pw, std::vector<float>(pw, pw + (size_t)num_tasks * D))) return rc;
        return upload(&d_pb, std::vector<float>(pb, pb + num_tasks));
    }
    // in front of a forward's first launch: the gates [N], when the attention readout is on; the set2set readout's state, when that is
    int reserve(const DeviceBatch& db, bool exact) {
        if (db.s2s) {
            const size_t G = (size_t)db.b.num_graphs;
            if (int rc = s2s_h.reserve(G * D)) return rc;
            if (int rc = s2s_c.reserve(G * D)) return rc;
            if (int rc = s2s_r.reserve(G * D)) return rc;
            if (int rc = s2s_e.reserve((size_t)db.b.n_tot)) return rc;
            if (exact) {
                if (int rc = s2s_q.reserve(G * 2 * D)) return rc;
                if (int rc = s2s_z.reserve(G * 4 * D)) return rc;
            }
        }
        return db.attn_pool ? attn_s.reserve((size_t)db.b.n_tot) : 0;
    }
    // h5: the rows the pool is taken over; hid: the exact attention gate's hidden rows [N][2 D]
    int run(DeviceBatch& db, Profiler& prof, hipStream_t s, const float* h5, bool exact, float* hid) {
        const int n = db.b.n_tot, G = db.b.num_graphs;
        if (db.s2s) {  // OGB's set2set readout (section 4.23): per step the LSTM on the graphs' q*, the rows' dots with h_t, their softmax-weighted
                       // sum; then its own head on [h, r].  No graph embeddings and no node logits beside it (the engine refuses both)
            for (int t = 0; t < db.s2s_steps; t++) {
                {
                    ProfScope p(prof, "s2s_lstm", s);
                    if (int rc = launch_s2s_lstm(D, db.s2s, s2s_h.p, s2s_c.p, s2s_r.p, s2s_q.p, s2s_z.p, G, t == 0, exact, db.range_flag, s)) return rc;
                }
                {
                    ProfScope p(prof, "s2s_dot_rows", s);
                    if (int rc = launch_s2s_dot_rows(D, h5, s2s_h.p, db.b.node_off, s2s_e.p, G, s)) return rc;
                }
                ProfScope p(prof, "s2s_pool_rows", s);
                if (int rc = launch_attn_pool_rows(D, h5, s2s_e.p, db.b.node_off, s2s_r.p, G, s)) return rc;
            }
            ProfScope p(prof, "s2s_head", s);
            return launch_s2s_head(D, db.s2s, s2s_h.p, s2s_r.p, db.out, G, num_tasks, s);
        }
        float* out = db.emb;
        if (!out) {
            if (int rc = pooled.reserve((size_t)G * D)) return rc;
            out = pooled.p;
        }
        if (db.attn_pool) {  // OGB's attention readout (section 4.20): the gates of the rows, then their softmax-weighted sum per graph
            {
                ProfScope p(prof, "attn_gate", s);
                if (int rc = launch_attn_gate(D, db.attn_pool, h5, attn_s.p, hid, n, exact, db.range_flag, s)) return rc;
            }
            ProfScope p(prof, "attn_pool_rows", s);
            if (int rc = launch_attn_pool_rows(D, h5, attn_s.p, db.b.node_off, out, G, s)) return rc;
        } else {
            ProfScope p(prof, "mean_pool_rows", s);
            const int grid = (G + 3) / 4;
            if (db.pooling == POOL_OP_SUM) gw_pool_rows_kernel<D, POOL_OP_SUM><<<grid, 256, 0, s>>>(h5, db.b.node_off, out, G);
            else if (db.pooling == POOL_OP_MAX) gw_pool_rows_kernel<D, POOL_OP_MAX><<<grid, 256, 0, s>>>(h5, db.b.node_off, out, G);
            else gw_pool_rows_kernel<D, POOL_OP_MEAN><<<grid, 256, 0, s>>>(h5, db.b.node_off, out, G);
        }
        {
            ProfScope p(prof, "pooled_head", s);
            launch_pooled_head<D>(out, d_pw, d_pb, db.out, G, num_tasks, s);
        }
        if (db.node_logits) {
            ProfScope p(prof, "node_logits", s);
            launch_node_logits_rows<D>(h5, d_pw, d_pb, db.node_logits, n, num_tasks, s);
        }
        return 0;
    }
    void release() {
        if (d_pw) { (void)hipFree(d_pw); d_pw = nullptr; }
        if (d_pb) { (void)hipFree(d_pb); d_pb = nullptr; }
        pooled.release();
        attn_s.release();
        for (GrowBuf* b : {&s2s_h, &s2s_c, &s2s_r, &s2s_e, &s2s_q, &s2s_z}) b->release();
    }
};

}  // namespace
}  // namespace fg
