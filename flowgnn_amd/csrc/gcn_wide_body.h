// gcn_wide_body.h -- the bodies of GCN's fused kernels at width 300: the weight stream's layout (GcwDims), the
// walk with its epilogue (gcw_walk), one step of the product (gcw_step), the virtual node's add and partial rows (gcw_vn_add_partials),
// and gcw_layer_body, whose instances are the kernels of two translation units.  gcn_wide.hip has the two it always had (EXT = false:
// the layer and its virtual-node instance), gcn_wide_jk.hip the two with OGB's residual=True and JK="sum" behind the walk (EXT = true;
// flowgnn_set_model_jk_residual, section 4.25) and the final stage with them (gcw_final_jk_body).  EXT is a compile-time constant:
// with it false the extra code does not exist and a kernel is the one it was before this header did.
#pragma once
#include <type_traits>

#include "common.h"
#include "dense_split.h"
#include "gcn_ogbvn.h"
#include "wide_common.h"

namespace fg {
namespace {

template <int D>
struct GcwDims {
    static_assert(D % 4 == 0, "rows are read as float4 pieces");
    static constexpr int C = D / 4;               // float4 pieces of a row
    static constexpr int KS = (D + 31) / 32;      // K-steps of the product (K padded to 32 KS)
    static constexpr int Q = 2 * KS;              // 16-feature pieces a lane holds four floats of
    static constexpr int T = (D + 15) / 16;       // 16-row output tiles, the last one masked at column D
    static constexpr int TPC = 2;                 // output tiles of a chunk of the weight stream
    static constexpr int STEPS = (T + TPC - 1) / TPC;
    static_assert(STEPS % 2 == 0, "the step loop alternates two LDS buffers");
    // chunk c, in 1 KiB fragments (64 lanes x 8 halves): output tile TPC c + tl, K-step ks, p = 0 hi, 1 lo: fragment (tl KS + ks) 2 + p;
    // tiles at or beyond T are zeros (their products are computed and dropped)
    static constexpr int TILE_BYTES = KS * 2 * 1024;
    static constexpr int CHUNK_BYTES = TPC * TILE_BYTES;
    static constexpr int PIECES = CHUNK_BYTES / 1024;
    static constexpr size_t LAYER_BYTES = (size_t)STEPS * CHUNK_BYTES;
    // per layer, contiguous in global memory and in LDS: the 60 combined edge rows | root | folded BN scale | folded BN shift
    static constexpr int ECOMB_FLOATS = EDGE_COMBOS * D;
    static constexpr int TAB_FLOATS = ECOMB_FLOATS + 3 * D;
    static constexpr int TAB_BYTES = TAB_FLOATS * 4;
    static constexpr int TAB_PIECES = (TAB_BYTES + 1023) / 1024;
    static constexpr int TAB_LAST_LANES = (TAB_BYTES - (TAB_PIECES - 1) * 1024) / 16;
    static_assert(TAB_BYTES % 16 == 0, "the table is copied in 16-byte pieces");
    static_assert(2 * CHUNK_BYTES + TAB_BYTES <= 160 * 1024, "two weight buffers and the table must fit the CU's LDS");
    static constexpr int SCALE_AT = STEPS * TPC * 16;  // per layer, read from global memory: b pre-scaled and padded, then 1 / s
    static constexpr int TAIL_FLOATS = SCALE_AT + 4;
};

// a[v] = act(BN(m[v] + relu(x[v] + root) / (deg(v) + 1))) of this lane's node in the B-operand layout; s_tab: the layer's table in LDS.
// The accumulate is an explicit fma at every place this is inlined (GcnAggPolicy::edge says why), and so is the epilogue.
template <int D, bool RELU_OUT>
__device__ __forceinline__ void gcw_walk(const float* __restrict__ x, const int* __restrict__ row_ptr, const int* __restrict__ src,
                                         const uint8_t* __restrict__ ecode, const float* __restrict__ esc, const int* __restrict__ out_deg,
                                         const float* s_tab, long long node, bool valid, int g, float (&a)[4 * GcwDims<D>::Q]) {
    using M = GcwDims<D>;
    int e = row_ptr[node];
    const int e_end = valid ? row_ptr[node + 1] : e;
    const int dv = out_deg[node];
    const float dinv_v = dv > 0 ? 1.0f / sqrtf((float)(dv + 1)) : 0.0f;
    const float idp1 = 1.0f / (float)(dv + 1);
#pragma unroll
    for (int k = 0; k < 4 * M::Q; k++) a[k] = 0.0f;
    int u_nx = 0, c_nx = 0;
    float n_nx = 0.0f;
    if (e < e_end) { u_nx = src[e]; c_nx = ecode[e]; n_nx = esc[e]; }
    // Piece q of a row is columns 16 q + 4 g .. + 3.  The one piece that straddles column D (D % 16 != 0) is read by the lanes beyond D
    // from the row's last four columns instead -- in bounds, and no branch inside the walk; what those lanes hold of it is zeroed
    // at the end, so pieces at or beyond column D stay zero.  NQ: the pieces that exist.
    constexpr int NQ = M::T;
    const int o_last = 16 * (NQ - 1) < D - 4 - 4 * g ? 16 * (NQ - 1) : D - 4 - 4 * g;
#define GCW_OFF(q) (16 * (q) + 16 > D ? o_last : 16 * (q))
    // ---- one in-edge per trip, in CSR order (a row's sum depends on the row alone); the CSR entry one edge ahead of the row loads
    // (a lane whose row is done runs the trip with norm 0 on the entry it read last, or on row 0: fma(0, finite, a) is a, and the 4 Q
    // accumulators are updated on one path -- under `if (e < e_end)` they were copied to and fro on every trip)
    while (__any(e < e_end)) {
        const int u = u_nx, code = c_nx;
        const float norm = e < e_end ? n_nx * dinv_v : 0.0f;
        e += e < e_end;
        if (e < e_end) { u_nx = src[e]; c_nx = ecode[e]; n_nx = esc[e]; }
        const float* hr = x + (size_t)u * D + 4 * g;
        const float* er = s_tab + code * D + 4 * g;
#pragma unroll
        for (int q0 = 0; q0 < NQ; q0 += M::KS) {
            if (q0) __builtin_amdgcn_sched_barrier(0);  // (one half row in flight, not both)
            float4 xv[M::KS];
#pragma unroll
            for (int q = 0; q < M::KS; q++)
                if (q0 + q < NQ) xv[q] = *reinterpret_cast<const float4*>(hr + GCW_OFF(q0 + q));
#pragma unroll
            for (int q = 0; q < M::KS; q++)
                if (q0 + q < NQ) {
                    const float4 w = *reinterpret_cast<const float4*>(er + GCW_OFF(q0 + q));
                    float r0 = __builtin_fmaf(norm, relu1(w.x + xv[q].x), a[4 * (q0 + q) + 0]);
                    float r1 = __builtin_fmaf(norm, relu1(w.y + xv[q].y), a[4 * (q0 + q) + 1]);
                    float r2 = __builtin_fmaf(norm, relu1(w.z + xv[q].z), a[4 * (q0 + q) + 2]);
                    float r3 = __builtin_fmaf(norm, relu1(w.w + xv[q].w), a[4 * (q0 + q) + 3]);
                    asm volatile("" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3));  // (computed in this trip, not carried into the next)
                    a[4 * (q0 + q) + 0] = r0; a[4 * (q0 + q) + 1] = r1; a[4 * (q0 + q) + 2] = r2; a[4 * (q0 + q) + 3] = r3;
                }
        }
    }
    // ---- the node's own row, after the walk (another 4 Q registers before it), and the epilogue: root, 1 / (deg + 1), folded BatchNorm
    const float* xr = x + (size_t)node * D + 4 * g;
    const float* ep = s_tab + M::ECOMB_FLOATS + 4 * g;
    // (a fence every four pieces: left alone, the scheduler hoists all 4 Q row loads and 12 Q table reads above the first FMA, and spills)
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        if (q % 4 == 0) __builtin_amdgcn_sched_barrier(0);
        const float4 xs = *reinterpret_cast<const float4*>(xr + GCW_OFF(q));
        const float4 rt = *reinterpret_cast<const float4*>(ep + GCW_OFF(q));
        const float4 sc = *reinterpret_cast<const float4*>(ep + D + GCW_OFF(q));
        const float4 sh = *reinterpret_cast<const float4*>(ep + 2 * D + GCW_OFF(q));
        float r0 = __builtin_fmaf(__builtin_fmaf(relu1(xs.x + rt.x), idp1, a[4 * q + 0]), sc.x, sh.x);
        float r1 = __builtin_fmaf(__builtin_fmaf(relu1(xs.y + rt.y), idp1, a[4 * q + 1]), sc.y, sh.y);
        float r2 = __builtin_fmaf(__builtin_fmaf(relu1(xs.z + rt.z), idp1, a[4 * q + 2]), sc.z, sh.z);
        float r3 = __builtin_fmaf(__builtin_fmaf(relu1(xs.w + rt.w), idp1, a[4 * q + 3]), sc.w, sh.w);
        if (RELU_OUT) { r0 = relu1(r0); r1 = relu1(r1); r2 = relu1(r2); r3 = relu1(r3); }
        if (16 * q + 16 > D && 16 * q + 4 * g >= D) r0 = r1 = r2 = r3 = 0.0f;  // the straddling piece, beyond column D
        asm volatile("" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3));  // (computed here, not sunk to where the value is used)
        a[4 * q + 0] = r0; a[4 * q + 1] = r1; a[4 * q + 2] = r2; a[4 * q + 3] = r3;
    }
#undef GCW_OFF
}

// the TPC output tiles of chunk c from the fragments in `wb`: three f16 MFMAs per product, stored as soon as they are done
template <int D>
__device__ __forceinline__ void gcw_step(const char* wb, int c, int lane, int g, const ds_uint4_t (&in_hi)[GcwDims<D>::KS],
                                         const ds_uint4_t (&in_lo)[GcwDims<D>::KS], const float* __restrict__ tailp, float oscale,
                                         float* __restrict__ row, bool valid) {
    using M = GcwDims<D>;
    float4_t acc[M::TPC];
#pragma unroll
    for (int tl = 0; tl < M::TPC; tl++) {
        const float4 b = *reinterpret_cast<const float4*>(tailp + 16 * (c * M::TPC + tl) + 4 * g);
        acc[tl] = (float4_t){b.x, b.y, b.z, b.w};
    }
#pragma unroll
    for (int ks = 0; ks < M::KS; ks++) {
        ds_uint4_t w[M::TPC][2];
#pragma unroll
        for (int tl = 0; tl < M::TPC; tl++)
#pragma unroll
            for (int p = 0; p < 2; p++) w[tl][p] = *reinterpret_cast<const ds_uint4_t*>(wb + ((tl * M::KS + ks) * 2 + p) * 1024 + lane * 16);
#pragma unroll
        for (int tl = 0; tl < M::TPC; tl++) acc[tl] = DS_MFMA16(w[tl][0], in_hi[ks], acc[tl]);
#pragma unroll
        for (int tl = 0; tl < M::TPC; tl++) acc[tl] = DS_MFMA16(w[tl][0], in_lo[ks], acc[tl]);
#pragma unroll
        for (int tl = 0; tl < M::TPC; tl++) acc[tl] = DS_MFMA16(w[tl][1], in_hi[ks], acc[tl]);
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

// what the VN instance of the layer kernel takes besides the layer's own arguments (GcnVnArgs of gcn_ogbvn.h at this width)
struct GcwVnArgs {
    const int* node_graph;  // [N] the graph of every node (gcw_vn_t0_kernel)
    const float* vn;        // [G][D] vn_{s+1}
    float* part;            // [(G + n_tiles)][D] partial sums of xin_{s+1}, or null: stage 3, which feeds no update
};
struct GcwNoVnArgs {};

// what an EXT instance takes on top (section 4.25); every pointer may be null, and which adds a launch does is decided by them alone.
// The rows are [N][D] and pre-linear: x_s = h_s (+ vn_s[g]), what OGB's h_list holds -- the kernel's own input x is W_s x_s + b_s
struct GcwExtArgs {
    const float* rin;    // residual: the rows x_s, added to relu(pre_s) (the final stage: to pre_4) before the virtual node's vector
    float* rout;         // the rows x_{s+1} this stage leaves for the next one's rin (may be rin); the final stage has none
    const float* jk_in;  // JK sum: the running sum x_0 + .. + x_s ...
    float* jk_out;       // ... and where jk_in + x_{s+1} goes (may be jk_in; jk_in may be rin)
};
struct GcwNoExtArgs {};

// Lane (j, g) holds a[4 q + r], columns 16 q + 4 g + r of node j of 16-node tile `tile`; gi is that node's graph, or -1 for a clamped
// lane behind the batch's last node (it adds nothing and stores nothing).  a += vn[gi]; with `part`, the column sums of the sum over
// the lanes of every graph present in the tile go to the partial row of slot gi + tile: gcn_ogbvn_tile_partials's segmented scan
// (row_shr 1 / 2 / 4 / 8 along the 16 lanes of a row, the graph's last lane stores), run per 16-column piece -- four live values at a
// time, not 4 Q.  Every cross-lane read is made by every lane of the wave, outside any test that differs between lanes (gcn_ogbvn.h
// records the bug).  Pieces at or beyond column D are neither added to nor stored: they stay zero.
template <int D>
__device__ __forceinline__ void gcw_vn_add_partials(float (&a)[4 * GcwDims<D>::Q], const float* __restrict__ vn, int gi, int j, int g,
                                                    long long tile, float* __restrict__ part) {
    using M = GcwDims<D>;
    const size_t gr = (size_t)(gi >= 0 ? gi : 0);
    const float* const vr = vn + gr * D + 4 * g;
    const bool take1 = gcn_ogbvn_row_shr<1>(gi, -2) == gi, take2 = gcn_ogbvn_row_shr<2>(gi, -2) == gi;
    const bool take4 = gcn_ogbvn_row_shr<4>(gi, -2) == gi, take8 = gcn_ogbvn_row_shr<8>(gi, -2) == gi;
    const int next_gi = gcn_ogbvn_row_shl1(gi, -2);
    const bool store = gi >= 0 && (j == 15 || next_gi != gi);
    float* const pr = part ? part + (gr + (size_t)tile) * D + 4 * g : nullptr;  // (formed by every lane, followed by the storing ones alone)
#pragma unroll
    for (int q = 0; q < M::T; q++) {
        const bool in = 16 * q + 16 <= D || 16 * q + 4 * g < D;
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gi >= 0 && in) w = *reinterpret_cast<const float4*>(vr + 16 * q);
        a[4 * q + 0] += w.x; a[4 * q + 1] += w.y; a[4 * q + 2] += w.z; a[4 * q + 3] += w.w;
        if (part) {  // (uniform over the launch)
            float s[4];
#pragma unroll
            for (int r = 0; r < 4; r++) s[r] = gi >= 0 ? a[4 * q + r] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float y = __builtin_bit_cast(float, gcn_ogbvn_row_shr<1>(__builtin_bit_cast(int, s[r]), 0));
                s[r] = take1 ? s[r] + y : s[r];
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float y = __builtin_bit_cast(float, gcn_ogbvn_row_shr<2>(__builtin_bit_cast(int, s[r]), 0));
                s[r] = take2 ? s[r] + y : s[r];
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float y = __builtin_bit_cast(float, gcn_ogbvn_row_shr<4>(__builtin_bit_cast(int, s[r]), 0));
                s[r] = take4 ? s[r] + y : s[r];
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float y = __builtin_bit_cast(float, gcn_ogbvn_row_shr<8>(__builtin_bit_cast(int, s[r]), 0));
                s[r] = take8 ? s[r] + y : s[r];
            }
            if (store && in) *reinterpret_cast<float4*>(pr + 16 * q) = make_float4(s[0], s[1], s[2], s[3]);
        }
    }
}

// EXT, the residual: a += rin[node], piece by piece, under gcw_vn_add_partials's `in` guard (the piece that straddles column D stays
// zero beyond it).  A clamped lane behind the batch's last node adds nothing: the row it would read is being rewritten in place by
// the lane that owns it.  (A fence every four pieces, as in the walk's epilogue: the loads are not hoisted above one another.)
template <int D>
__device__ __forceinline__ void gcw_ext_residual(float (&a)[4 * GcwDims<D>::Q], const float* rin, long long node, bool valid, int g) {
    using M = GcwDims<D>;
    const float* const rr = rin + (size_t)node * D + 4 * g;
#pragma unroll
    for (int q = 0; q < M::T; q++) {
        if (q % 4 == 0) __builtin_amdgcn_sched_barrier(0);
        const bool in = 16 * q + 16 <= D || 16 * q + 4 * g < D;
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid && in) w = *reinterpret_cast<const float4*>(rr + 16 * q);
        a[4 * q + 0] += w.x; a[4 * q + 1] += w.y; a[4 * q + 2] += w.z; a[4 * q + 3] += w.w;
    }
}

// EXT, the stores of the lane's own pieces: jk_out[node] = jk_in[node] + a, then rout[node] = a -- in this order, since jk_in may be
// the rows rout overwrites (stage 0 with both flags on).  A lane reads a piece before it writes it and nobody else touches it.
template <int D>
__device__ __forceinline__ void gcw_ext_store(const float (&a)[4 * GcwDims<D>::Q], float* rout, const float* jk_in, float* jk_out,
                                              long long node, bool valid, int g) {
    using M = GcwDims<D>;
    if (!valid) return;
    const size_t at = (size_t)node * D + 4 * g;
    if (jk_out) {  // (uniform over the launch, as is rout)
#pragma unroll
        for (int q = 0; q < M::T; q++) {
            if (q % 4 == 0) __builtin_amdgcn_sched_barrier(0);
            if (16 * q + 16 <= D || 16 * q + 4 * g < D) {
                const float4 s = *reinterpret_cast<const float4*>(jk_in + at + 16 * q);
                *reinterpret_cast<float4*>(jk_out + at + 16 * q) = make_float4(s.x + a[4 * q + 0], s.y + a[4 * q + 1], s.z + a[4 * q + 2], s.w + a[4 * q + 3]);
            }
        }
    }
    if (rout) {
#pragma unroll
        for (int q = 0; q < M::T; q++)
            if (16 * q + 16 <= D || 16 * q + 4 * g < D)
                *reinterpret_cast<float4*>(rout + at + 16 * q) = make_float4(a[4 * q + 0], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
    }
}

// xout[v] = W relu(pre[v]) + b: stages l = 0..3.  tab: the layer's table; wchunks / tailp: the NEXT layer's product (gcw_pack_layer).
// The body of the layer's two kernels (below); VN is a compile-time constant in each, and without it this compiles to what the one
// kernel was before the other existed.  VN: xout[v] = W (relu(pre[v]) + vn[g(v)]) + b, and the partial rows (gcw_vn_add_partials).
// EXT (gcn_wide_jk.hip): the residual in front of the virtual node's add, so that the partial rows hold it (OGB's order), and the
// stores of x_{s+1} and of the JK sum behind the range tracking, in front of the split.
template <int D, bool VN, bool EXT = false>
__device__ __forceinline__ void gcw_layer_body(const float* __restrict__ x, float* __restrict__ xout,
                                               const int* __restrict__ row_ptr, const int* __restrict__ src,
                                               const uint8_t* __restrict__ ecode, const float* __restrict__ esc,
                                               const int* __restrict__ out_deg, const float* __restrict__ tab,
                                               const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                               int n_tot, int* __restrict__ range_flag,
                                               typename std::conditional<VN, GcwVnArgs, GcwNoVnArgs>::type vna,
                                               typename std::conditional<EXT, GcwExtArgs, GcwNoExtArgs>::type ext = {}) {
    using M = GcwDims<D>;
    // three DISTINCT LDS objects: the DMA into one weight buffer does not alias the reads of the other, and the table stays
    __shared__ __attribute__((aligned(16))) char s_tab[M::TAB_BYTES];
    __shared__ __attribute__((aligned(16))) char s_w0[M::CHUNK_BYTES];  // the even chunks
    __shared__ __attribute__((aligned(16))) char s_w1[M::CHUNK_BYTES];  // the odd chunks
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const long long node0 = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;
    const bool valid = node0 < n_tot;
    const long long node = valid ? node0 : (long long)n_tot - 1;

    gw_issue_pieces<M::TAB_PIECES>(reinterpret_cast<const uint8_t*>(tab), s_tab, M::TAB_PIECES, M::TAB_LAST_LANES, wave, lane);
    gw_issue_pieces<M::PIECES>(wchunks, s_w0, M::PIECES, 64, wave, lane);  // chunk 0
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    float a[4 * M::Q];
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
    for (int k = 0; k < 4 * M::Q; k += 2) vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, __builtin_fabsf(a[k])), __builtin_fabsf(a[k + 1]));
    if constexpr (EXT) gcw_ext_store<D>(a, ext.rout, ext.jk_in, ext.jk_out, node, valid, g);
    ds_uint4_t in_hi[M::KS], in_lo[M::KS];
#pragma unroll
    for (int ks = 0; ks < M::KS; ks++) {
        DS_SPLIT2(a[8 * ks + 0], a[8 * ks + 1], in_hi[ks].x, in_lo[ks].x);
        DS_SPLIT2(a[8 * ks + 2], a[8 * ks + 3], in_hi[ks].y, in_lo[ks].y);
        DS_SPLIT2(a[8 * ks + 4], a[8 * ks + 5], in_hi[ks].z, in_lo[ks].z);
        DS_SPLIT2(a[8 * ks + 6], a[8 * ks + 7], in_hi[ks].w, in_lo[ks].w);
    }
    const float oscale = tailp[M::SCALE_AT];
    float* const row = xout + (size_t)node * D;

    // ---- the product, weights streamed through LDS (chunk 0 has been resident since the first barrier; nobody has touched s_w1)
#pragma unroll 1
    for (int c = 0; c < M::STEPS; c += 2) {
        gw_issue_pieces<M::PIECES>(wchunks + (size_t)(c + 1) * M::CHUNK_BYTES, s_w1, M::PIECES, 64, wave, lane);
        gcw_step<D>(s_w0, c, lane, g, in_hi, in_lo, tailp, oscale, row, valid);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of chunk c + 1 have landed
        __syncthreads();                                  // everyone's have; everyone is done with s_w0
        if (c + 2 < M::STEPS) gw_issue_pieces<M::PIECES>(wchunks + (size_t)(c + 2) * M::CHUNK_BYTES, s_w0, M::PIECES, 64, wave, lane);
        gcw_step<D>(s_w1, c + 1, lane, g, in_hi, in_lo, tailp, oscale, row, valid);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (__any(!(vmax < 6.0e4f))) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

// Stage 4 with the two options: out[v] = h_5[v] = pre_4[v] (+ rin[v]), and with the JK sum jk_out[v] = jk_in[v] + h_5[v]; the walk and
// the epilogue without ReLU and without a product, as in gcw_final_kernel (gcn_wide.hip).  That kernel keeps its own text and is not
// an instance of this: its pointers are kernel arguments, which the compiler knows to be global memory from the first pass on, and
// as arguments of an inlined function they are not -- the address arithmetic comes out in another order, and with it the schedule.
// (gcw_layer_body's two kernels have been instances of a body since they exist.)
template <int D>
__device__ __forceinline__ void gcw_final_jk_body(const float* __restrict__ x, float* __restrict__ out,
                                                  const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                  const uint8_t* __restrict__ ecode, const float* __restrict__ esc,
                                                  const int* __restrict__ out_deg, const float* __restrict__ tab, int n_tot, GcwExtArgs ext) {
    using M = GcwDims<D>;
    __shared__ __attribute__((aligned(16))) char s_tab[M::TAB_BYTES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const long long node0 = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;
    const bool valid = node0 < n_tot;
    const long long node = valid ? node0 : (long long)n_tot - 1;
    gw_issue_pieces<M::TAB_PIECES>(reinterpret_cast<const uint8_t*>(tab), s_tab, M::TAB_PIECES, M::TAB_LAST_LANES, wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    float a[4 * M::Q];
    gcw_walk<D, false>(x, row_ptr, src, ecode, esc, out_deg, reinterpret_cast<const float*>(s_tab), node, valid, g, a);
    if (ext.rin) gcw_ext_residual<D>(a, ext.rin, node, valid, g);  // (uniform over the launch)
    gcw_ext_store<D>(a, nullptr, ext.jk_in, ext.jk_out, node, valid, g);
    if (valid) {
        float* row = out + (size_t)node * D + 4 * g;
#pragma unroll
        for (int q = 0; q < M::Q; q++)
            if (16 * q + 4 * g < D) *reinterpret_cast<float4*>(row + 16 * q) = make_float4(a[4 * q + 0], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
    }
}

}  // namespace
}  // namespace fg
