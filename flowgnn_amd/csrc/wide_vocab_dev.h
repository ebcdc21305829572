// wide_vocab_dev.h -- what the vocabulary head's split-f16 translation units share (wide_vocab.hip: sections 4.33, 4.34;
// wide_vocab_score.hip: section 4.36): the chunk's dimensions, the tie rule, a tile's logits, the running soft-max pair and the parts
// of the head's device form.  Everything has internal linkage and is inlined where it is used; moving it here left wide_vocab.hip's
// device assembly as it was (section 4.36).
#pragma once
#include <climits>

#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"

namespace fg {
namespace {

template <int D>
struct VhDims {
    static_assert(D % 4 == 0, "rows are read as float4 pieces");
    static constexpr int KS = (D + 31) / 32;                   // K-steps (K padded to 32 KS)
    static constexpr int BIAS_OFF = KS * 2 * 1024;             // fragment (ks * 2 + p), p = 0 hi, 1 lo; then 16 floats
    static constexpr int CHUNK_BYTES = BIAS_OFF + 16 * 4;
    static constexpr int PIECES = (CHUNK_BYTES + 1023) / 1024; // DMA pieces of 1 KiB, the last one partial
    static constexpr int LAST_LANES = (CHUNK_BYTES - (PIECES - 1) * 1024) / 16;
    static constexpr int CHUNK_STRIDE = PIECES * 1024;         // in global memory
    static_assert(2 * CHUNK_BYTES <= 64 * 1024, "two chunk buffers, and room for three workgroups on a CU");
};

// (larger value, then lower index): the tie rule, wherever two candidates meet
__device__ __forceinline__ void vh_take(float& m, int& idx, float cm, int cidx) {
    if (cm > m || (cm == m && cidx < idx)) {
        m = cm;
        idx = cidx;
    }
}

// ... and the same rule as the order of the top-k form's lists and of every merge of them (section 4.34): whether a comes before b,
// asked of vh_take so that the rule stays stated once.  (a, b: two different candidates, so different indices unless both are the
// empty entry, which comes before nothing)
__device__ __forceinline__ bool vh_before(float av, int ai, float bv, int bi) {
    vh_take(bv, bi, av, ai);
    return bi == ai && ai != INT_MAX;
}

// The B operands: the pooled row of the lane's graph (clamped to the last one), split once; false: a value at or beyond 6e4 or not
// finite.  The load, the split and the range test as vh_kernel and vh_topk_kernel have them in line (wide_vocab.hip: their code stays
// as it was compiled, section 4.36); whoever changes the split there changes it here, and the other way round -- the target's logit
// has the stream pass's bits only while the two agree
template <int D>
__device__ __forceinline__ bool vh_load_b(const float* __restrict__ pooled, long long graph, int num_graphs, int g,
                                          ds_uint4_t (&b_hi)[VhDims<D>::KS], ds_uint4_t (&b_lo)[VhDims<D>::KS]) {
    const long long gr = graph < num_graphs ? graph : (long long)num_graphs - 1;
    const float* row = pooled + (size_t)gr * D + 4 * g;
    bool ok = true;
#pragma unroll
    for (int ks = 0; ks < VhDims<D>::KS; ks++) {
        float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;  // (columns at or beyond D: the K padding)
        if (32 * ks + 4 * g < D) x0 = *reinterpret_cast<const float4*>(row + 32 * ks);
        if (32 * ks + 16 + 4 * g < D) x1 = *reinterpret_cast<const float4*>(row + 32 * ks + 16);
        // (compares, not a max: a NaN fails them too)
        ok = ok && __builtin_fabsf(x0.x) < 6.0e4f && __builtin_fabsf(x0.y) < 6.0e4f && __builtin_fabsf(x0.z) < 6.0e4f && __builtin_fabsf(x0.w) < 6.0e4f &&
             __builtin_fabsf(x1.x) < 6.0e4f && __builtin_fabsf(x1.y) < 6.0e4f && __builtin_fabsf(x1.z) < 6.0e4f && __builtin_fabsf(x1.w) < 6.0e4f;
        DS_SPLIT2(x0.x, x0.y, b_hi[ks].x, b_lo[ks].x);
        DS_SPLIT2(x0.z, x0.w, b_hi[ks].y, b_lo[ks].y);
        DS_SPLIT2(x1.x, x1.y, b_hi[ks].z, b_lo[ks].z);
        DS_SPLIT2(x1.z, x1.w, b_hi[ks].w, b_lo[ks].w);
        asm volatile("" ::: "memory");  // (set-up code: keep the scheduler from holding every row piece at once)
    }
    return ok;
}

// One chunk from `wb`: the logits of a tile (rows 16 t + 4 g .. + 3 of the lane's graph), in the scaled domain
template <int D>
__device__ __forceinline__ float4_t vh_tile_logits(const char* wb, int lane, int g, const ds_uint4_t (&b_hi)[VhDims<D>::KS],
                                                   const ds_uint4_t (&b_lo)[VhDims<D>::KS]) {
    using M = VhDims<D>;
    const float4 bv = *reinterpret_cast<const float4*>(wb + M::BIAS_OFF + g * 16);
    float4_t acc = (float4_t){bv.x, bv.y, bv.z, bv.w};
    // the fragments one K-step ahead of their MFMAs, and no further: the B operands leave few registers (the compiler barrier keeps the
    // scheduler from hoisting all twenty reads of the chunk to the top)
    ds_uint4_t n_hi = *reinterpret_cast<const ds_uint4_t*>(wb + lane * 16);
    ds_uint4_t n_lo = *reinterpret_cast<const ds_uint4_t*>(wb + 1024 + lane * 16);
#pragma unroll
    for (int ks = 0; ks < M::KS; ks++) {
        const ds_uint4_t a_hi = n_hi, a_lo = n_lo;
        if (ks + 1 < M::KS) {
            n_hi = *reinterpret_cast<const ds_uint4_t*>(wb + (ks * 2 + 2) * 1024 + lane * 16);
            n_lo = *reinterpret_cast<const ds_uint4_t*>(wb + (ks * 2 + 3) * 1024 + lane * 16);
        }
        asm volatile("" ::: "memory");
        acc = DS_MFMA16(a_hi, b_hi[ks], acc);
        acc = DS_MFMA16(a_hi, b_lo[ks], acc);
        acc = DS_MFMA16(a_lo, b_hi[ks], acc);
    }
    return acc;
}

// The soft-max pair (m, s), s = sum 2^(y - m) over real logits y = logit log2(e) (section 4.34): the hardware's exp2, log2(e) folded
// into the inverse scale; lse = (m + log2 s) ln 2
constexpr float VH_LOG2E = 1.44269504088896340736f, VH_LN2 = 0.69314718055994530942f;

// one more y into (m, s)
__device__ __forceinline__ void vh_lse_add(float& m, float& s, float y) {
    if (y > m) {
        s *= __builtin_amdgcn_exp2f(m - y);  // (m = -inf: s is 0 and stays 0)
        m = y;
    }
    s += __builtin_amdgcn_exp2f(y - m);
}

// two pairs into one; a pair that has seen nothing is (-inf, 0)
__device__ __forceinline__ void vh_lse_fold(float& m, float& s, float om, float os) {
    const float nm = __builtin_fmaxf(m, om);
    s = (m == nm ? s : s * __builtin_amdgcn_exp2f(m - nm)) + (om == nm ? os : os * __builtin_amdgcn_exp2f(om - nm));
    m = nm;
}

__device__ __forceinline__ float vh_lse_value(float m, float s) { return (m + __builtin_amdgcn_logf(s)) * VH_LN2; }

constexpr int VH_D = FLOWGNN_EMB_DIM_OGB;  // the launchers' one width: the public constant's

// the parts of the head's device form (wide_vocab.h)
struct VhBlob {
    size_t inv_off, wt_off, b_off, bytes;
    int vtiles, v4;
    VhBlob(int positions, int vocab) {
        vtiles = (vocab + 15) / 16;
        v4 = (vocab + 3) / 4 * 4;
        inv_off = (size_t)positions * vtiles * VhDims<VH_D>::CHUNK_STRIDE;
        wt_off = inv_off + 16;
        b_off = wt_off + (size_t)positions * VH_D * v4 * 4;
        bytes = b_off + (size_t)positions * v4 * 4;
    }
};

inline bool vh_args(int emb_dim, int positions, int vocab) {
    return emb_dim == VH_D && positions >= 1 && positions <= FLOWGNN_MAX_VOCAB_POSITIONS && vocab >= 1 && vocab <= FLOWGNN_MAX_VOCAB;
}

}  // namespace
}  // namespace fg
