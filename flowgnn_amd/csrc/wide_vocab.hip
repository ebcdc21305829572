// ogbg-code2 on the 300-wide GIN: the vocabulary head with a fused argmax, and the AST node encoder.
//
// The head (flowgnn_set_vocab_head): code2 predicts a sequence of P = 5 tokens, each the argmax of Linear(300, 5002) on the pooled
// row.  vh_kernel computes the P x V logits of a tile of graphs on the f16 matrix pipe, fp32-accurate by the project's split scheme
// (w_hi x_hi + w_hi x_lo + w_lo x_hi, fp32 accumulate, weights times one power of two), and keeps only a running (max, index): the
// logits never reach memory.
//   * Transposed layout: a 16-row tile of W[p] is the A operand, 16 graphs are the B operand, so lane (j = lane & 15, g = lane >> 4)
//     of tile t holds the logits of vocabulary entries 16 t + 4 g .. + 3 of graph j.
//   * B: the pooled rows of the wave's graphs, split once into hi and lo halves and held in registers for the whole launch (10
//     K-steps, K padded to 320 with zeros: 80 registers).  A wave owns one tile of 16 graphs (section 4.33 says why not two).
//   * A: tile (p, t) is one chunk of the weight stream, 10 K-steps x {hi, lo} x 1 KiB in gw_pack_tile's layout and the tile's 16
//     pre-scaled biases, which are the accumulator's initial value.  Chunks go L2 -> LDS by LDS-DMA (gw_issue_pieces), double
//     buffered in two distinct LDS objects and shared by the workgroup's eight waves; one s_waitcnt vmcnt(0) + barrier per chunk.
//   * The running maximum: per lane and accumulator row one (max, tile) pair, updated with a strict > as t ascends, so the lowest
//     tile keeps a tie; rows at or beyond V are never compared.  At the end of a position the four pairs of the lane, then the four
//     lane groups of a graph (two xor shuffles), are folded by (larger value, then lower index).
//   * Grid: x = tiles of 128 graphs, y = slices of the vocabulary's 16-row tiles.  With more than one slice each block leaves a
//     partial (max, index) per (slice, graph, position) and vh_fold_kernel folds them, slices ascending, under the same rule.
// A pooled value at or beyond 6e4 or not finite raises *range_flag; the engine then repeats the pass with the exact form,
// vh_f32_kernel: a plain fma chain from the bias, k ascending, the same tie rule.
// flowgnn_set_vocab_topk (section 4.34) swaps the three for their top-k forms, vh_topk_*: described where they stand, below.
//
// The encoder (flowgnn_set_ast_encoder): OGB's ASTNodeEncoder, three table rows summed per node in the order type, attribute, depth
// (clamped to max_depth in the kernel), then the virtual node's E: gw_atom_encoder_body's scheme with the tables' sizes as arguments.
#include <climits>
#include <cmath>
#include <cstring>

#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "wide_common.h"  // GW_WAVES, gw_issue_pieces, gw_pack_tile, gw_pow2_scale
#include "wide_vocab.h"
#include "wide_vocab_dev.h"  // VhDims, vh_take, vh_tile_logits, vh_lse_*, VhBlob: shared with wide_vocab_score.hip

namespace fg {
namespace {

constexpr int VH_MIN_SLICE_TILES = 4;  // a slice is at least this many 16-row tiles per position: the B operands are set up once per block

// ... and the update of the running pairs
template <int D>
__device__ __forceinline__ void vh_tile(const char* wb, int t, int lane, int g, int vocab, const ds_uint4_t (&b_hi)[VhDims<D>::KS],
                                        const ds_uint4_t (&b_lo)[VhDims<D>::KS], float (&best)[4], int (&bt)[4]) {
    const float4_t acc = vh_tile_logits<D>(wb, lane, g, b_hi, b_lo);
    const int r0 = 16 * t + 4 * g;
    const float v[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int r = 0; r < 4; r++)
        if (r0 + r < vocab && v[r] > best[r]) {  // (strict: an equal logit of a later tile does not replace an earlier one)
            best[r] = v[r];
            bt[r] = t;
        }
}

// out_val / out_idx [slice][G][P]: the slice's partial pairs in the scaled domain; or, with `final` (one slice), scores and tokens
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void vh_kernel(const float* __restrict__ pooled, const uint8_t* __restrict__ chunks,
                                                           const float* __restrict__ inv_p, int num_graphs, int positions, int vocab,
                                                           int vtiles, int slice_tiles, int final, float* __restrict__ out_val,
                                                           int* __restrict__ out_idx, int* __restrict__ range_flag) {
    using M = VhDims<D>;
    // two DISTINCT LDS objects, as in gw_layer_body: the DMA into one does not alias the reads of the other
    __shared__ __attribute__((aligned(16))) char s_a[M::CHUNK_BYTES];
    __shared__ __attribute__((aligned(16))) char s_b[M::CHUNK_BYTES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int t0 = blockIdx.y * slice_tiles;
    const int nt = (vtiles - t0 < slice_tiles ? vtiles - t0 : slice_tiles);  // (the host cuts no empty slice)
    const int n = positions * nt;                                            // chunks of this block: (p, t) with t fastest
    auto chunk = [&](int i) {
        const int p = i / nt;
        return chunks + ((size_t)p * vtiles + t0 + (i - p * nt)) * M::CHUNK_STRIDE;
    };
    gw_issue_pieces<M::PIECES>(chunk(0), s_a, M::PIECES, M::LAST_LANES, wave, lane);

    // ---- the B operands: the pooled rows of this wave's 16 graphs, split once (wide_vocab_dev.h's vh_load_b is this block as a
    // function, for wide_vocab_score.hip; the two stay the same split, or a target's logit loses the stream's bits)
    ds_uint4_t b_hi[M::KS], b_lo[M::KS];
    const long long graph = ((long long)blockIdx.x * GW_WAVES + wave) * 16 + j;
    float vmax = 0.0f;
    {
        const long long gr = graph < num_graphs ? graph : (long long)num_graphs - 1;
        const float* row = pooled + (size_t)gr * D + 4 * g;
#pragma unroll
        for (int ks = 0; ks < M::KS; ks++) {
            float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;  // (columns at or beyond D: the K padding)
            if (32 * ks + 4 * g < D) x0 = *reinterpret_cast<const float4*>(row + 32 * ks);
            if (32 * ks + 16 + 4 * g < D) x1 = *reinterpret_cast<const float4*>(row + 32 * ks + 16);
            // (a compare, not a max: a NaN fails it too)
            vmax = (__builtin_fabsf(x0.x) < 6.0e4f && __builtin_fabsf(x0.y) < 6.0e4f && __builtin_fabsf(x0.z) < 6.0e4f && __builtin_fabsf(x0.w) < 6.0e4f &&
                    __builtin_fabsf(x1.x) < 6.0e4f && __builtin_fabsf(x1.y) < 6.0e4f && __builtin_fabsf(x1.z) < 6.0e4f && __builtin_fabsf(x1.w) < 6.0e4f)
                       ? vmax
                       : __builtin_inff();
            DS_SPLIT2(x0.x, x0.y, b_hi[ks].x, b_lo[ks].x);
            DS_SPLIT2(x0.z, x0.w, b_hi[ks].y, b_lo[ks].y);
            DS_SPLIT2(x1.x, x1.y, b_hi[ks].z, b_lo[ks].z);
            DS_SPLIT2(x1.z, x1.w, b_hi[ks].w, b_lo[ks].w);
            asm volatile("" ::: "memory");  // (set-up code: keep the scheduler from holding every row piece at once)
        }
    }
    float best[4];
    int bt[4];  // the tile of `best`; INT_MAX: none yet
#pragma unroll
    for (int r = 0; r < 4; r++) {
        best[r] = -__builtin_inff();
        bt[r] = INT_MAX;
    }
    const float inv = *inv_p;

    // the end of a position: fold the lane's four pairs, then the graph's four lane groups; lane group 0 stores
    auto finish = [&](int p) {
        float m = -__builtin_inff();
        int idx = INT_MAX;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            vh_take(m, idx, best[r], bt[r] == INT_MAX ? INT_MAX : 16 * bt[r] + 4 * g + r);
            best[r] = -__builtin_inff();
            bt[r] = INT_MAX;
        }
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
            const float om = __shfl_xor(m, off);
            const int oi = __shfl_xor(idx, off);
            vh_take(m, idx, om, oi);
        }
        if (g == 0 && graph < num_graphs) {
            const size_t o = ((size_t)blockIdx.y * num_graphs + (size_t)graph) * positions + p;
            out_val[o] = final ? m * inv : m;
            // INT_MAX survives only where no logit of the graph compared greater than -inf, that is where every one is NaN or -inf;
            // finite weights give that only from a non-finite pooled row, which also raises *range_flag, so the 0 written here (and by
            // vh_fold_kernel) is on a pass that the engine repeats with vh_f32_kernel and is never what a caller reads
            out_idx[o] = final && idx == INT_MAX ? 0 : idx;
        }
    };

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < n; i += 2) {
        if (i + 1 < n) gw_issue_pieces<M::PIECES>(chunk(i + 1), s_b, M::PIECES, M::LAST_LANES, wave, lane);
        {
            const int p = i / nt, tl = i - p * nt;
            vh_tile<D>(s_a, t0 + tl, lane, g, vocab, b_hi, b_lo, best, bt);
            if (tl == nt - 1) finish(p);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of chunk i + 1 have landed
        __syncthreads();                                  // everyone's have; everyone is done with s_a
        if (i + 1 < n) {                                  // (uniform over the workgroup)
            if (i + 2 < n) gw_issue_pieces<M::PIECES>(chunk(i + 2), s_a, M::PIECES, M::LAST_LANES, wave, lane);
            const int p = (i + 1) / nt, tl = i + 1 - p * nt;
            vh_tile<D>(s_b, t0 + tl, lane, g, vocab, b_hi, b_lo, best, bt);
            if (tl == nt - 1) finish(p);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
    if (__any(!(vmax < 6.0e4f))) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

// tokens / scores [G][P] out of the slices' partial pairs [S][G][P]: slices ascending, so are their indices
__global__ __launch_bounds__(256) void vh_fold_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                                                      const float* __restrict__ inv_p, int slices, long long items, int* __restrict__ tokens,
                                                      float* __restrict__ scores) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    float m = -__builtin_inff();
    int idx = INT_MAX;
    for (int s = 0; s < slices; s++) vh_take(m, idx, part_val[(size_t)s * items + i], part_idx[(size_t)s * items + i]);
    tokens[i] = idx == INT_MAX ? 0 : idx;
    scores[i] = m * *inv_p;
}

// The exact form: logit = fma chain from the bias, k ascending; eight graphs per workgroup staged in LDS, a thread owns vocabulary
// entries tid, tid + 256, .. (ascending: a strict > keeps the lowest), then a tree over the 256 threads under the tie rule
template <int D>
__global__ __launch_bounds__(256) void vh_f32_kernel(const float* __restrict__ pooled, const float* __restrict__ wt, const float* __restrict__ b,
                                                     int num_graphs, int positions, int vocab, int v4, int* __restrict__ tokens,
                                                     float* __restrict__ scores) {
    constexpr int RB = 8;
    __shared__ float s_in[RB][D];
    __shared__ float s_m[RB][256];
    __shared__ int s_i[RB][256];
    const long long g0 = (long long)blockIdx.x * RB;
    const int p = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < RB * D; i += 256) {
        const int r = i / D, k = i - r * D;
        s_in[r][k] = g0 + r < num_graphs ? pooled[(size_t)(g0 + r) * D + k] : 0.0f;
    }
    __syncthreads();
    float best[RB];
    int bi[RB];
#pragma unroll
    for (int r = 0; r < RB; r++) {
        best[r] = -__builtin_inff();
        bi[r] = INT_MAX;
    }
    const float* wp = wt + (size_t)p * D * v4;
    for (int v = tid; v < vocab; v += 256) {
        float acc[RB];
        const float bv = b[(size_t)p * v4 + v];
#pragma unroll
        for (int r = 0; r < RB; r++) acc[r] = bv;
        for (int k = 0; k < D; k++) {
            const float w = wp[(size_t)k * v4 + v];
#pragma unroll
            for (int r = 0; r < RB; r++) acc[r] = __builtin_fmaf(s_in[r][k], w, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < RB; r++)
            if (acc[r] > best[r]) {
                best[r] = acc[r];
                bi[r] = v;
            }
    }
#pragma unroll
    for (int r = 0; r < RB; r++) {
        s_m[r][tid] = best[r];
        s_i[r][tid] = bi[r];
    }
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off)
#pragma unroll
            for (int r = 0; r < RB; r++) vh_take(s_m[r][tid], s_i[r][tid], s_m[r][tid + off], s_i[r][tid + off]);
        __syncthreads();
    }
    if (tid < RB && g0 + tid < num_graphs) {
        const size_t o = (size_t)(g0 + tid) * positions + p;
        tokens[o] = s_i[tid][0] == INT_MAX ? 0 : s_i[tid][0];
        scores[o] = s_m[tid][0];
    }
}

// ---------------------------------------------------------------- the top-k form (flowgnn_set_vocab_topk)
// The same three kernels with the running (max, index) replaced by a sorted list of K (value, index) pairs and a running soft-max
// pair; rank 0 is the argmax form's pair bit for bit (the same chunk stream, split and MFMA order: vh_tile_logits).
//   * The lists live in LDS, [slot][thread]: a wave's 64 lanes hit 64 distinct banks, and no list costs a register.  A lane of
//     vh_topk_kernel has ONE list for its four accumulator rows and keeps only `thr`, the value of its K-th entry (-inf until the
//     list is full), in a register.  Its candidates arrive in ascending index order (tiles ascend, rows within a tile ascend), so the
//     test is the strict v > thr -- an equal later candidate loses, as the order wants -- and a candidate that passes takes the
//     divergent path: vh_list_insert.
//   * The soft-max pair (m, s), s = sum 2^(y - m) over the lane's real logits y = logit log2(e): the hardware's exp2, log2(e) folded
//     into the inverse scale; lse = (m + log2 s) ln 2.
//   * The end of a position: the graph's four lane groups hold four sorted lists; lane group 0 merges them in K steps (LDS operations
//     of a wave issue in order: a wave barrier, no workgroup barrier), the (m, s) pairs fold by two xor shuffles, everything is reset.
//   * Slices: partial lists [S][G][P][K] and partial (m, s) [S][G][P] in the scaled / log2 domain; vh_topk_fold_kernel merges them.
constexpr int VH_TOPK_MAX = FLOWGNN_MAX_VOCAB_TOPK;

// The list at lv / li, slot q at [q * stride], sorted under vh_before; (v, idx) comes before its last entry, which leaves
__device__ __forceinline__ void vh_list_insert(float* lv, int* li, int stride, int K, float v, int idx) {
    int q = K - 1;
    while (q > 0 && vh_before(v, idx, lv[(q - 1) * stride], li[(q - 1) * stride])) {
        lv[q * stride] = lv[(q - 1) * stride];
        li[q * stride] = li[(q - 1) * stride];
        q--;
    }
    lv[q * stride] = v;
    li[q * stride] = idx;
}

__device__ __forceinline__ void vh_list_clear(float* lv, int* li, int stride, int K) {
    for (int q = 0; q < K; q++) {
        lv[q * stride] = -__builtin_inff();
        li[q * stride] = INT_MAX;  // the empty entry: after every real one
    }
}

// out_val / out_idx [slice][G][P][K], out_m / out_s [slice][G][P]: the slice's partial lists and pair; or, with `final` (one slice),
// the top-k scores and tokens, lse in out_m, and rank 0 in tokens / scores
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void vh_topk_kernel(const float* __restrict__ pooled, const uint8_t* __restrict__ chunks,
                                                                const float* __restrict__ inv_p, int num_graphs, int positions, int vocab,
                                                                int vtiles, int slice_tiles, int final, int K, float* __restrict__ out_val,
                                                                int* __restrict__ out_idx, float* __restrict__ out_m, float* __restrict__ out_s,
                                                                int* __restrict__ tokens, float* __restrict__ scores, int* __restrict__ range_flag) {
    using M = VhDims<D>;
    constexpr int NT = GW_WAVES * 64;
    __shared__ __attribute__((aligned(16))) char s_a[M::CHUNK_BYTES];
    __shared__ __attribute__((aligned(16))) char s_b[M::CHUNK_BYTES];
    __shared__ float s_lv[VH_TOPK_MAX * NT];  // 2 x 16 KiB beside the 41 KiB of chunks: two workgroups on a CU still fit
    __shared__ int s_li[VH_TOPK_MAX * NT];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int t0 = blockIdx.y * slice_tiles;
    const int nt = (vtiles - t0 < slice_tiles ? vtiles - t0 : slice_tiles);
    const int n = positions * nt;
    auto chunk = [&](int i) {
        const int p = i / nt;
        return chunks + ((size_t)p * vtiles + t0 + (i - p * nt)) * M::CHUNK_STRIDE;
    };
    gw_issue_pieces<M::PIECES>(chunk(0), s_a, M::PIECES, M::LAST_LANES, wave, lane);

    // ---- the B operands, as in vh_kernel
    ds_uint4_t b_hi[M::KS], b_lo[M::KS];
    const long long graph = ((long long)blockIdx.x * GW_WAVES + wave) * 16 + j;
    float vmax = 0.0f;
    {
        const long long gr = graph < num_graphs ? graph : (long long)num_graphs - 1;
        const float* row = pooled + (size_t)gr * D + 4 * g;
#pragma unroll
        for (int ks = 0; ks < M::KS; ks++) {
            float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;
            if (32 * ks + 4 * g < D) x0 = *reinterpret_cast<const float4*>(row + 32 * ks);
            if (32 * ks + 16 + 4 * g < D) x1 = *reinterpret_cast<const float4*>(row + 32 * ks + 16);
            vmax = (__builtin_fabsf(x0.x) < 6.0e4f && __builtin_fabsf(x0.y) < 6.0e4f && __builtin_fabsf(x0.z) < 6.0e4f && __builtin_fabsf(x0.w) < 6.0e4f &&
                    __builtin_fabsf(x1.x) < 6.0e4f && __builtin_fabsf(x1.y) < 6.0e4f && __builtin_fabsf(x1.z) < 6.0e4f && __builtin_fabsf(x1.w) < 6.0e4f)
                       ? vmax
                       : __builtin_inff();
            DS_SPLIT2(x0.x, x0.y, b_hi[ks].x, b_lo[ks].x);
            DS_SPLIT2(x0.z, x0.w, b_hi[ks].y, b_lo[ks].y);
            DS_SPLIT2(x1.x, x1.y, b_hi[ks].z, b_lo[ks].z);
            DS_SPLIT2(x1.z, x1.w, b_hi[ks].w, b_lo[ks].w);
            asm volatile("" ::: "memory");
        }
    }
    float* const lv = s_lv + threadIdx.x;  // this lane's list: slot q at [q * NT]
    int* const li = s_li + threadIdx.x;
    vh_list_clear(lv, li, NT, K);
    float thr = -__builtin_inff(), m = -__builtin_inff(), sum = 0.0f;
    const float inv = *inv_p;
    const float c2 = inv * VH_LOG2E;  // scaled logit -> y

    auto tile = [&](const char* wb, int t) {
        const float4_t acc = vh_tile_logits<D>(wb, lane, g, b_hi, b_lo);
        const int r0 = 16 * t + 4 * g;
        const float v[4] = {acc.x, acc.y, acc.z, acc.w};
        // the tile's four y into (m, s) with one rescale; rows at or beyond V are neither summed nor candidates
        float tm = -__builtin_inff();
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (r0 + r < vocab) tm = __builtin_fmaxf(tm, v[r] * c2);
        if (tm > m) {
            sum *= __builtin_amdgcn_exp2f(m - tm);  // (m = -inf: sum is 0 and stays 0)
            m = tm;
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (r0 + r < vocab) sum += __builtin_amdgcn_exp2f(v[r] * c2 - m);
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (r0 + r < vocab && v[r] > thr) {
                vh_list_insert(lv, li, NT, K, v[r], r0 + r);
                thr = lv[(K - 1) * NT];
            }
    };

    auto finish = [&](int p) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
            const float om = __shfl_xor(m, off);
            const float os = __shfl_xor(sum, off);
            vh_lse_fold(m, sum, om, os);
        }
        if (g == 0) {  // the lists of lanes lane + 16 c, c = 0 .. 3: their heads, and how far each has been read
            const bool st = graph < num_graphs;
            const size_t o = ((size_t)blockIdx.y * num_graphs + (size_t)(st ? graph : 0)) * positions + p;
            float hv[4];
            int hi[4], hq[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                hq[c] = 0;
                hv[c] = lv[16 * c];
                hi[c] = li[16 * c];
            }
            for (int k = 0; k < K; k++) {
                float bv = hv[0];
                int bi = hi[0];
#pragma unroll
                for (int c = 1; c < 4; c++) vh_take(bv, bi, hv[c], hi[c]);
                if (st) {
                    out_val[o * K + k] = final ? bv * inv : bv;
                    out_idx[o * K + k] = final && bi == INT_MAX ? -1 : bi;
                    if (final && k == 0) {  // (0 for INT_MAX: on a pass that the engine repeats, as in vh_kernel)
                        scores[o] = bv * inv;
                        tokens[o] = bi == INT_MAX ? 0 : bi;
                    }
                }
                bool moved = false;  // the list that gave (bv, bi) moves on; indices are distinct but for the empty entry
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if (!moved && hi[c] == bi) {
                        moved = true;
                        hq[c]++;
                        const int q = hq[c] < K ? hq[c] : K - 1;
                        const float nv = lv[q * NT + 16 * c];
                        const int ni = li[q * NT + 16 * c];
                        hv[c] = hq[c] < K ? nv : -__builtin_inff();
                        hi[c] = hq[c] < K ? ni : INT_MAX;
                    }
            }
            if (st) {
                out_m[o] = final ? vh_lse_value(m, sum) : m;
                if (!final) out_s[o] = sum;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        vh_list_clear(lv, li, NT, K);
        thr = m = -__builtin_inff();
        sum = 0.0f;
    };

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < n; i += 2) {
        if (i + 1 < n) gw_issue_pieces<M::PIECES>(chunk(i + 1), s_b, M::PIECES, M::LAST_LANES, wave, lane);
        {
            const int p = i / nt, tl = i - p * nt;
            tile(s_a, t0 + tl);
            if (tl == nt - 1) finish(p);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (i + 1 < n) {
            if (i + 2 < n) gw_issue_pieces<M::PIECES>(chunk(i + 2), s_a, M::PIECES, M::LAST_LANES, wave, lane);
            const int p = (i + 1) / nt, tl = i + 1 - p * nt;
            tile(s_b, t0 + tl);
            if (tl == nt - 1) finish(p);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
    if (__any(!(vmax < 6.0e4f))) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

// The slices' partial lists and pairs into the results: one thread per (graph, position), its list in LDS, slices ascending; a
// slice's entries are sorted, so the first that does not come before the list's last entry ends that slice
__global__ __launch_bounds__(256) void vh_topk_fold_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                                                           const float* __restrict__ part_m, const float* __restrict__ part_s,
                                                           const float* __restrict__ inv_p, int slices, long long items, int K, int* __restrict__ tokens,
                                                           float* __restrict__ scores, int* __restrict__ top_tokens, float* __restrict__ top_scores,
                                                           float* __restrict__ lse) {
    __shared__ float s_lv[VH_TOPK_MAX * 256];
    __shared__ int s_li[VH_TOPK_MAX * 256];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    float* const lv = s_lv + threadIdx.x;
    int* const li = s_li + threadIdx.x;
    vh_list_clear(lv, li, 256, K);
    float m = -__builtin_inff(), sum = 0.0f;
    for (int s = 0; s < slices; s++) {
        const size_t o = (size_t)s * items + i;
        for (int k = 0; k < K; k++) {
            const float v = part_val[o * K + k];
            const int idx = part_idx[o * K + k];
            if (!vh_before(v, idx, lv[(K - 1) * 256], li[(K - 1) * 256])) break;
            vh_list_insert(lv, li, 256, K, v, idx);
        }
        vh_lse_fold(m, sum, part_m[o], part_s[o]);
    }
    const float inv = *inv_p;
    for (int k = 0; k < K; k++) {
        top_scores[i * K + k] = lv[k * 256] * inv;
        top_tokens[i * K + k] = li[k * 256] == INT_MAX ? -1 : li[k * 256];
    }
    tokens[i] = li[0] == INT_MAX ? 0 : li[0];
    scores[i] = lv[0] * inv;
    lse[i] = vh_lse_value(m, sum);
}

// The exact form: vh_f32_kernel's fma chain, four graphs per workgroup, a list per (graph, thread) in LDS fed in ascending index
// order as above; then K rounds of vh_f32_kernel's tree over the threads' list heads, the winner's thread moving on
template <int D>
__global__ __launch_bounds__(256) void vh_topk_f32_kernel(const float* __restrict__ pooled, const float* __restrict__ wt, const float* __restrict__ b,
                                                          int num_graphs, int positions, int vocab, int v4, int K, int* __restrict__ tokens,
                                                          float* __restrict__ scores, int* __restrict__ top_tokens, float* __restrict__ top_scores,
                                                          float* __restrict__ lse) {
    constexpr int RB = 4;
    __shared__ float s_in[RB][D];
    __shared__ float s_m[RB][256];
    __shared__ int s_i[RB][256];
    __shared__ float s_lv[RB][VH_TOPK_MAX * 256];
    __shared__ int s_li[RB][VH_TOPK_MAX * 256];
    __shared__ float s_pm[RB][4], s_ps[RB][4];  // the four waves' soft-max pairs
    const long long g0 = (long long)blockIdx.x * RB;
    const int p = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < RB * D; i += 256) {
        const int r = i / D, k = i - r * D;
        s_in[r][k] = g0 + r < num_graphs ? pooled[(size_t)(g0 + r) * D + k] : 0.0f;
    }
    float thr[RB], m[RB], sum[RB];
#pragma unroll
    for (int r = 0; r < RB; r++) {
        vh_list_clear(s_lv[r] + tid, s_li[r] + tid, 256, K);
        thr[r] = m[r] = -__builtin_inff();
        sum[r] = 0.0f;
    }
    __syncthreads();
    const float* wp = wt + (size_t)p * D * v4;
    for (int v = tid; v < vocab; v += 256) {
        float acc[RB];
        const float bv = b[(size_t)p * v4 + v];
#pragma unroll
        for (int r = 0; r < RB; r++) acc[r] = bv;
        for (int k = 0; k < D; k++) {
            const float w = wp[(size_t)k * v4 + v];
#pragma unroll
            for (int r = 0; r < RB; r++) acc[r] = __builtin_fmaf(s_in[r][k], w, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < RB; r++) {
            vh_lse_add(m[r], sum[r], acc[r] * VH_LOG2E);
            if (acc[r] > thr[r]) {
                vh_list_insert(s_lv[r] + tid, s_li[r] + tid, 256, K, acc[r], v);
                thr[r] = s_lv[r][(K - 1) * 256 + tid];
            }
        }
    }
    int hq[RB];
#pragma unroll
    for (int r = 0; r < RB; r++) hq[r] = 0;
    for (int k = 0; k < K; k++) {
        int mine[RB];
#pragma unroll
        for (int r = 0; r < RB; r++) {
            const int q = hq[r] < K ? hq[r] : K - 1;
            s_m[r][tid] = hq[r] < K ? s_lv[r][q * 256 + tid] : -__builtin_inff();
            s_i[r][tid] = mine[r] = hq[r] < K ? s_li[r][q * 256 + tid] : INT_MAX;
        }
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (tid < off)
#pragma unroll
                for (int r = 0; r < RB; r++) vh_take(s_m[r][tid], s_i[r][tid], s_m[r][tid + off], s_i[r][tid + off]);
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < RB; r++)
            if (mine[r] == s_i[r][0] && mine[r] != INT_MAX) hq[r]++;
        if (tid < RB && g0 + tid < num_graphs) {
            const size_t o = (size_t)(g0 + tid) * positions + p;
            top_tokens[o * K + k] = s_i[tid][0] == INT_MAX ? -1 : s_i[tid][0];
            top_scores[o * K + k] = s_m[tid][0];
            if (k == 0) {
                tokens[o] = s_i[tid][0] == INT_MAX ? 0 : s_i[tid][0];
                scores[o] = s_m[tid][0];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < RB; r++) {
        for (int off = 1; off < 64; off <<= 1) {
            const float om = __shfl_xor(m[r], off);
            const float os = __shfl_xor(sum[r], off);
            vh_lse_fold(m[r], sum[r], om, os);
        }
        if ((tid & 63) == 0) {
            s_pm[r][tid >> 6] = m[r];
            s_ps[r][tid >> 6] = sum[r];
        }
    }
    __syncthreads();
    if (tid < RB && g0 + tid < num_graphs) {
        float fm = s_pm[tid][0], fs = s_ps[tid][0];
        for (int w = 1; w < 4; w++) vh_lse_fold(fm, fs, s_pm[tid][w], s_ps[tid][w]);
        lse[(size_t)(g0 + tid) * positions + p] = vh_lse_value(fm, fs);
    }
}

// ---------------------------------------------------------------- the AST node encoder: one lane per (node, float4 piece), the tables
// read through the caches; VN: the virtual node's E added last, the bits of a separate add (gw_atom_encoder_body)
template <int D, bool VN>
__global__ __launch_bounds__(256) void ast_encoder_kernel(const int* __restrict__ x, const int* __restrict__ depth, const float* __restrict__ type_tab,
                                                          const float* __restrict__ attr_tab, const float* __restrict__ depth_tab, int n_types,
                                                          int n_attrs, int max_depth, float* __restrict__ h, int n_tot, int* __restrict__ err,
                                                          const float* __restrict__ vn_e) {
    constexpr int C = D / 4;
    const long long items = (long long)n_tot * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const long long v = i / C;
        const int c = (int)(i - v * C);
        int ty = x[2 * v], at = x[2 * v + 1], dp = depth[v];
        if (ty < 0 || ty >= n_types || at < 0 || at >= n_attrs || dp < 0) {
            atomicMax(err, ERR_NODE_FEAT);
            ty = ty < 0 || ty >= n_types ? 0 : ty;
            at = at < 0 || at >= n_attrs ? 0 : at;
            dp = dp < 0 ? 0 : dp;
        }
        dp = dp > max_depth ? max_depth : dp;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 w0 = reinterpret_cast<const float4*>(type_tab)[(size_t)ty * C + c];
        s.x += w0.x; s.y += w0.y; s.z += w0.z; s.w += w0.w;
        const float4 w1 = reinterpret_cast<const float4*>(attr_tab)[(size_t)at * C + c];
        s.x += w1.x; s.y += w1.y; s.z += w1.z; s.w += w1.w;
        const float4 w2 = reinterpret_cast<const float4*>(depth_tab)[(size_t)dp * C + c];
        s.x += w2.x; s.y += w2.y; s.z += w2.z; s.w += w2.w;
        if (VN) {
            const float4 w = reinterpret_cast<const float4*>(vn_e)[c];
            s.x += w.x; s.y += w.y; s.z += w.z; s.w += w.w;
        }
        reinterpret_cast<float4*>(h)[i] = s;
    }
}

}  // namespace

size_t vocab_head_blob_bytes(int emb_dim, int positions, int vocab) { return vh_args(emb_dim, positions, vocab) ? VhBlob(positions, vocab).bytes : 0; }

void vocab_head_blob_pack(int emb_dim, int positions, int vocab, const float* w, const float* b, void* out) {
    if (!vh_args(emb_dim, positions, vocab)) return;
    constexpr int D = VH_D;
    using M = VhDims<D>;
    const VhBlob L(positions, vocab);
    uint8_t* const o = static_cast<uint8_t*>(out);
    std::memset(o, 0, L.bytes);
    const float scale = gw_pow2_scale(w, (size_t)positions * vocab * D);  // one scale: its inverse is one exact multiply at the end
    for (int p = 0; p < positions; p++) {
        const float* wp = w + (size_t)p * vocab * D;
        const float* bp = b + (size_t)p * vocab;
        for (int t = 0; t < L.vtiles; t++) {
            uint8_t* ck = o + ((size_t)p * L.vtiles + t) * M::CHUNK_STRIDE;
            gw_pack_tile(wp, vocab, D, 16 * t, scale, 0, M::KS, ck, 2048);
            for (int x = 0; x < 16; x++) {
                const float bb = 16 * t + x < vocab ? bp[16 * t + x] * scale : 0.0f;
                std::memcpy(ck + M::BIAS_OFF + x * 4, &bb, 4);
            }
        }
        float* wt = reinterpret_cast<float*>(o + L.wt_off) + (size_t)p * D * L.v4;  // [D][V4]: the exact form reads a weight row per k
        for (int v = 0; v < vocab; v++)
            for (int k = 0; k < D; k++) wt[(size_t)k * L.v4 + v] = wp[(size_t)v * D + k];
        std::memcpy(o + L.b_off + (size_t)p * L.v4 * 4, bp, (size_t)vocab * 4);
    }
    const float inv = 1.0f / scale;
    std::memcpy(o + L.inv_off, &inv, 4);
}

VocabHeadPlan vocab_head_plan(int num_graphs, int vocab, int cus) {
    VocabHeadPlan pl;
    pl.graph_blocks = (int)ceil_div_ll(num_graphs, GW_WAVES * 16);
    // slices: enough blocks for two per compute unit, no slice under VH_MIN_SLICE_TILES tiles, none empty
    const int vtiles = (vocab + 15) / 16;
    long long want = ceil_div_ll(2LL * (cus > 0 ? cus : 1), pl.graph_blocks > 0 ? pl.graph_blocks : 1);
    const long long most = ceil_div_ll(vtiles, VH_MIN_SLICE_TILES);
    if (want > most) want = most;
    if (want < 1) want = 1;
    const int slice_tiles = (int)ceil_div_ll(vtiles, want);
    pl.slices = (int)ceil_div_ll(vtiles, slice_tiles);
    return pl;
}

size_t vocab_head_part_words(const VocabHeadPlan& plan, int num_graphs, int positions, int k) {
    return plan.slices > 1 ? (2 * (size_t)k + 2) * (size_t)plan.slices * (size_t)num_graphs * (size_t)positions : 0;
}

int launch_vocab_head(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, const VocabHeadPlan& plan,
                      void* part, int* tokens, float* scores, int* range_flag, hipStream_t s) {
    if (!vh_args(emb_dim, positions, vocab)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || plan.slices < 1 || (plan.slices > 1 && !part)) return FLOWGNN_ERR_ARG;
    if (num_graphs <= 0) return 0;
    constexpr int D = VH_D;
    const VhBlob L(positions, vocab);
    const uint8_t* const o = static_cast<const uint8_t*>(blob);
    const float* const inv = reinterpret_cast<const float*>(o + L.inv_off);
    const int slice_tiles = (int)ceil_div_ll(L.vtiles, plan.slices);
    if ((int)ceil_div_ll(L.vtiles, slice_tiles) != plan.slices) return FLOWGNN_ERR_ARG;  // (an empty slice: not a plan of vocab_head_plan)
    const size_t items = (size_t)num_graphs * positions;
    const int final = plan.slices == 1;
    float* const out_val = final ? scores : static_cast<float*>(part);
    int* const out_idx = final ? tokens : reinterpret_cast<int*>(static_cast<float*>(part) + (size_t)plan.slices * items);
    const dim3 grid((unsigned)plan.graph_blocks, (unsigned)plan.slices);
    vh_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(pooled, o, inv, num_graphs, positions, vocab, L.vtiles, slice_tiles, final, out_val, out_idx, range_flag);
    return 0;
}

int launch_vocab_head_fold(int emb_dim, const void* blob, int positions, int vocab, const VocabHeadPlan& plan, const void* part, int num_graphs,
                           int* tokens, float* scores, hipStream_t s) {
    if (!vh_args(emb_dim, positions, vocab)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || !part) return FLOWGNN_ERR_ARG;
    if (num_graphs <= 0 || plan.slices <= 1) return 0;
    const long long items = (long long)num_graphs * positions;
    const float* pv = static_cast<const float*>(part);
    vh_fold_kernel<<<(unsigned)ceil_div_ll(items, 256), 256, 0, s>>>(
        pv, reinterpret_cast<const int*>(pv + (size_t)plan.slices * items),
        reinterpret_cast<const float*>(static_cast<const uint8_t*>(blob) + VhBlob(positions, vocab).inv_off), plan.slices, items, tokens, scores);
    return 0;
}

int launch_vocab_head_f32(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, int* tokens, float* scores,
                          hipStream_t s) {
    if (!vh_args(emb_dim, positions, vocab)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob) return FLOWGNN_ERR_ARG;
    if (num_graphs <= 0) return 0;
    constexpr int D = VH_D;
    const VhBlob L(positions, vocab);
    const uint8_t* const o = static_cast<const uint8_t*>(blob);
    vh_f32_kernel<D><<<dim3((unsigned)ceil_div_ll(num_graphs, 8), (unsigned)positions), 256, 0, s>>>(
        pooled, reinterpret_cast<const float*>(o + L.wt_off), reinterpret_cast<const float*>(o + L.b_off), num_graphs, positions, vocab, L.v4, tokens,
        scores);
    return 0;
}

// ---- the top-k form's launchers
namespace {
inline bool vh_topk_args(const VocabTopk& top) { return top.k >= 1 && top.k <= VH_TOPK_MAX && top.tokens && top.scores && top.lse; }

// the parts of `part`: values and indices [S][G][P][K], then m and s [S][G][P]; all null where there is no `part` (one slice)
struct VhTopkPart {
    float *val = nullptr, *m = nullptr, *s = nullptr;
    int* idx = nullptr;
    VhTopkPart(const void* part, int slices, size_t items, int k) {
        if (!part || slices <= 1) return;
        const size_t lists = (size_t)slices * items * k;
        val = static_cast<float*>(const_cast<void*>(part));
        idx = reinterpret_cast<int*>(val + lists);
        m = val + 2 * lists;
        s = m + (size_t)slices * items;
    }
};
}  // namespace

int launch_vocab_topk(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, const VocabHeadPlan& plan,
                      void* part, int* tokens, float* scores, const VocabTopk& top, int* range_flag, hipStream_t s) {
    if (!vh_args(emb_dim, positions, vocab)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || !vh_topk_args(top) || plan.slices < 1 || (plan.slices > 1 && !part)) return FLOWGNN_ERR_ARG;
    if (num_graphs <= 0) return 0;
    constexpr int D = VH_D;
    const VhBlob L(positions, vocab);
    const uint8_t* const o = static_cast<const uint8_t*>(blob);
    const float* const inv = reinterpret_cast<const float*>(o + L.inv_off);
    const int slice_tiles = (int)ceil_div_ll(L.vtiles, plan.slices);
    if ((int)ceil_div_ll(L.vtiles, slice_tiles) != plan.slices) return FLOWGNN_ERR_ARG;  // (an empty slice: not a plan of vocab_head_plan)
    const int final = plan.slices == 1;
    const VhTopkPart pt(part, plan.slices, (size_t)num_graphs * positions, top.k);
    const dim3 grid((unsigned)plan.graph_blocks, (unsigned)plan.slices);
    vh_topk_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(pooled, o, inv, num_graphs, positions, vocab, L.vtiles, slice_tiles, final, top.k,
                                                     final ? top.scores : pt.val, final ? top.tokens : pt.idx, final ? top.lse : pt.m, pt.s, tokens,
                                                     scores, range_flag);
    return 0;
}

int launch_vocab_topk_fold(int emb_dim, const void* blob, int positions, int vocab, const VocabHeadPlan& plan, const void* part, int num_graphs,
                           int* tokens, float* scores, const VocabTopk& top, hipStream_t s) {
    if (!vh_args(emb_dim, positions, vocab)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || !part || !vh_topk_args(top)) return FLOWGNN_ERR_ARG;
    if (num_graphs <= 0 || plan.slices <= 1) return 0;
    const long long items = (long long)num_graphs * positions;
    const VhTopkPart pt(part, plan.slices, (size_t)items, top.k);
    vh_topk_fold_kernel<<<(unsigned)ceil_div_ll(items, 256), 256, 0, s>>>(
        pt.val, pt.idx, pt.m, pt.s, reinterpret_cast<const float*>(static_cast<const uint8_t*>(blob) + VhBlob(positions, vocab).inv_off), plan.slices,
        items, top.k, tokens, scores, top.tokens, top.scores, top.lse);
    return 0;
}

int launch_vocab_topk_f32(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, int* tokens, float* scores,
                          const VocabTopk& top, hipStream_t s) {
    if (!vh_args(emb_dim, positions, vocab)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || !vh_topk_args(top)) return FLOWGNN_ERR_ARG;
    if (num_graphs <= 0) return 0;
    constexpr int D = VH_D;
    const VhBlob L(positions, vocab);
    const uint8_t* const o = static_cast<const uint8_t*>(blob);
    vh_topk_f32_kernel<D><<<dim3((unsigned)ceil_div_ll(num_graphs, 4), (unsigned)positions), 256, 0, s>>>(
        pooled, reinterpret_cast<const float*>(o + L.wt_off), reinterpret_cast<const float*>(o + L.b_off), num_graphs, positions, vocab, L.v4, top.k,
        tokens, scores, top.tokens, top.scores, top.lse);
    return 0;
}

size_t ast_encoder_blob_bytes(int emb_dim, int n_types, int n_attrs, int max_depth) {
    if (emb_dim != VH_D || n_types < 1 || n_attrs < 1 || max_depth < 0) return 0;
    return ((size_t)n_types + (size_t)n_attrs + (size_t)max_depth + 1) * VH_D * 4;
}

void ast_encoder_blob_pack(int emb_dim, int n_types, int n_attrs, int max_depth, const float* type_tab, const float* attr_tab, const float* depth_tab,
                           void* out) {
    if (!ast_encoder_blob_bytes(emb_dim, n_types, n_attrs, max_depth)) return;
    float* o = static_cast<float*>(out);
    std::memcpy(o, type_tab, (size_t)n_types * VH_D * 4);
    std::memcpy(o + (size_t)n_types * VH_D, attr_tab, (size_t)n_attrs * VH_D * 4);
    std::memcpy(o + ((size_t)n_types + n_attrs) * VH_D, depth_tab, ((size_t)max_depth + 1) * VH_D * 4);
}

int launch_ast_encoder(int emb_dim, const void* blob, int n_types, int n_attrs, int max_depth, const int* x, const int* depth, float* h, int n_tot,
                       int* err, const float* vn_e, hipStream_t s) {
    if (!ast_encoder_blob_bytes(emb_dim, n_types, n_attrs, max_depth)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || !x || !depth) return FLOWGNN_ERR_ARG;
    if (n_tot <= 0) return 0;
    constexpr int D = VH_D;
    const float* const ty = static_cast<const float*>(blob);
    const float* const at = ty + (size_t)n_types * D;
    const float* const dp = at + (size_t)n_attrs * D;
    const int grid = grid_for((long long)n_tot * (D / 4), 256, 256 * 8);
    if (vn_e)
        ast_encoder_kernel<D, true><<<grid, 256, 0, s>>>(x, depth, ty, at, dp, n_types, n_attrs, max_depth, h, n_tot, err, vn_e);
    else
        ast_encoder_kernel<D, false><<<grid, 256, 0, s>>>(x, depth, ty, at, dp, n_types, n_attrs, max_depth, h, n_tot, err, nullptr);
    return 0;
}

}  // namespace fg
