// code2's vocabulary head scoring given target tokens (flowgnn_set_vocab_targets).
//
// With targets t [G][P] attached to the batch a run leaves, beside tokens and scores, per (g, p): the logit of entry t, the
// log-sum-exp of the position's V logits, and the rank of t -- how many entries v != t come before it under the head's one order
// (larger value, then lower index: vh_take).  The logits still never reach memory.  The rank compares every logit of the stream
// against the target's, so that value must exist before the stream pass and carry the bits the stream pass computes for entry t
// (otherwise t would be compared against another rounding of itself).  Three kernels:
//   * vh_target_kernel, a gathered-row product.  A wave holds 16 graphs (B: their pooled rows, split once as in vh_kernel) and loops
//     over the positions.  Row i of its A operand is not a vocabulary tile's: it is W[p][t_i], the target row of graph i, read where it
//     sits in the head's chunks -- gw_pack_tile puts row r of a tile's fragment at lane 16 gk + r, so lane (i, gk) reads its 16 bytes
//     of fragment (ks, hi | lo) of tile t_i / 16 at lane slot 16 gk + t_i % 16: global memory to registers, no LDS.  The accumulator
//     starts from that row's pre-scaled bias and the 30 MFMAs come in vh_tile_logits' order.  An MFMA output element depends on its own
//     A row and B column alone, so element (i, i) has the bits the stream pass gives entry t_i of graph i; the lane that holds it
//     writes it, scaled, to x [G][P] and times 1 / scale to the target's logit.  30 MFMAs per (16 graphs, position), where the stream
//     has 30 per (16 graphs, position, tile).
//   * vh_score_kernel: vh_kernel's grid, plan, chunk stream, LDS double buffer and B operands.  A lane keeps ONE running (max, index)
//     -- its candidates arrive in ascending index order, so a strict > gives what vh_kernel's four pairs and their fold give -- and
//     adds x and t of its graph, a count of the entries before t, and section 4.34's running (m, s).  Rows at or beyond V and the row
//     with index t are never counted.  At a position's end the four lane groups fold by two xor shuffles.  With more than one slice a
//     block leaves (value, index, count, m, s) per (slice, graph, position) and vh_score_fold_kernel folds them.
//   * vh_score_f32_kernel, the exact form behind the range guard: vh_f32_kernel's fma chain, k ascending, eight graphs per workgroup;
//     the target's logit comes from the same chain first, then the same counting rule and soft-max pair.
// A target outside -1 .. V - 1 raises the batch's error word (ERR_NODE_FEAT) and counts as -1: no address is formed from it.
#include <climits>
#include <cmath>

#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "wide_common.h"  // GW_WAVES, gw_issue_pieces
#include "wide_vocab_dev.h"
#include "wide_vocab_score.h"

namespace fg {
namespace {

__device__ __forceinline__ bool vs_is_target(int t, int vocab) { return t >= 0 && t < vocab; }

// x [G][P]: the targets' logits in the scaled domain (NaN: no target); logit [G][P]: times 1 / scale
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void vh_target_kernel(const float* __restrict__ pooled, const uint8_t* __restrict__ chunks,
                                                                  const float* __restrict__ inv_p, const int* __restrict__ targets, int num_graphs,
                                                                  int positions, int vocab, int vtiles, float* __restrict__ x,
                                                                  float* __restrict__ logit, int* __restrict__ err, int* __restrict__ range_flag) {
    using M = VhDims<D>;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const long long graph = ((long long)blockIdx.x * GW_WAVES + wave) * 16 + j;
    if (((long long)blockIdx.x * GW_WAVES + wave) * 16 >= num_graphs) return;  // (wave-uniform: a wave with no graph)
    ds_uint4_t b_hi[M::KS], b_lo[M::KS];
    const bool in_range = vh_load_b<D>(pooled, graph, num_graphs, g, b_hi, b_lo);
    const float inv = *inv_p;
#pragma unroll 1
    for (int p = 0; p < positions; p++) {
        int t = graph < num_graphs ? targets[(size_t)graph * positions + p] : -1;
        if (t != -1 && !vs_is_target(t, vocab)) {
            atomicMax(err, ERR_NODE_FEAT);
            t = -1;
        }
        const int tr = t < 0 ? 0 : t;  // (no target: row 0's product, discarded)
        // row tr % 16 of tile tr / 16: gw_pack_tile's lane slot 16 gk + row of every fragment, and the row's bias behind the fragments
        const uint8_t* const ck = chunks + ((size_t)p * vtiles + (tr >> 4)) * M::CHUNK_STRIDE;
        const uint8_t* const frag = ck + (16 * g + (tr & 15)) * 16;
        const float bias = *reinterpret_cast<const float*>(ck + M::BIAS_OFF + (tr & 15) * 4);
        float4_t acc = (float4_t){bias, bias, bias, bias};  // (column j of the accumulator: graph j's target row is A's row j)
        ds_uint4_t a_hi[M::KS], a_lo[M::KS];
#pragma unroll
        for (int ks = 0; ks < M::KS; ks++) {
            a_hi[ks] = *reinterpret_cast<const ds_uint4_t*>(frag + (ks * 2) * 1024);
            a_lo[ks] = *reinterpret_cast<const ds_uint4_t*>(frag + (ks * 2 + 1) * 1024);
        }
#pragma unroll
        for (int ks = 0; ks < M::KS; ks++) {  // vh_tile_logits' order
            acc = DS_MFMA16(a_hi[ks], b_hi[ks], acc);
            acc = DS_MFMA16(a_hi[ks], b_lo[ks], acc);
            acc = DS_MFMA16(a_lo[ks], b_hi[ks], acc);
        }
        // the lane holds rows 4 g .. 4 g + 3 of column j: the diagonal is row j, in lane group j / 4
        const int r = j & 3;
        const float v = r == 0 ? acc.x : r == 1 ? acc.y : r == 2 ? acc.z : acc.w;
        if (g == (j >> 2) && graph < num_graphs) {
            const size_t o = (size_t)graph * positions + p;
            x[o] = t < 0 ? __builtin_nanf("") : v;
            logit[o] = t < 0 ? __builtin_nanf("") : v * inv;
        }
    }
    if (__any(!in_range)) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

// out_val / out_idx / out_cnt / out_m / out_s [slice][G][P]: the slice's partial results (value and m in the scaled / log2 domain); or,
// with `final` (one slice), scores, tokens, rank and lse (out_s unused)
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void vh_score_kernel(const float* __restrict__ pooled, const uint8_t* __restrict__ chunks,
                                                                 const float* __restrict__ inv_p, const int* __restrict__ targets,
                                                                 const float* __restrict__ x, int num_graphs, int positions, int vocab, int vtiles,
                                                                 int slice_tiles, int final, float* __restrict__ out_val, int* __restrict__ out_idx,
                                                                 int* __restrict__ out_cnt, float* __restrict__ out_m, float* __restrict__ out_s,
                                                                 int* __restrict__ range_flag) {
    using M = VhDims<D>;
    // two DISTINCT LDS objects, as in vh_kernel: the DMA into one does not alias the reads of the other
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

    ds_uint4_t b_hi[M::KS], b_lo[M::KS];
    const long long graph = ((long long)blockIdx.x * GW_WAVES + wave) * 16 + j;
    const bool in_range = vh_load_b<D>(pooled, graph, num_graphs, g, b_hi, b_lo);
    const float inv = *inv_p;
    const float c2 = inv * VH_LOG2E;  // scaled logit -> y
    const size_t item0 = (size_t)(graph < num_graphs ? graph : 0) * positions;

    float best = -__builtin_inff(), m = -__builtin_inff(), sum = 0.0f;
    int bi = INT_MAX, cnt = 0;  // bi INT_MAX: none yet
    // this position's target and its scaled logit; a lane beyond the batch has none (every compare with NaN fails)
    int tt = graph < num_graphs ? targets[item0] : -1;
    float tx = graph < num_graphs ? x[item0] : __builtin_nanf("");

    auto tile = [&](const char* wb, int t) {
        const float4_t acc = vh_tile_logits<D>(wb, lane, g, b_hi, b_lo);
        const int r0 = 16 * t + 4 * g;
        const float v[4] = {acc.x, acc.y, acc.z, acc.w};
        // the tile's four y into (m, s) with one rescale, as in vh_topk_kernel; rows at or beyond V are nothing at all
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
            if (r0 + r < vocab) {
                sum += __builtin_amdgcn_exp2f(v[r] * c2 - m);
                if (v[r] > best) {  // (strict, indices ascending: the lowest index keeps a tie)
                    best = v[r];
                    bi = r0 + r;
                }
                cnt += (r0 + r != tt && (v[r] > tx || (v[r] == tx && r0 + r < tt))) ? 1 : 0;
            }
    };

    // the end of a position: fold the graph's four lane groups; lane group 0 stores; then the next position's target
    auto finish = [&](int p) {
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
            const float ob = __shfl_xor(best, off);
            const int oi = __shfl_xor(bi, off);
            vh_take(best, bi, ob, oi);
            cnt += __shfl_xor(cnt, off);
            const float om = __shfl_xor(m, off);
            const float os = __shfl_xor(sum, off);
            vh_lse_fold(m, sum, om, os);
        }
        if (g == 0 && graph < num_graphs) {
            const size_t o = ((size_t)blockIdx.y * num_graphs + (size_t)graph) * positions + p;
            out_val[o] = final ? best * inv : best;
            out_idx[o] = final && bi == INT_MAX ? 0 : bi;  // (0 for INT_MAX: on a pass that the engine repeats, as in vh_kernel)
            out_cnt[o] = final && !vs_is_target(tt, vocab) ? -1 : cnt;
            out_m[o] = final ? vh_lse_value(m, sum) : m;
            if (!final) out_s[o] = sum;
        }
        best = m = -__builtin_inff();
        sum = 0.0f;
        bi = INT_MAX;
        cnt = 0;
        if (p + 1 < positions && graph < num_graphs) {
            tt = targets[item0 + p + 1];
            tx = x[item0 + p + 1];
        }
    };

    // every wait for the DMA also takes (tt, tx) as operands: the compiler then puts its own wait for their loads here, where nothing
    // is in flight afterwards anyway, and not in front of their first use, where the next chunk's DMA has just been issued
#define VS_WAIT_ALL() asm volatile("s_waitcnt vmcnt(0)" : "+v"(tt), "+v"(tx)::"memory")
    VS_WAIT_ALL();
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < n; i += 2) {
        if (i + 1 < n) gw_issue_pieces<M::PIECES>(chunk(i + 1), s_b, M::PIECES, M::LAST_LANES, wave, lane);
        {
            const int p = i / nt, tl = i - p * nt;
            tile(s_a, t0 + tl);
            if (tl == nt - 1) finish(p);
        }
        VS_WAIT_ALL();  // this wave's pieces of chunk i + 1 have landed (and the next target)
        __syncthreads();                                  // everyone's have; everyone is done with s_a
        if (i + 1 < n) {                                  // (uniform over the workgroup)
            if (i + 2 < n) gw_issue_pieces<M::PIECES>(chunk(i + 2), s_a, M::PIECES, M::LAST_LANES, wave, lane);
            const int p = (i + 1) / nt, tl = i + 1 - p * nt;
            tile(s_b, t0 + tl);
            if (tl == nt - 1) finish(p);
            VS_WAIT_ALL();
            __syncthreads();
        }
    }
#undef VS_WAIT_ALL
    if (__any(!in_range)) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

// The slices' partial results [S][G][P] into tokens, scores, rank and lse [G][P]: slices ascending, so are their indices
__global__ __launch_bounds__(256) void vh_score_fold_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                                                            const int* __restrict__ part_cnt, const float* __restrict__ part_m,
                                                            const float* __restrict__ part_s, const float* __restrict__ inv_p,
                                                            const int* __restrict__ targets, int slices, long long items, int vocab,
                                                            int* __restrict__ tokens, float* __restrict__ scores, int* __restrict__ rank,
                                                            float* __restrict__ lse) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    float best = -__builtin_inff(), m = -__builtin_inff(), sum = 0.0f;
    int bi = INT_MAX, cnt = 0;
    for (int s = 0; s < slices; s++) {
        const size_t o = (size_t)s * items + i;
        vh_take(best, bi, part_val[o], part_idx[o]);
        cnt += part_cnt[o];
        vh_lse_fold(m, sum, part_m[o], part_s[o]);
    }
    tokens[i] = bi == INT_MAX ? 0 : bi;
    scores[i] = best * *inv_p;
    rank[i] = vs_is_target(targets[i], vocab) ? cnt : -1;
    lse[i] = vh_lse_value(m, sum);
}

// The exact form: logit = fma chain from the bias, k ascending, as in vh_f32_kernel: eight graphs per workgroup staged in LDS, the
// first eight threads run the chain of their graph's target entry, then a thread owns vocabulary entries tid, tid + 256, .. and the
// 256 threads' maxima, counts and soft-max pairs are folded
template <int D>
__global__ __launch_bounds__(256) void vh_score_f32_kernel(const float* __restrict__ pooled, const float* __restrict__ wt, const float* __restrict__ b,
                                                           const int* __restrict__ targets, int num_graphs, int positions, int vocab, int v4,
                                                           int* __restrict__ tokens, float* __restrict__ scores, float* __restrict__ logit,
                                                           float* __restrict__ lse, int* __restrict__ rank, int* __restrict__ err) {
    constexpr int RB = 8;
    __shared__ float s_in[RB][D];
    __shared__ float s_m[RB][256];
    __shared__ int s_i[RB][256];
    __shared__ float s_x[RB];
    __shared__ int s_t[RB];
    __shared__ float s_pm[RB][4], s_ps[RB][4];  // the four waves' soft-max pairs ...
    __shared__ int s_pc[RB][4];                 // ... and counts
    const long long g0 = (long long)blockIdx.x * RB;
    const int p = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < RB * D; i += 256) {
        const int r = i / D, k = i - r * D;
        s_in[r][k] = g0 + r < num_graphs ? pooled[(size_t)(g0 + r) * D + k] : 0.0f;
    }
    __syncthreads();
    const float* wp = wt + (size_t)p * D * v4;
    if (tid < RB) {
        int t = g0 + tid < num_graphs ? targets[(size_t)(g0 + tid) * positions + p] : -1;
        if (t != -1 && !vs_is_target(t, vocab)) {
            atomicMax(err, ERR_NODE_FEAT);
            t = -1;
        }
        float acc = __builtin_nanf("");
        if (t >= 0) {
            acc = b[(size_t)p * v4 + t];
            for (int k = 0; k < D; k++) acc = __builtin_fmaf(s_in[tid][k], wp[(size_t)k * v4 + t], acc);
        }
        s_t[tid] = t;
        s_x[tid] = acc;
    }
    __syncthreads();
    float best[RB], m[RB], sum[RB];
    int bi[RB], cnt[RB];
#pragma unroll
    for (int r = 0; r < RB; r++) {
        best[r] = m[r] = -__builtin_inff();
        sum[r] = 0.0f;
        bi[r] = INT_MAX;
        cnt[r] = 0;
    }
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
            if (acc[r] > best[r]) {
                best[r] = acc[r];
                bi[r] = v;
            }
            cnt[r] += (v != s_t[r] && (acc[r] > s_x[r] || (acc[r] == s_x[r] && v < s_t[r]))) ? 1 : 0;
        }
    }
#pragma unroll
    for (int r = 0; r < RB; r++) {
        s_m[r][tid] = best[r];
        s_i[r][tid] = bi[r];
        for (int off = 1; off < 64; off <<= 1) {
            const float om = __shfl_xor(m[r], off);
            const float os = __shfl_xor(sum[r], off);
            vh_lse_fold(m[r], sum[r], om, os);
            cnt[r] += __shfl_xor(cnt[r], off);
        }
        if ((tid & 63) == 0) {
            s_pm[r][tid >> 6] = m[r];
            s_ps[r][tid >> 6] = sum[r];
            s_pc[r][tid >> 6] = cnt[r];
        }
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
        float fm = s_pm[tid][0], fs = s_ps[tid][0];
        int fc = s_pc[tid][0];
        for (int w = 1; w < 4; w++) {
            vh_lse_fold(fm, fs, s_pm[tid][w], s_ps[tid][w]);
            fc += s_pc[tid][w];
        }
        logit[o] = s_x[tid];
        lse[o] = vh_lse_value(fm, fs);
        rank[o] = s_t[tid] < 0 ? -1 : fc;
    }
}

inline bool vs_args(const VocabScore& sc) { return sc.targets && sc.logit && sc.lse && sc.rank; }

// the parts of `part`: x [G][P], then -- more than one slice -- values, indices, counts, m and s [S][G][P]
struct VsPart {
    float *x, *val = nullptr, *m = nullptr, *s = nullptr;
    int *idx = nullptr, *cnt = nullptr;
    VsPart(const void* part, int slices, size_t items) {
        x = static_cast<float*>(const_cast<void*>(part));
        if (slices <= 1) return;
        const size_t n = (size_t)slices * items;
        val = x + items;
        idx = reinterpret_cast<int*>(val + n);
        cnt = idx + n;
        m = val + 3 * n;
        s = m + n;
    }
};

}  // namespace

size_t vocab_score_part_words(const VocabHeadPlan& plan, int num_graphs, int positions) {
    const size_t items = (size_t)num_graphs * (size_t)positions;
    // section 4.33's pairs per (slice, item), and a count and an (m, s) pair more
    return items + vocab_head_part_words(plan, num_graphs, positions, 0) + (plan.slices > 1 ? 3 * (size_t)plan.slices * items : 0);
}

int launch_vocab_target(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, void* part,
                        const VocabScore& sc, int* err, int* range_flag, hipStream_t s) {
    if (!vh_args(emb_dim, positions, vocab)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || !part || !vs_args(sc) || !err) return FLOWGNN_ERR_ARG;
    if (num_graphs <= 0) return 0;
    const VhBlob L(positions, vocab);
    const uint8_t* const o = static_cast<const uint8_t*>(blob);
    vh_target_kernel<VH_D><<<(unsigned)ceil_div_ll(num_graphs, GW_WAVES * 16), GW_WAVES * 64, 0, s>>>(
        pooled, o, reinterpret_cast<const float*>(o + L.inv_off), sc.targets, num_graphs, positions, vocab, L.vtiles, static_cast<float*>(part), sc.logit,
        err, range_flag);
    return 0;
}

int launch_vocab_score(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, const VocabHeadPlan& plan,
                       void* part, int* tokens, float* scores, const VocabScore& sc, int* range_flag, hipStream_t s) {
    if (!vh_args(emb_dim, positions, vocab)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || !part || !vs_args(sc) || plan.slices < 1) return FLOWGNN_ERR_ARG;
    if (num_graphs <= 0) return 0;
    const VhBlob L(positions, vocab);
    const uint8_t* const o = static_cast<const uint8_t*>(blob);
    const int slice_tiles = (int)ceil_div_ll(L.vtiles, plan.slices);
    if ((int)ceil_div_ll(L.vtiles, slice_tiles) != plan.slices) return FLOWGNN_ERR_ARG;  // (an empty slice: not a plan of vocab_head_plan)
    const int final = plan.slices == 1;
    const VsPart pt(part, plan.slices, (size_t)num_graphs * positions);
    const dim3 grid((unsigned)plan.graph_blocks, (unsigned)plan.slices);
    vh_score_kernel<VH_D><<<grid, GW_WAVES * 64, 0, s>>>(pooled, o, reinterpret_cast<const float*>(o + L.inv_off), sc.targets, pt.x, num_graphs, positions,
                                                         vocab, L.vtiles, slice_tiles, final, final ? scores : pt.val, final ? tokens : pt.idx,
                                                         final ? sc.rank : pt.cnt, final ? sc.lse : pt.m, pt.s, range_flag);
    return 0;
}

int launch_vocab_score_fold(int emb_dim, const void* blob, int positions, int vocab, const VocabHeadPlan& plan, const void* part, int num_graphs,
                            int* tokens, float* scores, const VocabScore& sc, hipStream_t s) {
    if (!vh_args(emb_dim, positions, vocab)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || !part || !vs_args(sc)) return FLOWGNN_ERR_ARG;
    if (num_graphs <= 0 || plan.slices <= 1) return 0;
    const long long items = (long long)num_graphs * positions;
    const VsPart pt(part, plan.slices, (size_t)items);
    vh_score_fold_kernel<<<(unsigned)ceil_div_ll(items, 256), 256, 0, s>>>(
        pt.val, pt.idx, pt.cnt, pt.m, pt.s, reinterpret_cast<const float*>(static_cast<const uint8_t*>(blob) + VhBlob(positions, vocab).inv_off),
        sc.targets, plan.slices, items, vocab, tokens, scores, sc.rank, sc.lse);
    return 0;
}

int launch_vocab_score_f32(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, int* tokens, float* scores,
                           const VocabScore& sc, int* err, hipStream_t s) {
    if (!vh_args(emb_dim, positions, vocab)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!blob || !vs_args(sc) || !err) return FLOWGNN_ERR_ARG;
    if (num_graphs <= 0) return 0;
    const VhBlob L(positions, vocab);
    const uint8_t* const o = static_cast<const uint8_t*>(blob);
    vh_score_f32_kernel<VH_D><<<dim3((unsigned)ceil_div_ll(num_graphs, 8), (unsigned)positions), 256, 0, s>>>(
        pooled, reinterpret_cast<const float*>(o + L.wt_off), reinterpret_cast<const float*>(o + L.b_off), sc.targets, num_graphs, positions, vocab, L.v4,
        tokens, scores, sc.logit, sc.lse, sc.rank, err);
    return 0;
}

}  // namespace fg
