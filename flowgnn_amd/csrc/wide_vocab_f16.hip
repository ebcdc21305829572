// code2's vocabulary head in its f16 numeric mode (flowgnn_set_vocab_head_numeric): vh_f16_kernel.
//
// The rule: logit = (b s + sum_k r(W s) r(pooled)) / s, r to nearest even to f16, fp32 accumulation on the matrix pipe from the
// pre-scaled bias.  One MFMA per K-step where vh_kernel (wide_vocab.hip, section 4.33) issues three, half the weight stream, and B
// operands of 40 registers per graph tile instead of 80 -- which is what lets a wave hold SEVERAL graph tiles:
//   * B: the pooled rows of the wave's T tiles of 16 graphs, rounded once (gwf_pack_rne, the f16 layer kernels' conversion) and held
//     in registers for the whole launch: 40 T registers.  A workgroup of eight waves owns 128 T graphs.
//   * A: a chunk of the stream is TWO 16-row vocabulary tiles, each its 10 hi fragments of 1 KiB (gw_pack_tile's layout) and its 16
//     pre-scaled biases: 20 608 bytes, 21 DMA pieces, so a chunk buffer is the size it is in vh_kernel.  Chunks go L2 -> LDS by
//     LDS-DMA (gw_issue_pieces), double buffered in two distinct LDS objects and shared by the eight waves; one s_waitcnt vmcnt(0) and
//     one barrier per chunk, that is per 20 T MFMAs of a wave where vh_kernel has one per 30.
//   * A fragment read of 1 KiB feeds T MFMAs: the T accumulators of a vocabulary tile advance side by side, so consecutive MFMAs are
//     independent and the LDS traffic per MFMA is 1 / T of a one-tile wave's.
//   * The running maximum, the fold at the end of a position, the slices' partial pairs and the INT_MAX convention are vh_kernel's,
//     per graph tile: 8 T registers.  Rows at or beyond V -- the zero rows of a last tile, and the zero second tile of a position's last
//     chunk when the tile count is odd -- are never compared.
//   * Grid: x = blocks of 128 T graphs, y = slices of a whole number of chunks (vocab_head_f16_plan).
// The range rule is section 4.33's: a pooled value at or beyond 6e4 or not finite raises *range_flag.
#include <climits>
#include <cstring>

#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "gin_wide_f16_body.h"  // gwf_pack_rne
#include "wide_common.h"        // GW_WAVES, gw_issue_pieces
#include "wide_vocab_f16.h"

#ifndef FLOWGNN_VHF_TILES
#define FLOWGNN_VHF_TILES 2  // T, the graph tiles of a wave: section 4.35 has the candidates and their measurement
#endif
#ifdef FLOWGNN_VHF_WAVES
#define VHF_OCCUPANCY __attribute__((amdgpu_waves_per_eu(FLOWGNN_VHF_WAVES, FLOWGNN_VHF_WAVES)))
#else
#define VHF_OCCUPANCY
#endif

namespace fg {
namespace {

constexpr int VHF_T = FLOWGNN_VHF_TILES;
constexpr int VHF_D = FLOWGNN_EMB_DIM_OGB;
constexpr int VHF_MIN_SLICE_TILES = 4;  // as in section 4.33: the B operands are set up once per block

template <int D>
struct VhfDims {
    static_assert(D % 4 == 0, "rows are read as float4 pieces");
    static constexpr int KS = (D + 31) / 32;          // K-steps (K padded to 32 KS)
    static constexpr int BIAS_OFF = KS * 1024;        // of a tile: fragment ks at ks * 1024, then 16 floats
    static constexpr int TILE_BYTES = BIAS_OFF + 64;  // (a multiple of 16: the second tile's fragments stay aligned)
    static constexpr int CHUNK_BYTES = 2 * TILE_BYTES;
    static constexpr int PIECES = (CHUNK_BYTES + 1023) / 1024;
    static constexpr int LAST_LANES = (CHUNK_BYTES - (PIECES - 1) * 1024) / 16;
    static constexpr int CHUNK_STRIDE = PIECES * 1024;  // in global memory
    // the head's own chunk (wide_vocab.hip: VhDims): fragment (ks * 2 + half), then the biases
    static constexpr int SRC_BIAS_OFF = KS * 2 * 1024;
    static constexpr int SRC_STRIDE = (SRC_BIAS_OFF + 64 + 1023) / 1024 * 1024;
    static_assert(2 * CHUNK_BYTES <= 64 * 1024, "two chunk buffers, and room for more than one workgroup on a CU");
};

// (larger value, then lower index): vh_take's rule (wide_vocab.hip), restated so that that file stays as it is
__device__ __forceinline__ void vhf_take(float& m, int& idx, float cm, int cidx) {
    if (cm > m || (cm == m && cidx < idx)) {
        m = cm;
        idx = cidx;
    }
}

// One chunk from `wb`: vocabulary tiles t2, t2 + 1 against the wave's T graph tiles, and the update of the running pairs
template <int D, int T>
__device__ __forceinline__ void vhf_chunk(const char* wb, int t2, int lane, int g, int vocab, const ds_uint4_t (&b)[T][VhfDims<D>::KS],
                                          float (&best)[T][4], int (&bt)[T][4]) {
    using M = VhfDims<D>;
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const char* tb = wb + u * M::TILE_BYTES;
        const float4 bv = *reinterpret_cast<const float4*>(tb + M::BIAS_OFF + g * 16);
        float4_t acc[T];
#pragma unroll
        for (int t = 0; t < T; t++) acc[t] = (float4_t){bv.x, bv.y, bv.z, bv.w};
        // the fragment one K-step ahead of its MFMAs, and no further (the compiler barrier keeps the scheduler from hoisting all ten reads)
        ds_uint4_t nx = *reinterpret_cast<const ds_uint4_t*>(tb + lane * 16);
#pragma unroll
        for (int ks = 0; ks < M::KS; ks++) {
            const ds_uint4_t a = nx;
            if (ks + 1 < M::KS) nx = *reinterpret_cast<const ds_uint4_t*>(tb + (ks + 1) * 1024 + lane * 16);
            asm volatile("" ::: "memory");
#pragma unroll
            for (int t = 0; t < T; t++) acc[t] = DS_MFMA16(a, b[t][ks], acc[t]);
        }
        const int r0 = 16 * (t2 + u) + 4 * g;  // rows r0 .. r0 + 3 of the lane's graph in every graph tile
#pragma unroll
        for (int t = 0; t < T; t++) {
            const float v[4] = {acc[t].x, acc[t].y, acc[t].z, acc[t].w};
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (r0 + r < vocab && v[r] > best[t][r]) {  // (strict: an equal logit of a later tile does not replace an earlier one)
                    best[t][r] = v[r];
                    bt[t][r] = t2 + u;
                }
        }
    }
}

// out_val / out_idx [slice][G][P]: the slice's partial pairs in the scaled domain; or, with `final` (one slice), scores and tokens.
// vchunks: chunks per position in the stream; slice_chunks: of a slice (the last one of a position may be shorter, none is empty)
template <int D, int T = VHF_T>
__global__ __launch_bounds__(GW_WAVES * 64) VHF_OCCUPANCY void vh_f16_kernel(const float* __restrict__ pooled, const uint8_t* __restrict__ chunks,
                                                               const float* __restrict__ inv_p, int num_graphs, int positions, int vocab,
                                                               int vchunks, int slice_chunks, int final, float* __restrict__ out_val,
                                                               int* __restrict__ out_idx, int* __restrict__ range_flag) {
    using M = VhfDims<D>;
    // two DISTINCT LDS objects, as in vh_kernel: the DMA into one does not alias the reads of the other
    __shared__ __attribute__((aligned(16))) char s_a[M::CHUNK_BYTES];
    __shared__ __attribute__((aligned(16))) char s_b[M::CHUNK_BYTES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int c0 = blockIdx.y * slice_chunks;
    const int nc = (vchunks - c0 < slice_chunks ? vchunks - c0 : slice_chunks);  // (the host cuts no empty slice)
    const int n = positions * nc;                                                // chunks of this block: (p, c) with c fastest
    auto chunk = [&](int i) {
        const int p = i / nc;
        return chunks + ((size_t)p * vchunks + c0 + (i - p * nc)) * M::CHUNK_STRIDE;
    };
    gw_issue_pieces<M::PIECES>(chunk(0), s_a, M::PIECES, M::LAST_LANES, wave, lane);

    // ---- the B operands: the pooled rows of this wave's T x 16 graphs, rounded once to nearest
    ds_uint4_t b[T][M::KS];
    const long long graph0 = ((long long)blockIdx.x * GW_WAVES + wave) * (16 * T) + j;  // of graph tile 0; tile t: + 16 t
    float vmax = 0.0f;
#pragma unroll
    for (int t = 0; t < T; t++) {
        const long long graph = graph0 + 16 * t;
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
            b[t][ks].x = gwf_pack_rne(x0.x, x0.y);
            b[t][ks].y = gwf_pack_rne(x0.z, x0.w);
            b[t][ks].z = gwf_pack_rne(x1.x, x1.y);
            b[t][ks].w = gwf_pack_rne(x1.z, x1.w);
            // (set-up code: keep the scheduler from holding every row piece at once, and from sinking the range compares -- and with
            // them every fp32 piece -- to the end of the kernel, where vmax is read)
            asm volatile("" : "+v"(vmax)::"memory");
        }
    }
    float best[T][4];
    int bt[T][4];  // the vocabulary tile of `best`; INT_MAX: none yet
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            best[t][r] = -__builtin_inff();
            bt[t][r] = INT_MAX;
        }
    const float inv = *inv_p;

    // the end of a position: per graph tile, fold the lane's four pairs, then the graph's four lane groups; lane group 0 stores
    auto finish = [&](int p) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            float m = -__builtin_inff();
            int idx = INT_MAX;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                vhf_take(m, idx, best[t][r], bt[t][r] == INT_MAX ? INT_MAX : 16 * bt[t][r] + 4 * g + r);
                best[t][r] = -__builtin_inff();
                bt[t][r] = INT_MAX;
            }
#pragma unroll
            for (int off = 16; off < 64; off <<= 1) {
                const float om = __shfl_xor(m, off);
                const int oi = __shfl_xor(idx, off);
                vhf_take(m, idx, om, oi);
            }
            const long long graph = graph0 + 16 * t;
            if (g == 0 && graph < num_graphs) {
                const size_t o = ((size_t)blockIdx.y * num_graphs + (size_t)graph) * positions + p;
                out_val[o] = final ? m * inv : m;
                // (INT_MAX: only on a pass that the engine repeats with vh_f32_kernel, as vh_kernel says where it writes its 0)
                out_idx[o] = final && idx == INT_MAX ? 0 : idx;
            }
        }
    };

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < n; i += 2) {
        if (i + 1 < n) gw_issue_pieces<M::PIECES>(chunk(i + 1), s_b, M::PIECES, M::LAST_LANES, wave, lane);
        {
            const int p = i / nc, cl = i - p * nc;
            vhf_chunk<D, T>(s_a, 2 * (c0 + cl), lane, g, vocab, b, best, bt);
            if (cl == nc - 1) finish(p);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of chunk i + 1 have landed
        __syncthreads();                                  // everyone's have; everyone is done with s_a
        if (i + 1 < n) {                                  // (uniform over the workgroup)
            if (i + 2 < n) gw_issue_pieces<M::PIECES>(chunk(i + 2), s_a, M::PIECES, M::LAST_LANES, wave, lane);
            const int p = (i + 1) / nc, cl = i + 1 - p * nc;
            vhf_chunk<D, T>(s_b, 2 * (c0 + cl), lane, g, vocab, b, best, bt);
            if (cl == nc - 1) finish(p);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
    if (__any(!(vmax < 6.0e4f))) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

// the parts of the stream (wide_vocab_f16.h)
struct VhfBlob {
    size_t inv_off, bytes, src_inv_off;
    int vtiles, vchunks;
    VhfBlob(int positions, int vocab) {
        vtiles = (vocab + 15) / 16;
        vchunks = (vtiles + 1) / 2;
        inv_off = (size_t)positions * vchunks * VhfDims<VHF_D>::CHUNK_STRIDE;
        bytes = inv_off + 16;
        src_inv_off = (size_t)positions * vtiles * VhfDims<VHF_D>::SRC_STRIDE;
    }
};

inline bool vhf_args(int emb_dim, int positions, int vocab) {
    return emb_dim == VHF_D && positions >= 1 && positions <= FLOWGNN_MAX_VOCAB_POSITIONS && vocab >= 1 && vocab <= FLOWGNN_MAX_VOCAB;
}

// a slice's tiles for `slices` slices: whole chunks
inline int vhf_slice_tiles(int vtiles, long long slices) { return (int)((ceil_div_ll(vtiles, slices) + 1) / 2 * 2); }

}  // namespace

size_t vocab_head_f16_blob_bytes(int emb_dim, int positions, int vocab) { return vhf_args(emb_dim, positions, vocab) ? VhfBlob(positions, vocab).bytes : 0; }

size_t vocab_head_f16_source_bytes(int emb_dim, int positions, int vocab) {
    return vhf_args(emb_dim, positions, vocab) ? VhfBlob(positions, vocab).src_inv_off + 16 : 0;
}

void vocab_head_f16_blob_pack(int emb_dim, int positions, int vocab, const void* blob, void* out) {
    if (!vhf_args(emb_dim, positions, vocab)) return;
    using M = VhfDims<VHF_D>;
    const VhfBlob L(positions, vocab);
    const uint8_t* const src = static_cast<const uint8_t*>(blob);
    uint8_t* const o = static_cast<uint8_t*>(out);
    std::memset(o, 0, L.bytes);
    for (int p = 0; p < positions; p++)
        for (int t = 0; t < L.vtiles; t++) {
            const uint8_t* ck = src + ((size_t)p * L.vtiles + t) * M::SRC_STRIDE;
            uint8_t* tile = o + ((size_t)p * L.vchunks + t / 2) * M::CHUNK_STRIDE + (size_t)(t & 1) * M::TILE_BYTES;
            for (int ks = 0; ks < M::KS; ks++) std::memcpy(tile + ks * 1024, ck + (size_t)ks * 2048, 1024);  // the hi half of the pair
            std::memcpy(tile + M::BIAS_OFF, ck + M::SRC_BIAS_OFF, 64);
        }
    std::memcpy(o + L.inv_off, src + L.src_inv_off, 4);
}

int vocab_head_f16_graph_tiles() { return VHF_T; }

VocabHeadPlan vocab_head_f16_plan(int num_graphs, int vocab, int cus) {
    VocabHeadPlan pl;
    pl.graph_blocks = (int)ceil_div_ll(num_graphs, GW_WAVES * 16 * VHF_T);
    // slices as vocab_head_plan cuts them -- enough blocks for two per compute unit, none under VHF_MIN_SLICE_TILES tiles, none empty --
    // and of an even number of tiles: a chunk never straddles two slices, and only a position's last chunk can be half empty
    const int vtiles = (vocab + 15) / 16;
    long long want = ceil_div_ll(2LL * (cus > 0 ? cus : 1), pl.graph_blocks > 0 ? pl.graph_blocks : 1);
    const long long most = ceil_div_ll(vtiles, VHF_MIN_SLICE_TILES);
    if (want > most) want = most;
    if (want < 1) want = 1;
    pl.slices = (int)ceil_div_ll(vtiles, vhf_slice_tiles(vtiles, want));
    return pl;
}

int launch_vocab_head_f16(int emb_dim, const void* stream, int positions, int vocab, const float* pooled, int num_graphs, const VocabHeadPlan& plan,
                          void* part, int* tokens, float* scores, int* range_flag, hipStream_t s) {
    if (!vhf_args(emb_dim, positions, vocab)) return FLOWGNN_ERR_UNSUPPORTED;
    if (!stream || plan.slices < 1 || (plan.slices > 1 && !part)) return FLOWGNN_ERR_ARG;
    if (num_graphs <= 0) return 0;
    const VhfBlob L(positions, vocab);
    const uint8_t* const o = static_cast<const uint8_t*>(stream);
    const int slice_tiles = vhf_slice_tiles(L.vtiles, plan.slices);
    // (an empty slice, or blocks that do not cover the graphs: not a plan of vocab_head_f16_plan)
    if ((int)ceil_div_ll(L.vtiles, slice_tiles) != plan.slices || (long long)plan.graph_blocks * GW_WAVES * 16 * VHF_T < num_graphs) return FLOWGNN_ERR_ARG;
    const size_t items = (size_t)num_graphs * positions;
    const int final = plan.slices == 1;
    float* const out_val = final ? scores : static_cast<float*>(part);
    int* const out_idx = final ? tokens : reinterpret_cast<int*>(static_cast<float*>(part) + (size_t)plan.slices * items);
    const dim3 grid((unsigned)plan.graph_blocks, (unsigned)plan.slices);
    vh_f16_kernel<VHF_D><<<grid, GW_WAVES * 64, 0, s>>>(pooled, o, reinterpret_cast<const float*>(o + L.inv_off), num_graphs, positions, vocab, L.vchunks,
                                                        slice_tiles / 2, final, out_val, out_idx, range_flag);
    return 0;
}

}  // namespace fg
