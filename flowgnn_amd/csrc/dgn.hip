// dgn.hip -- DGN hot path for gfx950 (MI355X).
//
// Reference per graph (DGN/src/*.cc), 4 layers, dim 100, no edge features, eigenvector #1 per node:
//   h0[v]   = sum_{k<9} Table[k][feat_k(v)]              (dense [9][119][100] table)   load_inputs.cc:114-172
//   w_e     = eig1[u] - eig1[v]  for edge (u -> v);  abssum[v] = sum |w_e|,  wsum[v] = sum w_e   load_inputs.cc:92-111
//   m1[v]   = sum h[u],   m2[v] = sum h[u] w_e                                          message_passing.cc:148-149
//   a1      = m1 / outdeg(v)   (x / 0 = 0, see oracle/dgn_oracle.c),
//   a2      = | (m2 - wsum[v] h[v]) / abssum[v] |   (abssum 0 -> 2^-13)                node_embedding.cc:125-146
//   h'[v]   = h[v] + relu(b + W[:,0,:] a1 + W[:,1,:] a2)       W viewed as [100][2][100] node_embedding.cc:148-181
//   out[g]  = head(mean_v h_4[v]),  head = 100 -> 50 (ReLU) -> 25 (ReLU) -> 1            finalize.cc:28-52
//
// Here: one HBM-bound aggregation kernel per layer that writes z[v] = [a1 | a2] (the directional weights are
// recomputed from the eigenvector column, 4 B per node, instead of being stored per edge), one fp32-MFMA
// dense kernel (K = 200) with the residual in its epilogue, one wave-per-graph readout kernel.
#include "common.h"
#include "device_common.h"
#include "modelq.h"
#include "dense_split.h"
#include "dgn_plan.h"
#include <cmath>
#include <cstring>

namespace fg {
// dgn_emb.hip compiles this file once more with FG_RESIDENT_EMB_TU defined, for ONE kernel: dgn_resident_kernel under the name
// dgn_resident_emb_kernel, the instance that also stores every graph's pooled row (flowgnn_set_embeddings).  A second instance in
// this translation unit or a pointer tested at run time both cost the default kernel registers (and 0.4 - 1.7 % of its time); this way
// the default kernel is the code it was.  In that translation unit the host side is left out and the other kernels, with internal linkage and unused, are dropped.
// ... and dgn_rows.hip with FG_RESIDENT_ROWS_TU, for dgn_resident_rows_kernel: the instance that also stores every node's h_4 row, in
// the caller's node order (flowgnn_set_node_embeddings).  That one tests the embeddings pointer at run time, to serve both at once.
// what a launch of the resident kernel takes, the ONE type of the three translation units: the kernel's DgnResidentArgs (below) adds nothing
struct DgnResidentLaunch {
    const uint32_t* rec;      // [n_tot + 128][12] (dgn_tile_build_kernel<true>)
    const float* table;       // [173][100]
    const uint8_t* wpk;       // 4 x DGN_FT_LAYER_BYTES (dgn_pack_fused_layer)
    const int* tile_row;      // GraphTiles::row_start, or bp_row (the tile's first row in the record space)
    const int* tile_graph;    // GraphTiles::graph_start, or bp_graph
    const int* list;          // GraphTiles::bp_list (tile t = the graphs list[tile_graph[t]] ..), or null (tile t = graphs tile_graph[t] ..)
    BatchView b;              // node counts for the readout; the edge list for rows with duplicate in-edges
    const float* head;        // DGN_HEAD_BYTES: w1 [100][50] and w2 [50][25] transposed ([in][out]: unit along the lanes), b1, b2, w3, b3
    float* out;               // [G]
    float* emb;               // [G][100]: the pooled rows the head reads (flowgnn_set_embeddings), or null
    int* range_flag;
    int n_tiles;
    float* node_emb;          // [N][100]: every node's h_4 row in the caller's node order (flowgnn_set_node_embeddings;
                              // dgn_resident_rows_kernel stores them), or null.  Last: the other members keep their places
};
void launch_dgn_resident_default(const DgnResidentLaunch& a, int grid, hipStream_t s);  // dgn.hip
void launch_dgn_resident_emb(const DgnResidentLaunch& a, int grid, hipStream_t s);      // dgn_emb.hip
void launch_dgn_resident_rows(const DgnResidentLaunch& a, int grid, hipStream_t s);     // dgn_rows.hip
// Single-product instances (FLOWGNN_NUMERIC_F16): dgn_f16.hip, dgn_emb_f16.hip and dgn_rows_f16.hip compile this
// file once more with DGN_SINGLE_PRODUCT = 1 -- dgn_resident_kernel and dgn_layer_mfma_kernel under names of their own, every operand of
// the matrix-pipe products (transposed source rows, directional weights, a1 / a2, the scaled update weights) ONE f16 value, rounded to
// nearest even, and every product ONE f16 MFMA (fp32 accumulate).  wpk is then the hi-halves-only stream (7 KiB per K-step, bias block
// behind it).  Host side and the other kernels exist in this file's own translation unit only.
#ifndef DGN_SINGLE_PRODUCT
#define DGN_SINGLE_PRODUCT 0
#endif
void launch_dgn_resident_f16_default(const DgnResidentLaunch& a, int grid, hipStream_t s);  // dgn_f16.hip
void launch_dgn_resident_f16_emb(const DgnResidentLaunch& a, int grid, hipStream_t s);      // dgn_emb_f16.hip
void launch_dgn_resident_f16_rows(const DgnResidentLaunch& a, int grid, hipStream_t s);     // dgn_rows_f16.hip
// the per-layer matrix-pipe kernel's single-product instances (dgn_f16.hip): dgn_layer_mfma_kernel<info, pool>'s arguments; (info, pool) is
// one of (1, false), (2, false), (2, true)
struct DgnLayerMfmaLaunch {
    const float* h; float* hout;
    const int *row_ptr, *src, *out_deg;
    const float* eig4;
    const uint8_t* wpk;
    const int* tile_row;
    int n_tiles;
    int* range_flag;
    int ablate;
    uint32_t* rowinfo;
    const int2* ginfo;
    float* pool_part;
    int* pool_cnt;
};
void launch_dgn_layer_mfma_f16(const DgnLayerMfmaLaunch& a, int info, bool pool, int grid, hipStream_t s);
#if defined(FG_RESIDENT_EMB_TU) || defined(FG_RESIDENT_ROWS_TU) || DGN_SINGLE_PRODUCT
#define FG_RESIDENT_KERNEL_TU 1
namespace {
#endif
constexpr bool DGN_F16 = DGN_SINGLE_PRODUCT != 0;
#ifdef FG_RESIDENT_EMB_TU
constexpr bool RESIDENT_EMB = true;
#else
constexpr bool RESIDENT_EMB = false;
#endif
#ifdef FG_RESIDENT_ROWS_TU
constexpr bool RESIDENT_ROWS = true;
#else
constexpr bool RESIDENT_ROWS = false;
#endif

constexpr int DGN_D = 100;
constexpr int DGN_L = 4;
constexpr int DGN_C = DGN_D / 4;
constexpr int DGN_OT = 7;
constexpr int DGN_TBL = 119;


// z[v] = [a1 | a2]: policy of the generic tiled aggregation (device_common.h).  The directional weight of an edge
// is eig1[u] - eig1[v]: the source half is staged per CSR entry, the destination half is read once per item.
struct DgnAggPolicy {
    static constexpr int D = DGN_D, TR = 128, NTHR = 512, TE = 20 * 128, TABLE_ROWS = 0;
    static constexpr bool HAS_SCALAR = true;
    static constexpr int NDST = 2, CONST_FLOATS = 0;  // eig1[v], outdeg(v)
    struct Params {
        const float* eig;     // [N][4]
        const int* out_deg;
        const float* esc;     // [E] eig1[src_e] in CSR order (edge_scalar_kernel)
    };
    struct Acc { float4 m1, m2; float wsum, abssum; };
    __device__ static float src_scalar(const Params& p, int u) { return p.eig[(size_t)u * 4 + 1]; }
    __device__ static void dst_stage(const Params& p, int v, float* o) {
        o[0] = p.eig[(size_t)v * 4 + 1];
        o[1] = (float)p.out_deg[v];
    }
    __device__ static const float* const_ptr(const Params&) { return nullptr; }
    __device__ static void init(Acc& a) {
        a.m1 = make_float4(0.f, 0.f, 0.f, 0.f);
        a.m2 = a.m1;
        a.wsum = 0.f;
        a.abssum = 0.f;
    }
    __device__ static void edge(Acc& a, const float4& x, const float4&, float ss, const float* sd) {
        const float w = ss - sd[0];
        a.wsum += w;
        a.abssum += fabsf(w);
        a.m1.x += x.x; a.m1.y += x.y; a.m1.z += x.z; a.m1.w += x.w;
        a.m2.x += x.x * w; a.m2.y += x.y * w; a.m2.z += x.z * w; a.m2.w += x.w * w;
    }
    __device__ static void finish(const Params&, const Acc& a, const float4& hv, int v, int c, int, const float* sd, const float*,
                                  float* out) {
        const float abssum = a.abssum == 0.0f ? 1.0f / 8192.0f : a.abssum;  // epsilon of ap_fixed<16,3>
        const float deg = sd[1];
        const bool dv = deg == 0.0f;
        float4 a1, a2;
        a1.x = dv ? 0.f : a.m1.x / deg; a1.y = dv ? 0.f : a.m1.y / deg;
        a1.z = dv ? 0.f : a.m1.z / deg; a1.w = dv ? 0.f : a.m1.w / deg;
        a2.x = fabsf((a.m2.x - a.wsum * hv.x) / abssum); a2.y = fabsf((a.m2.y - a.wsum * hv.y) / abssum);
        a2.z = fabsf((a.m2.z - a.wsum * hv.z) / abssum); a2.w = fabsf((a.m2.w - a.wsum * hv.w) / abssum);
        float4* o = reinterpret_cast<float4*>(out) + (size_t)v * (2 * DGN_C) + c;
        stream_store4(o, a1);
        stream_store4(o + DGN_C, a2);
    }
};

// h'[v] = h[v] + relu(b + W0 a1 + W1 a2), K = 2 x 100.  One wave = 16 nodes; fragments [2][7][6][64][4] + tails [2][7][64]
__global__ __launch_bounds__(256) void dgn_dense_kernel(const float* __restrict__ z, const float* __restrict__ h,
                                                         float* __restrict__ hout, const float* __restrict__ wf,
                                                         const float* __restrict__ wtail, const float* __restrict__ biasp,
                                                         int n_tot) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const long long node_base = (long long)wave * 16;
    if (node_base >= n_tot) return;
    long long node = node_base + j;
    const bool valid = node < n_tot;
    if (!valid) node = n_tot - 1;
    float bq[2][25];
#pragma unroll
    for (int b = 0; b < 2; b++) {
        const float* row = z + ((size_t)node * 2 + b) * DGN_D;
#pragma unroll
        for (int q = 0; q < 6; q++) {
            const float4 x = *reinterpret_cast<const float4*>(row + 16 * q + 4 * g);
            bq[b][4 * q + 0] = x.x; bq[b][4 * q + 1] = x.y; bq[b][4 * q + 2] = x.z; bq[b][4 * q + 3] = x.w;
        }
        bq[b][24] = row[96 + g];
    }
    const float4* wf4 = reinterpret_cast<const float4*>(wf);
#pragma unroll 1
    for (int t = 0; t < DGN_OT; t++) {
        const float4 bb = *reinterpret_cast<const float4*>(biasp + 16 * t + 4 * g);
        float4_t y0 = (float4_t){bb.x, bb.y, bb.z, bb.w}, y1 = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 2; b++) {
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const float4 af = wf4[(((size_t)b * DGN_OT + t) * 6 + q) * 64 + lane];
                y0 = __builtin_amdgcn_mfma_f32_16x16x4f32(af.x, bq[b][4 * q + 0], y0, 0, 0, 0);
                y1 = __builtin_amdgcn_mfma_f32_16x16x4f32(af.y, bq[b][4 * q + 1], y1, 0, 0, 0);
                y0 = __builtin_amdgcn_mfma_f32_16x16x4f32(af.z, bq[b][4 * q + 2], y0, 0, 0, 0);
                y1 = __builtin_amdgcn_mfma_f32_16x16x4f32(af.w, bq[b][4 * q + 3], y1, 0, 0, 0);
            }
            const float at = wtail[((size_t)b * DGN_OT + t) * 64 + lane];
            y0 = __builtin_amdgcn_mfma_f32_16x16x4f32(at, bq[b][24], y0, 0, 0, 0);
        }
        const int col = 16 * t + 4 * g;
        if (valid && col < DGN_D) {
            const size_t off = (size_t)node * DGN_D + col;
            const float4 hv = *reinterpret_cast<const float4*>(h + off);
            *reinterpret_cast<float4*>(hout + off) = make_float4(hv.x + relu1(y0.x + y1.x), hv.y + relu1(y0.y + y1.y),
                                                                 hv.z + relu1(y0.z + y1.z), hv.w + relu1(y0.w + y1.w));
        }
    }
}

// ---------------------------------------------------------------- fused layer: aggregation + dense update in one kernel
// Neither the aggregates z = [a1 | a2] (800 B per node) nor any weight chunk ever crosses a barrier here.  The contraction index
// is re-ordered FEATURE-major: K-step k (of 7) covers a1 and a2 of features 16k .. 16k+15, lane (j, g) supplying the two
// quadruples of features 16k + 4g .. +3 of node j (K-slot e: feature 16k + 4g + (e & 3), a1 for e < 4, a2 for e >= 4) -- one
// 16-byte read per in-edge and eight accumulators per K-step, then the step's 21 MFMAs.  The layer's split weights in that
// order are 98 KiB: they stay in LDS for the whole kernel, so inside a tile the eight waves of the (persistent, one per CU)
// workgroup never meet a barrier and drift against each other -- one wave's gather (VALU / LDS) runs under another's MFMAs.
// Tiles are WHOLE graphs (GraphTiles: <= 128 rows, <= 2 560 in-edges): the tile's rows of h, its CSR slice (bytes) and its
// eigenvector column live in LDS; the next tile's are fetched into registers while this one is computed and written to LDS
// between the two barriers that end a tile.  In-edges are summed in CSR order; the directional weights eig1[u] - eig1[v] of a
// row's first 16 in-edges are kept in registers.
constexpr int DGN_FT_ROWS = 128;
constexpr int DGN_FT_EDGES = 2560;
constexpr int DGN_FT_KS = 7;
constexpr int DGN_FT_WBYTES = DGN_FT_KS * DGN_OT * 2 * 1024;  // 100 352: [k][t][hi, lo] fragments
constexpr int DGN_FT_BIAS = DGN_FT_WBYTES;                     // then bias[112] (pre-scaled) and 1 / scale
constexpr size_t DGN_FT_LAYER_BYTES = DGN_FT_WBYTES + 512;
// what the matrix-pipe kernels (dgn_layer_mfma_kernel, dgn_resident_kernel) read: the same, or (single product) the hi fragments alone,
// [k][t] x 1 KiB, with the same bias block and 1 / scale behind them
constexpr int DGN_FRAGS = DGN_F16 ? 1 : 2;  // fragments per output tile and K-step: hi and lo, or hi alone
constexpr int DGN_MP_WBYTES = DGN_FT_KS * DGN_OT * DGN_FRAGS * 1024;
constexpr int DGN_MP_BIAS = DGN_MP_WBYTES;
constexpr size_t DGN_MP_LAYER_BYTES = DGN_MP_WBYTES + 512;
constexpr size_t DGN_F16_LAYER_BYTES = (size_t)DGN_FT_KS * DGN_OT * 1024 + 512;  // the single-product stream of a layer: 50 176 + 512 B

// an operand pair of a matrix-pipe product: split (hi + lo) or, single product, the pair rounded to f16 once, to nearest even (LO is left alone)
typedef _Float16 dgn_half2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t dgn_pack_rne(float a, float b) { return __builtin_bit_cast(uint32_t, (dgn_half2_t){(_Float16)a, (_Float16)b}); }
#define DGN_OPER2(a, b, HI, LO)                                   \
    do {                                                          \
        if constexpr (DGN_F16) { (HI) = dgn_pack_rne((a), (b)); } \
        else { DS_SPLIT2(a, b, HI, LO); }                         \
    } while (0)

__global__ __launch_bounds__(512, 2) void dgn_layer_fused_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                  const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                  const int* __restrict__ out_deg, const float* __restrict__ eig4,
                                                                  const uint8_t* __restrict__ wpk, const int* __restrict__ tile_row,
                                                                  int n_tiles, int* __restrict__ range_flag, int ablate_arg) {
    const int ablate = FG_ABLATE(ablate_arg);  // 0 in the shipped build: the branches below fold away (common.h)
    (void)ablate_arg;
    // one LDS object with the row tile at offset 0: a neighbour row's byte address (row * 400 + 16 g < 2^16) then packs two to a
    // register and the K-step's column is the ds_read's immediate offset -- no address arithmetic inside the seven walks
    constexpr int OFF_W = DGN_FT_ROWS * DGN_D * 4, OFF_SRC = OFF_W + (int)DGN_FT_LAYER_BYTES, OFF_RP = OFF_SRC + DGN_FT_EDGES,
                  OFF_EIG = OFF_RP + 2 * (DGN_FT_ROWS + 4), LDS_TOTAL = OFF_EIG + 4 * DGN_FT_ROWS;
    static_assert(OFF_W % 16 == 0 && OFF_SRC % 16 == 0 && OFF_RP % 4 == 0 && OFF_EIG % 4 == 0, "alignment");
    __shared__ __attribute__((aligned(16))) char s_all[LDS_TOTAL];
    float* s_h = reinterpret_cast<float*>(s_all);
    char* s_w = s_all + OFF_W;
    uint8_t* s_src = reinterpret_cast<uint8_t*>(s_all + OFF_SRC);
    uint16_t* s_rp = reinterpret_cast<uint16_t*>(s_all + OFF_RP);
    float* s_eig = reinterpret_cast<float*>(s_all + OFF_EIG);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    int tile = blockIdx.x;
    if (tile >= n_tiles) return;
    // the layer's weights: once per workgroup
    for (int i = tid; i < (int)(DGN_FT_LAYER_BYTES / 16); i += 512)
        reinterpret_cast<uint4*>(s_w)[i] = reinterpret_cast<const uint4*>(wpk)[i];
    // first tile straight into LDS
    int t0 = tile_row[tile], rows = tile_row[tile + 1] - t0;
    if (rows > DGN_FT_ROWS) rows = DGN_FT_ROWS;
    int e0 = row_ptr[t0], ne = row_ptr[t0 + rows] - e0;
    if (ne > DGN_FT_EDGES) ne = DGN_FT_EDGES;  // cannot happen for a validated batch (the host packed by edge count)
    for (int i = tid; i < rows * (DGN_D / 4); i += 512) reinterpret_cast<float4*>(s_h)[i] = reinterpret_cast<const float4*>(h + (size_t)t0 * DGN_D)[i];
    for (int i = tid; i < ne; i += 512) s_src[i] = (uint8_t)((src[e0 + i] - t0) & 127);
    if (tid <= rows) { const int o = row_ptr[t0 + tid] - e0; s_rp[tid] = (uint16_t)(o < 0 ? 0 : (o > ne ? ne : o)); }
    if (tid < rows) s_eig[tid] = eig4[(size_t)(t0 + tid) * 4 + 1];
    __syncthreads();
    const float oscale = *reinterpret_cast<const float*>(s_w + DGN_FT_BIAS + 112 * 4);
    float vmax = 0.0f;
    while (true) {
        const int ntile = tile + gridDim.x;
        const bool has_next = ntile < n_tiles;
        // ---- the next tile: requested now into registers (rows: 7 float4 per thread), written to LDS after this tile's work
        // (unconditional loads from clamped addresses: a conditionally filled array would be kept in scratch memory, and the
        // store to it would wait for the loads right here)
        int nt0 = t0, nrows = rows, ne0 = e0, nne = ne;
        if (has_next) {
            nt0 = tile_row[ntile];
            nrows = tile_row[ntile + 1] - nt0;
            if (nrows > DGN_FT_ROWS) nrows = DGN_FT_ROWS;
            ne0 = row_ptr[nt0];
            nne = row_ptr[nt0 + nrows] - ne0;
            if (nne > DGN_FT_EDGES) nne = DGN_FT_EDGES;
        }
        const float4* nb = reinterpret_cast<const float4*>(h + (size_t)nt0 * DGN_D);
        const int last = nrows * (DGN_D / 4) - 1, elast = nne > 0 ? nne - 1 : 0;
#define DGN_NXI(P) ((tid + 512 * (P)) < last ? (tid + 512 * (P)) : last)
#define DGN_NXE(P) (nne > 0 ? src[ne0 + ((tid + 512 * (P)) < elast ? (tid + 512 * (P)) : elast)] : 0)
        // named scalars, not arrays: hipcc keeps a seven-element float4 array that is filled here and consumed at the loop's end
        // in scratch memory, and its store would wait for the loads on the spot
        const float4 nr0 = nb[DGN_NXI(0)], nr1 = nb[DGN_NXI(1)], nr2 = nb[DGN_NXI(2)], nr3 = nb[DGN_NXI(3)], nr4 = nb[DGN_NXI(4)],
                     nr5 = nb[DGN_NXI(5)], nr6 = nb[DGN_NXI(6)];
        const int ns0 = DGN_NXE(0), ns1 = DGN_NXE(1), ns2 = DGN_NXE(2), ns3 = DGN_NXE(3), ns4 = DGN_NXE(4);
#undef DGN_NXI
#undef DGN_NXE
        const int nx_rp = row_ptr[nt0 + (tid <= nrows ? tid : nrows)];
        const float nx_eig = eig4[(size_t)(nt0 + (tid < nrows ? tid : 0)) * 4 + 1];
        // ---- this wave's 16 rows
        const int r = wave * 16 + j;
        const bool valid = r < rows;
        const int e_base = valid ? (int)s_rp[r] : 0;
        int indeg = valid ? (int)s_rp[r + 1] - e_base : 0;
        if (ablate & 1) indeg = 0;  // development aid (dgn_ablate, -DFLOWGNN_DEV builds): timing without the gather
        const float eig_v = s_eig[valid ? r : 0];
        const long long node = (long long)t0 + (valid ? r : 0);
        const int odeg = out_deg[node];
        // first 16 in-edges: source rows as bytes, directional weights in registers; wsum / abssum over ALL in-edges
        // (DGN/src/load_inputs.cc:105-110)
        uint32_t adr[8];  // byte addresses (row * 400 + 16 g) of the first 16 source rows, two per register
        float ew[16];
        float wsum = 0.0f, abssum = 0.0f;
#pragma unroll
        for (int w = 0; w < 8; w++) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const int e = 2 * w + b;
                const int u = e < indeg ? (int)s_src[e_base + e] : 0;
                v |= (uint32_t)(u * (DGN_D * 4) + 16 * g) << (16 * b);
                const float we = e < indeg ? s_eig[u] - eig_v : 0.0f;
                ew[e] = we;
                wsum += we;
                abssum += fabsf(we);
            }
            adr[w] = v;
        }
        for (int e = 16; __any(e < indeg); e++)
            if (e < indeg) { const float we = s_eig[s_src[e_base + e]] - eig_v; wsum += we; abssum += fabsf(we); }
        const float inv_abs = 1.0f / (abssum == 0.0f ? 1.0f / 8192.0f : abssum);  // epsilon of ap_fixed<16,3> (node_embedding.cc:125-128)
        // a1 = m1 / outdeg with x / 0 = 0: one reciprocal per row and tile instead of four IEEE divisions (~40 dependent instructions)
        // per K-step; the row's arithmetic does not depend on its tile mates either way
        const float inv_dg = odeg == 0 ? 0.0f : 1.0f / (float)odeg;
        float4_t acc[DGN_OT];
#pragma unroll
        for (int t = 0; t < DGN_OT; t++) {
            const float4 bv = *reinterpret_cast<const float4*>(s_w + DGN_FT_BIAS + (16 * t + 4 * g) * 4);
            acc[t] = (float4_t){bv.x, bv.y, bv.z, bv.w};
        }
        const float* hrow = s_h + (valid ? r : 0) * DGN_D;
#pragma unroll
        for (int k = 0; k < DGN_FT_KS; k++) {
            if (ablate & 2) break;
            // K-step k: features 16k + 4g .. +3 (k = 6: only g = 0 holds real features, 96..99; the others supply zeros)
            // (k = 6: the address of lane group g > 0 points 16 g bytes past features 96..99 -- inside the next row or the weights;
            //  the values are discarded below)
            const bool real = k < 6 || g == 0;
            const int col = real ? 16 * k + 4 * g : 0;
            const char* hk = s_all + 64 * k;
            float4 m1 = make_float4(0.f, 0.f, 0.f, 0.f), m2 = m1;
#pragma unroll
            for (int w = 0; w < 4; w += 2) {
                if (__all(indeg >= 4 * w + 8)) {
                    // every row of the wave has these eight in-edges (kNN graphs): eight reads in flight, no masks.  The walk is bound by
                    // LDS round trips, not by instructions: two waves per SIMD hide little, so the reads are batched as deep as registers allow
                    float4 x[8];
#pragma unroll
                    for (int b = 0; b < 8; b++) x[b] = *reinterpret_cast<const float4*>(hk + ((adr[2 * w + (b >> 1)] >> (16 * (b & 1))) & 0xFFFFu));
#pragma unroll
                    for (int b = 0; b < 8; b++) {
                        const float we = ew[4 * w + b];
                        m1.x += x[b].x; m1.y += x[b].y; m1.z += x[b].z; m1.w += x[b].w;
                        m2.x = __builtin_fmaf(x[b].x, we, m2.x); m2.y = __builtin_fmaf(x[b].y, we, m2.y); m2.z = __builtin_fmaf(x[b].z, we, m2.z); m2.w = __builtin_fmaf(x[b].w, we, m2.w);
                    }
                } else if (__any(indeg > 4 * w)) {
#pragma unroll
                    for (int b = 0; b < 8; b++)
                        if (indeg > 4 * w + b) {
                            const float4 x = *reinterpret_cast<const float4*>(hk + ((adr[2 * w + (b >> 1)] >> (16 * (b & 1))) & 0xFFFFu));
                            const float we = ew[4 * w + b];
                            m1.x += x.x; m1.y += x.y; m1.z += x.z; m1.w += x.w;
                            m2.x = __builtin_fmaf(x.x, we, m2.x); m2.y = __builtin_fmaf(x.y, we, m2.y); m2.z = __builtin_fmaf(x.z, we, m2.z); m2.w = __builtin_fmaf(x.w, we, m2.w);
                        }
                }
            }
            for (int e = 16; __any(e < indeg); e++)  // rows with more than 16 in-edges: the rest from the LDS copies
                if (e < indeg) {
                    const int u = s_src[e_base + e];
                    const float we = s_eig[u] - eig_v;
                    const float4 x = *reinterpret_cast<const float4*>(s_h + u * DGN_D + col);
                    m1.x += x.x; m1.y += x.y; m1.z += x.z; m1.w += x.w;
                    m2.x = __builtin_fmaf(x.x, we, m2.x); m2.y = __builtin_fmaf(x.y, we, m2.y); m2.z = __builtin_fmaf(x.z, we, m2.z); m2.w = __builtin_fmaf(x.w, we, m2.w);
                }
            // a1 = m1 / outdeg (x / 0 = 0), a2 = |(m2 - wsum h[v]) / abssum|   (node_embedding.cc:143-146)
            const float4 hv = *reinterpret_cast<const float4*>(hrow + col);
            float4 a1, a2;
            a1.x = m1.x * inv_dg; a1.y = m1.y * inv_dg; a1.z = m1.z * inv_dg; a1.w = m1.w * inv_dg;
            // explicit fma: every path a wave can take (all rows full / ragged) rounds alike, so a row's result never depends on its tile mates
            a2.x = fabsf(__builtin_fmaf(-wsum, hv.x, m2.x) * inv_abs); a2.y = fabsf(__builtin_fmaf(-wsum, hv.y, m2.y) * inv_abs);
            a2.z = fabsf(__builtin_fmaf(-wsum, hv.z, m2.z) * inv_abs); a2.w = fabsf(__builtin_fmaf(-wsum, hv.w, m2.w) * inv_abs);
            if (!real) { a1 = make_float4(0.f, 0.f, 0.f, 0.f); a2 = a1; }
            ds_uint4_t b_hi, b_lo;
            DS_SPLIT2(a1.x, a1.y, b_hi.x, b_lo.x);
            DS_SPLIT2(a1.z, a1.w, b_hi.y, b_lo.y);
            DS_SPLIT2(a2.x, a2.y, b_hi.z, b_lo.z);
            DS_SPLIT2(a2.z, a2.w, b_hi.w, b_lo.w);
            asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(vmax) : "v"(a1.x), "v"(a1.y));
            asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(vmax) : "v"(a1.z), "v"(a1.w));
            asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(vmax) : "v"(a2.x), "v"(a2.y));
            asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(vmax) : "v"(a2.z), "v"(a2.w));
            asm volatile("" : "+v"(vmax));
            const char* wb = s_w + (size_t)k * (DGN_OT * 2 * 1024);
#pragma unroll
            for (int t0_ = 0; t0_ < DGN_OT; t0_ += 2) {  // pairs of output tiles, product-major: no MFMA waits for its predecessor
                const int n = t0_ + 1 < DGN_OT ? 2 : 1;
                ds_uint4_t f[4];
#pragma unroll
                for (int i = 0; i < 2 * n; i++) f[i] = *reinterpret_cast<const ds_uint4_t*>(wb + ((t0_ * 2) + i) * 1024 + lane * 16);
#pragma unroll
                for (int i = 0; i < n; i++) acc[t0_ + i] = DS_MFMA16(f[2 * i], b_hi, acc[t0_ + i]);
#pragma unroll
                for (int i = 0; i < n; i++) acc[t0_ + i] = DS_MFMA16(f[2 * i], b_lo, acc[t0_ + i]);
#pragma unroll
                for (int i = 0; i < n; i++) acc[t0_ + i] = DS_MFMA16(f[2 * i + 1], b_hi, acc[t0_ + i]);
            }
        }
        // ---- epilogue: h' = h + relu(b + W0 a1 + W1 a2)   (node_embedding.cc:176-181)
        if (valid) {
#pragma unroll
            for (int t = 0; t < DGN_OT; t++) {
                const int c = 16 * t + 4 * g;
                if (c < DGN_D) {
                    const float4 hv = *reinterpret_cast<const float4*>(hrow + c);
                    const float4_t rr = acc[t] * oscale;
                    *reinterpret_cast<float4*>(hout + (size_t)node * DGN_D + c) =
                        make_float4(hv.x + relu1(rr.x), hv.y + relu1(rr.y), hv.z + relu1(rr.z), hv.w + relu1(rr.w));
                }
            }
        }
        if (!has_next) break;
        __syncthreads();  // every wave is done with this tile's rows, CSR slice and eigenvector column
#define DGN_PUT(P, V) if (tid + 512 * (P) < nrows * (DGN_D / 4)) reinterpret_cast<float4*>(s_h)[tid + 512 * (P)] = V;
        DGN_PUT(0, nr0) DGN_PUT(1, nr1) DGN_PUT(2, nr2) DGN_PUT(3, nr3) DGN_PUT(4, nr4) DGN_PUT(5, nr5) DGN_PUT(6, nr6)
#undef DGN_PUT
#define DGN_PUTE(P, V) if (tid + 512 * (P) < nne) s_src[tid + 512 * (P)] = (uint8_t)(((V) - nt0) & 127);
        DGN_PUTE(0, ns0) DGN_PUTE(1, ns1) DGN_PUTE(2, ns2) DGN_PUTE(3, ns3) DGN_PUTE(4, ns4)
#undef DGN_PUTE
        if (tid <= nrows) { const int o = nx_rp - ne0; s_rp[tid] = (uint16_t)(o < 0 ? 0 : (o > nne ? nne : o)); }
        if (tid < nrows) s_eig[tid] = nx_eig;
        __syncthreads();
        tile = ntile; t0 = nt0; rows = nrows; e0 = ne0; ne = nne;
    }
    if (__any(!(vmax < 6.0e4f))) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

// ---------------------------------------------------------------- fused layer, aggregation on the MATRIX pipe (kNN-dense tiles)
// In dgn_layer_fused_kernel a K-step's operand is a walk over the row's in-edges: 16 LDS reads + 128 VALU instructions per lane,
// seven times per tile -- the walk, not the 21 MFMAs behind it, is where the layer's time goes (wait share 0.61, MFMA busy 14 %).
// Both aggregates are LINEAR in h, and a tile of whole graphs is a block-diagonal adjacency matrix A (v, u) of 0 / 1 entries:
//     m1[v] = sum_u A[v][u] h[u]                     m2[v] = sum_u A[v][u] (eig[u] - eig[v]) h[u]      (DGN/src/message_passing.cc:148-149)
// so for K-step k (features 16k .. 16k+15) the two aggregates of the wave's 16 rows are  H^T[16 features][128 sources] x B[128][16]
// -- MFMAs with the TRANSPOSED, f16-split rows of the tile as the A operand (s_ht: [feature][source] hi and lo, built by the tile
// loader) and, as the B operand, the row's adjacency: lane (j, g) holds its row's entries for sources 32 s + 8 g .. + 7 of the four
// 32-source blocks s as f16 -- ones (exact: m1 = two products, H_hi A + H_lo A) and the row's WEIGHTS w = eig[u] - eig[v], formed in
// fp32 as the reference forms them, scaled by the power of two that brings sum |w| into [1, 2) and split hi / lo (m2 = three
// products).  The operands are built ONCE per tile from a 32-bit mask per lane (the row's sources that fall into this lane's slots)
// and 32 differences: ~260 VALU instructions per tile instead of 896 for the seven walks; source blocks that are empty for the whole
// wave are skipped (block diagonal: a 16-row group sees two or three of the four).  The result lands in the lanes that need it:
// D[feature 4g + r][v_j] -> lane (j, g).
// Order of summation differs from the CSR order of the walk (and depends on where the graph sits in its tile), so this path is
// toleranced, not bit-identical under batch splits (tests/test_dgn_gpu.py says so); duplicate edges (multiplicity > 1: not a 0 / 1
// matrix) are added by a correction walk over just those edges.  h[v] (self term, residual) is read from HBM / L2, not from LDS:
// the fp32 rows are not kept on chip.
constexpr int DGN_HT_STRIDE = 136;                           // f16 per feature row of s_ht (128 sources + 8: 68 banks, conflict-free)
constexpr int DGN_HT_BYTES = DGN_D * DGN_HT_STRIDE * 2;      // 27 200 per half (hi | lo)
constexpr int DGN_REC_DW = 12;  // words of a row's record for dgn_resident_kernel: [0..3] mask per lane group, wsum, abssum, ndup, outdeg, eig1, 9 table rows as bytes

// INFO: what a row's in-edge pass produces -- this lane's adjacency mask, wsum, abssum, the duplicate count -- depends on the graph and
// the eigenvector only, not on the layer: the first layer's launch (INFO 1) stores it, 32 B per row, the later ones (INFO 2) load it
// (requested a tile ahead) instead of walking the row's in-edges again (0.10-0.12 ms per launch).  INFO 0: neither.
// POOL (the last layer when nothing asks for its rows): h' does not leave the kernel.  Every wave sums its 16 rows per graph (fixed
// DPP butterfly over the 16 lanes that share a feature slice) and writes one partial row per (graph, wave): pool_part[graph][rel][100],
// rel = the wave's index counted from the graph's first one (a graph of <= 128 rows spans <= 8 waves); the graph's first wave also
// writes how many there are.  dgn_pool_part_mlp3_kernel adds them in order and runs the head: the 400 B per node of h' are neither
// written nor read back (2 x 0.64 GB per step at 2^15 hep10k graphs).  The association depends on where the graph sits in its tile
// -- toleranced like the rest of this path.  ginfo[node] = (graph, (node - first) | (end - node) << 8), dgn_graph_info_kernel.
template <int INFO, bool POOL>
__global__ __launch_bounds__(512, 2) void dgn_layer_mfma_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                 const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                 const int* __restrict__ out_deg, const float* __restrict__ eig4,
                                                                 const uint8_t* __restrict__ wpk, const int* __restrict__ tile_row,
                                                                 int n_tiles, int* __restrict__ range_flag, int ablate_arg,
                                                                 uint32_t* __restrict__ rowinfo /* [n_tot][8] */,
                                                                 const int2* __restrict__ ginfo, float* __restrict__ pool_part,
                                                                 int* __restrict__ pool_cnt) {
    const int ablate = FG_ABLATE(ablate_arg);  // development aid (dgn_ablate, -DFLOWGNN_DEV builds): 1 no aggregation MFMAs, 2 no dense
    (void)ablate_arg;                          // MFMAs, 4 no transposing stores of the next tile, 8 no in-edge pass, 16 no h[v] loads
    constexpr int OFF_W = (DGN_F16 ? 1 : 2) * DGN_HT_BYTES, OFF_SRC = OFF_W + (int)DGN_MP_LAYER_BYTES, OFF_RP = OFF_SRC + DGN_FT_EDGES,  // (single product: one s_ht half)
                  OFF_EIG = OFF_RP + 2 * (DGN_FT_ROWS + 8), LDS_TOTAL = OFF_EIG + 4 * DGN_FT_ROWS;
    static_assert(OFF_W % 16 == 0 && OFF_SRC % 16 == 0 && OFF_RP % 4 == 0 && OFF_EIG % 16 == 0, "alignment");
    __shared__ __attribute__((aligned(16))) char s_all[LDS_TOTAL];
    uint16_t* s_ht_hi = reinterpret_cast<uint16_t*>(s_all);
    uint16_t* s_ht_lo = reinterpret_cast<uint16_t*>(s_all + DGN_HT_BYTES);
    char* s_w = s_all + OFF_W;
    uint8_t* s_src = reinterpret_cast<uint8_t*>(s_all + OFF_SRC);
    uint16_t* s_rp = reinterpret_cast<uint16_t*>(s_all + OFF_RP);
    float* s_eig = reinterpret_cast<float*>(s_all + OFF_EIG);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    int tile = blockIdx.x;
    if (tile >= n_tiles) return;
    for (int i = tid; i < (int)(DGN_MP_LAYER_BYTES / 16); i += 512)
        reinterpret_cast<uint4*>(s_w)[i] = reinterpret_cast<const uint4*>(wpk)[i];
    // loader geometry: wave w owns rows 16 w .. 16 w + 15; its p-th load covers chunks 4 p .. 4 p + 3 of them -- lane = (row lane & 15,
    // chunk lane >> 4): a wave instruction reads sixteen 64-byte row segments (lanes along rows alone would touch 64 different lines
    // per instruction: measured +0.23 ms per layer), and the 2-byte stores of the transposition fall into 32 different banks
    const int lr = 16 * wave + (lane & 15), cg = lane >> 4;
    float hmax = 0.0f;  // single product: the largest |h| rounded into s_ht (joins vmax at the end: beyond 6e4 the range flag trips)
    auto put_row_piece = [&](int c, const float4& v, bool real) {
        if (c >= DGN_C) return;
        const float4 x = real ? v : make_float4(0.f, 0.f, 0.f, 0.f);  // rows beyond the tile's last: zeros (never NaN under a zero mask)
        if constexpr (DGN_F16) {  // one rounding to nearest even per feature, no lo half
            const uint32_t r01 = dgn_pack_rne(x.x, x.y), r23 = dgn_pack_rne(x.z, x.w);
            hmax = __builtin_fmaxf(__builtin_fmaxf(hmax, __builtin_fabsf(x.x)), __builtin_fabsf(x.y));
            hmax = __builtin_fmaxf(__builtin_fmaxf(hmax, __builtin_fabsf(x.z)), __builtin_fabsf(x.w));
            uint16_t* pr = s_ht_hi + (4 * c) * DGN_HT_STRIDE + lr;
            pr[0] = (uint16_t)r01; pr[DGN_HT_STRIDE] = (uint16_t)(r01 >> 16); pr[2 * DGN_HT_STRIDE] = (uint16_t)r23; pr[3 * DGN_HT_STRIDE] = (uint16_t)(r23 >> 16);
            return;
        }
        uint32_t h01, l01, h23, l23;
        DS_SPLIT2(x.x, x.y, h01, l01);
        DS_SPLIT2(x.z, x.w, h23, l23);
        uint16_t* ph = s_ht_hi + (4 * c) * DGN_HT_STRIDE + lr;
        uint16_t* pl = s_ht_lo + (4 * c) * DGN_HT_STRIDE + lr;
        ph[0] = (uint16_t)h01; ph[DGN_HT_STRIDE] = (uint16_t)(h01 >> 16); ph[2 * DGN_HT_STRIDE] = (uint16_t)h23; ph[3 * DGN_HT_STRIDE] = (uint16_t)(h23 >> 16);
        pl[0] = (uint16_t)l01; pl[DGN_HT_STRIDE] = (uint16_t)(l01 >> 16); pl[2 * DGN_HT_STRIDE] = (uint16_t)l23; pl[3 * DGN_HT_STRIDE] = (uint16_t)(l23 >> 16);
    };
    auto put_eig = [&](int r, float e, bool real) { s_eig[r] = real ? e : 0.0f; };
    int t0 = tile_row[tile], rows = tile_row[tile + 1] - t0;
    if (rows > DGN_FT_ROWS) rows = DGN_FT_ROWS;
    int e0 = row_ptr[t0], ne = row_ptr[t0 + rows] - e0;
    if (ne > DGN_FT_EDGES) ne = DGN_FT_EDGES;
    {
        const float4* hb = reinterpret_cast<const float4*>(h + (size_t)(t0 + (lr < rows ? lr : 0)) * DGN_D);
#pragma unroll
        for (int p = 0; p < 7; p++) {
            const int c = 4 * p + cg;
            put_row_piece(c, hb[c < DGN_C ? c : 0], lr < rows);
        }
    }
    constexpr bool STAGE_CSR = INFO != 2;  // INFO 2 never walks a row's in-edges (the rare duplicate edges: from global memory)
    if constexpr (STAGE_CSR) {
        for (int i = tid; i < ne; i += 512) s_src[i] = (uint8_t)((src[e0 + i] - t0) & 127);
        if (tid <= rows) { const int o = row_ptr[t0 + tid] - e0; s_rp[tid] = (uint16_t)(o < 0 ? 0 : (o > ne ? ne : o)); }
    }
    if (tid < DGN_FT_ROWS) put_eig(tid, eig4[(size_t)(t0 + (tid < rows ? tid : 0)) * 4 + 1], tid < rows);
    __syncthreads();
    const float oscale = *reinterpret_cast<const float*>(s_w + DGN_MP_BIAS + 112 * 4);
    float vmax = 0.0f;
    uint32_t cur_bits = 0;
    uint4 cur_info = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (INFO == 2) {  // the first tile's stored pass results (later tiles': requested a tile ahead, below)
        const int r1 = wave * 16 + j;
        const size_t n1 = (size_t)t0 + (r1 < rows ? r1 : 0);
        cur_bits = rowinfo[n1 * 8 + g];
        cur_info = *reinterpret_cast<const uint4*>(rowinfo + n1 * 8 + 4);
    }
    while (true) {
        const int ntile = tile + gridDim.x;
        const bool has_next = ntile < n_tiles;
        int nt0 = t0, nrows = rows, ne0 = e0, nne = ne;
        if (has_next) {
            nt0 = tile_row[ntile];
            nrows = tile_row[ntile + 1] - nt0;
            if (nrows > DGN_FT_ROWS) nrows = DGN_FT_ROWS;
            ne0 = row_ptr[nt0];
            nne = row_ptr[nt0 + nrows] - ne0;
            if (nne > DGN_FT_EDGES) nne = DGN_FT_EDGES;
        }
        // the next tile, requested now into registers (named scalars: an array filled here and consumed at the loop's end goes to scratch)
        const float4* nb = reinterpret_cast<const float4*>(h + (size_t)(nt0 + (lr < nrows ? lr : 0)) * DGN_D);
#define DGN_NC(P) ((4 * (P) + cg) < DGN_C ? (4 * (P) + cg) : 0)
        const float4 nr0 = nb[DGN_NC(0)], nr1 = nb[DGN_NC(1)], nr2 = nb[DGN_NC(2)], nr3 = nb[DGN_NC(3)], nr4 = nb[DGN_NC(4)], nr5 = nb[DGN_NC(5)],
                     nr6 = nb[DGN_NC(6)];
#undef DGN_NC
        const int elast = nne > 0 ? nne - 1 : 0;
#define DGN_NXE(P) ((STAGE_CSR && nne > 0) ? src[ne0 + ((tid + 512 * (P)) < elast ? (tid + 512 * (P)) : elast)] : 0)
        const int ns0 = DGN_NXE(0), ns1 = DGN_NXE(1), ns2 = DGN_NXE(2), ns3 = DGN_NXE(3), ns4 = DGN_NXE(4);
#undef DGN_NXE
        const int nx_rp = STAGE_CSR ? row_ptr[nt0 + (tid <= nrows ? tid : nrows)] : 0;
        const float nx_eig = eig4[(size_t)(nt0 + (tid < nrows ? tid : 0)) * 4 + 1];
        // ---- this wave's 16 rows
        const int r = wave * 16 + j;
        const bool valid = r < rows;
        uint32_t nx_bits = 0;
        uint4 nx_info = make_uint4(0u, 0u, 0u, 0u);
        if constexpr (INFO == 2) {  // the stored pass results of this lane's row in the NEXT tile
            const size_t nn = (size_t)nt0 + (r < nrows ? r : 0);
            nx_bits = rowinfo[nn * 8 + g];
            nx_info = *reinterpret_cast<const uint4*>(rowinfo + nn * 8 + 4);
        }
        const int e_base = (STAGE_CSR && valid) ? (int)s_rp[r] : 0;
        const int indeg = (STAGE_CSR && valid && !(ablate & 8)) ? (int)s_rp[r + 1] - e_base : 0;
        const float eig_v = s_eig[valid ? r : 0];
        const long long node = (long long)t0 + (valid ? r : 0);
        int odeg;
        if constexpr (INFO == 2) odeg = (int)cur_info.w;  // (a row past the tile's end carries row 0's record, as out_deg[node] read row 0's)
        else odeg = out_deg[node];
        int2 gi = make_int2(0, 0);
        if constexpr (POOL) gi = ginfo[node];  // requested here, used in the epilogue
        // one pass over the row's in-edges: wsum, abssum (DGN/src/load_inputs.cc:105-110), this lane's slice of the adjacency row as a
        // bit mask (bit 8 s + e <-> source 32 s + 8 g + e), and the number of duplicate edges (CSR rows are sorted by source)
        float wsum = 0.0f, abssum = 0.0f;
        uint32_t bits = 0;
        int ndup = 0;
        if constexpr (INFO == 2) {
            bits = valid ? cur_bits : 0u;
            wsum = valid ? __builtin_bit_cast(float, cur_info.x) : 0.0f;
            abssum = valid ? __builtin_bit_cast(float, cur_info.y) : 0.0f;
            ndup = valid ? (int)cur_info.z : 0;
        } else {
            // the first 16 in-edges (kNN rows have exactly 16) as two batches of independent LDS reads -- source bytes, then their
            // eigenvector entries: two round trips instead of 32 dependent ones
            int us[16];
            float es[16];
#pragma unroll
            for (int e = 0; e < 16; e++) us[e] = e < indeg ? (int)s_src[e_base + e] : 0;
#pragma unroll
            for (int e = 0; e < 16; e++) es[e] = s_eig[us[e]];
            int prev = -1;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const bool on = e < indeg;
                const int u = us[e];
                const float we = on ? es[e] - eig_v : 0.0f;
                wsum += we;
                abssum += fabsf(we);
                if (on && ((u >> 3) & 3) == g) bits |= 1u << (((u >> 5) << 3) | (u & 7));
                ndup += (on && u == prev);
                prev = on ? u : prev;
            }
            for (int e = 16; __any(e < indeg); e++)
                if (e < indeg) {
                    const int u = s_src[e_base + e];
                    const float we = s_eig[u] - eig_v;
                    wsum += we;
                    abssum += fabsf(we);
                    if (((u >> 3) & 3) == g) bits |= 1u << (((u >> 5) << 3) | (u & 7));
                    ndup += (u == prev);
                    prev = u;
                }
            if constexpr (INFO == 1) {
                if (valid) {
                    rowinfo[(size_t)node * 8 + g] = bits;
                    if (g == 0) *reinterpret_cast<uint4*>(rowinfo + (size_t)node * 8 + 4) =
                        make_uint4(__builtin_bit_cast(uint32_t, wsum), __builtin_bit_cast(uint32_t, abssum), (uint32_t)ndup, (uint32_t)odeg);
                }
            }
        }
        const float inv_abs = 1.0f / (abssum == 0.0f ? 1.0f / 8192.0f : abssum);  // epsilon of ap_fixed<16,3> (node_embedding.cc:125-128)
        const float inv_dg = odeg == 0 ? 0.0f : 1.0f / (float)odeg;
        // adjacency operands of the four source blocks: 16-bit lane masks, then ones and the row's WEIGHTS w = eig[u] - eig[v] (split
        // hi / lo) under the mask.  The weights are formed per (row, source) in fp32 exactly as the reference forms them, and scaled by
        // the power of two that brings the row's sum |w| into [1, 2) before they are split into f16 pairs: the directional sum then
        // comes out of the matrix pipe as m2 = sum w h[u] itself, accurate relative to sum |w| |h| whatever the size of the weights.
        // (The first version multiplied by eig[u] and subtracted eig[v] m1 afterwards: two separately rounded sums whose difference a
        // row of nearly equal eigenvector entries -- sum |w| = 1e-5 -- turned into a 1.6 % error of its aggregate; found by the fuzzer.)
        const int ae = (int)((__builtin_bit_cast(uint32_t, abssum) >> 23) & 0xFFu) - 127;  // abssum in [2^ae, 2^(ae+1))
        const int aec = ae < -100 ? -100 : ae;
        const float wscale = __builtin_bit_cast(float, (uint32_t)(127 - aec) << 23);        // 2^-ae: w wscale in (-2, 2)
        const float inv_abs_s = inv_abs * __builtin_bit_cast(float, (uint32_t)(127 + aec) << 23);  // inv_abs / wscale (exact)
        const float wsum_s = wsum * wscale;
        ds_uint4_t b_one[4], b_eh[4], b_el[4];
        bool blk[4];
#pragma unroll
        for (int sb = 0; sb < 4; sb++) {
            ds_uint4_t m;
#pragma unroll
            for (int pr = 0; pr < 4; pr++) {
                const uint32_t lo16 = (uint32_t)(-(int)((bits >> (8 * sb + 2 * pr)) & 1u)) & 0xFFFFu;
                const uint32_t hi16 = (uint32_t)(-(int)((bits >> (8 * sb + 2 * pr + 1)) & 1u)) & 0xFFFF0000u;
                m[pr] = lo16 | hi16;
            }
            blk[sb] = __any(((bits >> (8 * sb)) & 0xFFu) != 0);  // wave-uniform: a source block none of the 16 rows touches is skipped
            b_one[sb] = m & (ds_uint4_t){0x3C003C00u, 0x3C003C00u, 0x3C003C00u, 0x3C003C00u};
            b_eh[sb] = (ds_uint4_t){0u, 0u, 0u, 0u};
            b_el[sb] = b_eh[sb];
            if (blk[sb]) {  // (block diagonal: a 16-row group sees two or three of the four blocks)
                const float4 ea = *reinterpret_cast<const float4*>(s_eig + 32 * sb + 8 * g), eb = *reinterpret_cast<const float4*>(s_eig + 32 * sb + 8 * g + 4);
                ds_uint4_t eh, el = {0u, 0u, 0u, 0u};  // (single product: the one rounded weight, d_uv = rne_f16((eig[u] - eig[v]) wscale); no lo half)
                DGN_OPER2((ea.x - eig_v) * wscale, (ea.y - eig_v) * wscale, eh.x, el.x);
                DGN_OPER2((ea.z - eig_v) * wscale, (ea.w - eig_v) * wscale, eh.y, el.y);
                DGN_OPER2((eb.x - eig_v) * wscale, (eb.y - eig_v) * wscale, eh.z, el.z);
                DGN_OPER2((eb.z - eig_v) * wscale, (eb.w - eig_v) * wscale, eh.w, el.w);
                b_eh[sb] = m & eh;
                b_el[sb] = m & el;
            }
        }
        float4_t acc[DGN_OT];
#pragma unroll
        for (int t = 0; t < DGN_OT; t++) {
            const float4 bv = *reinterpret_cast<const float4*>(s_w + DGN_MP_BIAS + (16 * t + 4 * g) * 4);
            acc[t] = (float4_t){bv.x, bv.y, bv.z, bv.w};
        }
        const float* hrow = h + (size_t)node * DGN_D;  // the row itself: from HBM / L2 (the tile's fp32 rows are not kept in LDS)
        if (ablate & 16) hrow = reinterpret_cast<const float*>(s_w);
        float4 hv_next = *reinterpret_cast<const float4*>(hrow + 4 * g);
        const bool dups = __any(ndup > 0);
#pragma unroll
        for (int k = 0; k < DGN_FT_KS; k++) {
            const bool real = k < 6 || g == 0;
            const float4 hv = hv_next;
            if (k + 1 < DGN_FT_KS) hv_next = *reinterpret_cast<const float4*>(hrow + ((k + 1 < 6 || g == 0) ? 16 * (k + 1) + 4 * g : 0));
            // A operand: lane (i = j, g) reads feature row 16 k + j of s_ht, sources 32 sb + 8 g .. + 7 (k = 6: rows 96 + (j & 3); the
            // other output rows of that step are discarded below)
            const int frow = k < 6 ? 16 * k + j : 96 + (j & 3);
            const uint16_t* ah = s_ht_hi + frow * DGN_HT_STRIDE + 8 * g;
            const uint16_t* al = s_ht_lo + frow * DGN_HT_STRIDE + 8 * g;
            float4_t m1 = (float4_t){0.f, 0.f, 0.f, 0.f}, pp = m1;
#pragma unroll
            for (int sb = 0; sb < 4; sb++) {
                if (blk[sb] && !(ablate & 1)) {
                    if constexpr (DGN_F16) {  // one product per aggregate and block
                        const ds_uint4_t fx = *reinterpret_cast<const ds_uint4_t*>(ah + 32 * sb);
                        m1 = DS_MFMA16(fx, b_one[sb], m1);
                        pp = DS_MFMA16(fx, b_eh[sb], pp);
                        continue;
                    }
                    const ds_uint4_t fh = *reinterpret_cast<const ds_uint4_t*>(ah + 32 * sb);
                    const ds_uint4_t fl = *reinterpret_cast<const ds_uint4_t*>(al + 32 * sb);
                    m1 = DS_MFMA16(fh, b_one[sb], m1);
                    pp = DS_MFMA16(fh, b_eh[sb], pp);
                    m1 = DS_MFMA16(fl, b_one[sb], m1);
                    pp = DS_MFMA16(fl, b_eh[sb], pp);
                    pp = DS_MFMA16(fh, b_el[sb], pp);
                }
            }
            if (dups) {  // multiplicity > 1: the extra copies of a duplicate edge, from the split rows (hi + lo)
                int prev = -1;
                const int gb = (!STAGE_CSR && valid) ? row_ptr[node] : 0;             // INFO 2: the row's in-edges straight from the CSR
                const int cnt = STAGE_CSR ? indeg : ((valid && ndup > 0) ? row_ptr[node + 1] - gb : 0);
                for (int e = 0; __any(e < cnt); e++)
                    if (e < cnt) {
                        const int u = STAGE_CSR ? (int)s_src[e_base + e] : ((src[gb + e] - t0) & 127);
                        if (u == prev && real) {
                            float eu = (s_eig[u] - eig_v) * wscale;  // the copy's (scaled) weight
                            if constexpr (DGN_F16) eu = (float)(_Float16)eu;  // ... as the first copy's: rounded once
#pragma unroll
                            for (int c = 0; c < 4; c++) {
                                const int f = (k < 6 ? 16 * k : 96) + 4 * g + c;
                                float x = (float)__builtin_bit_cast(_Float16, s_ht_hi[f * DGN_HT_STRIDE + u]);
                                if constexpr (!DGN_F16) x += (float)__builtin_bit_cast(_Float16, s_ht_lo[f * DGN_HT_STRIDE + u]);
                                m1[c] += x;
                                pp[c] = __builtin_fmaf(x, eu, pp[c]);
                            }
                        }
                        prev = u;
                    }
            }
            // a1 = m1 / outdeg (x / 0 = 0), a2 = |(m2 - wsum h[v]) / abssum|   (node_embedding.cc:143-146); pp = m2 wscale
            float4 a1, a2;
            a1.x = m1.x * inv_dg; a1.y = m1.y * inv_dg; a1.z = m1.z * inv_dg; a1.w = m1.w * inv_dg;
            a2.x = fabsf(__builtin_fmaf(-wsum_s, hv.x, pp.x) * inv_abs_s);
            a2.y = fabsf(__builtin_fmaf(-wsum_s, hv.y, pp.y) * inv_abs_s);
            a2.z = fabsf(__builtin_fmaf(-wsum_s, hv.z, pp.z) * inv_abs_s);
            a2.w = fabsf(__builtin_fmaf(-wsum_s, hv.w, pp.w) * inv_abs_s);
            if (!real || !valid) { a1 = make_float4(0.f, 0.f, 0.f, 0.f); a2 = a1; }
            ds_uint4_t b_hi, b_lo = {0u, 0u, 0u, 0u};
            DGN_OPER2(a1.x, a1.y, b_hi.x, b_lo.x);
            DGN_OPER2(a1.z, a1.w, b_hi.y, b_lo.y);
            DGN_OPER2(a2.x, a2.y, b_hi.z, b_lo.z);
            DGN_OPER2(a2.z, a2.w, b_hi.w, b_lo.w);
            asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(vmax) : "v"(a1.x), "v"(a1.y));
            asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(vmax) : "v"(a1.z), "v"(a1.w));
            asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(vmax) : "v"(a2.x), "v"(a2.y));
            asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(vmax) : "v"(a2.z), "v"(a2.w));
            asm volatile("" : "+v"(vmax));
            const char* wb = s_w + (size_t)k * (DGN_OT * DGN_FRAGS * 1024);
            if constexpr (DGN_F16) {  // single product: seven fragments, seven MFMAs, one per accumulator
                if (!(ablate & 2)) {
                    ds_uint4_t f7[DGN_OT];
#pragma unroll
                    for (int t = 0; t < DGN_OT; t++) f7[t] = *reinterpret_cast<const ds_uint4_t*>(wb + t * 1024 + lane * 16);
#pragma unroll
                    for (int t = 0; t < DGN_OT; t++) acc[t] = DS_MFMA16(f7[t], b_hi, acc[t]);
                } else { acc[0].x += b_hi.x; }
                continue;
            }
            if (!(ablate & 2)) {
            ds_uint4_t ff[2][4];  // the fragments of the NEXT pair of output tiles are requested before this pair's MFMAs issue
#pragma unroll
            for (int i = 0; i < 4; i++) ff[0][i] = *reinterpret_cast<const ds_uint4_t*>(wb + i * 1024 + lane * 16);
#pragma unroll
            for (int t0_ = 0; t0_ < DGN_OT; t0_ += 2) {
                const int n = t0_ + 1 < DGN_OT ? 2 : 1;
                const int n2 = t0_ + 3 < DGN_OT ? 2 : 1;
                if (t0_ + 2 < DGN_OT) {
#pragma unroll
                    for (int i = 0; i < 2 * n2; i++) ff[((t0_ >> 1) + 1) & 1][i] = *reinterpret_cast<const ds_uint4_t*>(wb + (((t0_ + 2) * 2) + i) * 1024 + lane * 16);
                }
                __builtin_amdgcn_sched_barrier(0);
                const ds_uint4_t (&f)[4] = ff[(t0_ >> 1) & 1];
#pragma unroll
                for (int i = 0; i < n; i++) acc[t0_ + i] = DS_MFMA16(f[2 * i], b_hi, acc[t0_ + i]);
#pragma unroll
                for (int i = 0; i < n; i++) acc[t0_ + i] = DS_MFMA16(f[2 * i], b_lo, acc[t0_ + i]);
#pragma unroll
                for (int i = 0; i < n; i++) acc[t0_ + i] = DS_MFMA16(f[2 * i + 1], b_hi, acc[t0_ + i]);
                __builtin_amdgcn_sched_barrier(0);
            }
            } else { acc[0].x += b_hi.x + b_lo.y; }
        }
        // ---- epilogue: h' = h + relu(b + W0 a1 + W1 a2)   (node_embedding.cc:176-181)
        if constexpr (!POOL) {
            if (valid) {
                // the row's own slices are requested TOGETHER, ahead of the stores: a load issued between two stores is waited for with
                // vmcnt(0), i.e. together with the store before it -- seven serialized global round trips per tile
                float4 hvv[DGN_OT];
#pragma unroll
                for (int t = 0; t < DGN_OT; t++) hvv[t] = *reinterpret_cast<const float4*>(hrow + (16 * t + 4 * g < DGN_D ? 16 * t + 4 * g : 0));
#pragma unroll
                for (int t = 0; t < DGN_OT; t++) {
                    const int c = 16 * t + 4 * g;
                    if (c < DGN_D) {
                        const float4 hv = hvv[t];
                        const float4_t rr = acc[t] * oscale;
                        *reinterpret_cast<float4*>(hout + (size_t)node * DGN_D + c) =
                            make_float4(hv.x + relu1(rr.x), hv.y + relu1(rr.y), hv.z + relu1(rr.z), hv.w + relu1(rr.w));
                    }
                }
            }
        } else if (16 * wave < rows) {  // wave-uniform: this wave owns rows of the tile
            float4_t hp[DGN_OT];
#pragma unroll
            for (int t = 0; t < DGN_OT; t++) {
                const int c = 16 * t + 4 * g;
                const float4 hv = *reinterpret_cast<const float4*>(hrow + (c < DGN_D ? c : 0));
                const float4_t rr = acc[t] * oscale;
                hp[t] = (float4_t){hv.x + relu1(rr.x), hv.y + relu1(rr.y), hv.z + relu1(rr.z), hv.w + relu1(rr.w)};
            }
            const int last = rows - 16 * wave < 16 ? rows - 16 * wave - 1 : 15;  // the wave's last row of the tile (lane = its j)
            const int g_lo = __builtin_amdgcn_readlane(gi.x, 0), g_hi = __builtin_amdgcn_readlane(gi.x, last);
            for (int G = g_lo; G <= g_hi; G++) {  // the graphs this wave has rows of (one or two; more only for tiny graphs)
                const bool in = valid && gi.x == G;
                float4_t sum[DGN_OT];
#pragma unroll
                for (int t = 0; t < DGN_OT; t++) sum[t] = in ? hp[t] : (float4_t){0.f, 0.f, 0.f, 0.f};
                // all-reduce over the 16 lanes of a feature slice (DPP row rotations 8, 4, 2, 1: the same pairs at every level in every lane)
                // (on scalar copies: with the DPP source an element of a float4_t, sum[t][i], hipcc 7.2 produced wrong sums here)
                float sv[4 * DGN_OT];
#pragma unroll
                for (int t = 0; t < DGN_OT; t++) {
#pragma unroll
                    for (int i = 0; i < 4; i++) sv[4 * t + i] = sum[t][i];
                }
                // (one v_add_f32_dpp per register and level, spelled out and in source order: hipcc leaves `x += update_dpp(x)` as
                // v_mov_b32_dpp + v_add_f32; a register is read again 28 instructions after it was written, the s_nop covers a level's first read)
#define DGN_ROR_ADD(ROR)                                                                                                          \
    asm volatile("s_nop 1");                                                                                                      \
    _Pragma("unroll") for (int k = 0; k < 4 * DGN_OT; k++)                                                                        \
        asm volatile("v_add_f32_dpp %0, %1, %1 row_ror:" #ROR " row_mask:0xf bank_mask:0xf" : "=v"(sv[k]) : "v"(sv[k]));
                DGN_ROR_ADD(8) DGN_ROR_ADD(4) DGN_ROR_ADD(2) DGN_ROR_ADD(1)
#undef DGN_ROR_ADD
#pragma unroll
                for (int t = 0; t < DGN_OT; t++) sum[t] = (float4_t){sv[4 * t], sv[4 * t + 1], sv[4 * t + 2], sv[4 * t + 3]};
                // the lane of the graph's first row held by this wave writes, in every feature slice
                const unsigned long long inm = __ballot(in && g == 0);
                if (inm == 0ull) continue;  // (cannot happen: a graph's rows are contiguous)
                const int jf = __ffsll((long long)inm) - 1;
                const int first_rel = __builtin_amdgcn_readlane(gi.y & 0xFF, jf);        // (row of jf) - (graph's first row)
                const int to_end = __builtin_amdgcn_readlane((gi.y >> 8) & 0xFFF, jf);   // (graph's end) - (row of jf)
                const int row_jf = 16 * wave + jf;                                        // inside the tile
                const int gstart = row_jf - first_rel, gend = row_jf + to_end;            // the graph's rows inside the tile: [gstart, gend)
                const int rel = wave - (gstart >> 4);
                if (j == jf) {
                    float* dst = pool_part + ((size_t)G * 8 + rel) * DGN_D;
#pragma unroll
                    for (int t = 0; t < DGN_OT; t++) {
                        const int c = 16 * t + 4 * g;
                        if (c < DGN_D) *reinterpret_cast<float4*>(dst + c) = make_float4(sum[t].x, sum[t].y, sum[t].z, sum[t].w);
                    }
                    if (rel == 0 && g == 0) pool_cnt[G] = ((gend - 1) >> 4) - (gstart >> 4) + 1;
                }
            }
        }
        if (!has_next) break;
        __syncthreads();  // every wave is done with this tile's transposed rows, CSR slice and eigenvector column
        if (!(ablate & 4)) {
        put_row_piece(cg, nr0, lr < nrows); put_row_piece(4 + cg, nr1, lr < nrows); put_row_piece(8 + cg, nr2, lr < nrows);
        put_row_piece(12 + cg, nr3, lr < nrows); put_row_piece(16 + cg, nr4, lr < nrows); put_row_piece(20 + cg, nr5, lr < nrows);
        put_row_piece(24 + cg, nr6, lr < nrows);
        } else { s_ht_hi[tid] = (uint16_t)(nr0.x + nr1.x + nr2.x + nr3.x + nr4.x + nr5.x + nr6.x); }
#define DGN_PUTE(P, V) if (STAGE_CSR && tid + 512 * (P) < nne) s_src[tid + 512 * (P)] = (uint8_t)(((V) - nt0) & 127);
        DGN_PUTE(0, ns0) DGN_PUTE(1, ns1) DGN_PUTE(2, ns2) DGN_PUTE(3, ns3) DGN_PUTE(4, ns4)
#undef DGN_PUTE
        if (STAGE_CSR && tid <= nrows) { const int o = nx_rp - ne0; s_rp[tid] = (uint16_t)(o < 0 ? 0 : (o > nne ? nne : o)); }
        if (tid < DGN_FT_ROWS) put_eig(tid, nx_eig, tid < nrows);
        __syncthreads();
        tile = ntile; t0 = nt0; rows = nrows; e0 = ne0; ne = nne;
        cur_bits = nx_bits; cur_info = nx_info;
    }
    if constexpr (DGN_F16) vmax = __builtin_fmaxf(vmax, hmax);
    if (__any(!(vmax < 6.0e4f))) {
        if (lane == 0) atomicOr(range_flag, 1);
    }
}

// The in-edge pass of dgn_layer_mfma_kernel<1> -- adjacency mask, wsum, abssum, duplicate count per row -- and the out-degrees,
// straight from the caller's edge list: what the matrix-pipe path needs of load_graph (DGN/src/load_inputs.cc:87-172) WITHOUT the
// CSR.  One 256-thread workgroup per tile of whole graphs (<= 128 rows): the tile's edges are a contiguous slice of edge_list;
// each is validated, turned into (source row, destination row) of the tile and ORed into a 128 x 128 bit matrix in LDS (an
// atomicOr that finds its bit set has found a duplicate edge).  Thread v then walks the set bits of row v in ascending order --
// the CSR's order (sources ascending), so wsum and abssum add the same terms in the same order as the walk over the CSR row and
// rowinfo is bit-identical to what INFO = 1 stores.  Rows with duplicate in-edges (multiplicity is not in the mask) count the
// copies by a scan over the tile's edges -- rare -- and raise *dup_flag: the launching model then also builds the CSR (on the
// device's say-so: launch_build_csr(..., only_if)), because the layer kernels' correction walk for duplicates reads it.
// REC (the graph-resident kernel's tile build): the row's record is 12 words -- the eight above, eig1[v], and the nine encoder
// table rows offset_k + feature_k (validated as atom_encoder_kernel validates them) as bytes: everything dgn_resident_kernel reads
// per row.  Duplicate edges need no CSR there (that kernel re-sums such rows from the caller's edge list): dup_flag is not raised.
// `list` (REC only, GraphTiles::bp_list; null: tile t holds the graphs tile_graph[t] .. tile_graph[t + 1] - 1 and its rows are the batch's
// rows tile_row[t] ..): tile t holds the graphs list[tile_graph[t]] .. list[tile_graph[t + 1] - 1], one behind the other, and
// tile_row[t] is its first row in the tile-ordered record space -- a row's inputs (features, eig1) are then found through its graph.
template <bool REC>
__global__ __launch_bounds__(256) void dgn_rowinfo_kernel(BatchView b, const int* __restrict__ tile_row, const int* __restrict__ tile_graph,
                                                          int n_tiles, const float* __restrict__ eig4, uint32_t* __restrict__ rowinfo,
                                                          int* __restrict__ out_deg, int* __restrict__ err, int* __restrict__ dup_flag,
                                                          const int* __restrict__ list = nullptr) {
    __shared__ uint32_t s_adj[DGN_FT_ROWS][4];
    __shared__ int s_odeg[DGN_FT_ROWS], s_ndup[DGN_FT_ROWS];
    __shared__ float s_eig[DGN_FT_ROWS];
    __shared__ int s_node[DGN_FT_ROWS];  // the batch's node behind every row of the tile
    const int tile = blockIdx.x, tid = threadIdx.x;
    if (tile >= n_tiles) return;
    const int t0 = tile_row[tile];
    int rows = tile_row[tile + 1] - t0;
    if (rows > DGN_FT_ROWS) rows = DGN_FT_ROWS;
    const int g0 = tile_graph[tile], g1 = tile_graph[tile + 1];
    if (tid < DGN_FT_ROWS) {
        s_adj[tid][0] = 0u; s_adj[tid][1] = 0u; s_adj[tid][2] = 0u; s_adj[tid][3] = 0u;
        s_odeg[tid] = 0; s_ndup[tid] = 0;
        s_node[tid] = 0;
    }
    __syncthreads();
    {
        int run = 0;
        for (int i = g0; i < g1; i++) {
            const int gph = list ? list[i] : i;
            const int n = b.nums_of_nodes[gph], first = b.node_off[gph], base = list ? run : first - t0;
            for (int k = tid; k < n; k += 256)
                if (base + k < DGN_FT_ROWS) s_node[base + k] = first + k;
            run += n;
        }
    }
    __syncthreads();
    if (tid < DGN_FT_ROWS) s_eig[tid] = tid < rows ? eig4[(size_t)s_node[tid] * 4 + 1] : 0.0f;
    {
        int run = 0;
        for (int i = g0; i < g1; i++) {
            const int gph = list ? list[i] : i;
            const int n = b.nums_of_nodes[gph], base = list ? run : b.node_off[gph] - t0, e0 = b.edge_off[gph], ne = b.edge_off[gph + 1] - e0;
            run += n;
            for (int e = tid; e < ne; e += 256) {
                const int2 uv = reinterpret_cast<const int2*>(b.edge_list)[e0 + e];
                int u = uv.x, v = uv.y;
                if (!((u >= 0) & (u < n) & (v >= 0) & (v < n))) {  // as the index build: flag it, then a self-loop on the graph's node 0
                    atomicMax(err, ERR_EDGE_RANGE);
                    u = 0;
                    v = 0;
                }
                u += base; v += base;
                if (u >= DGN_FT_ROWS || v >= DGN_FT_ROWS) continue;  // (cannot happen: the host packed whole graphs into <= 128 rows)
                const uint32_t bit = 1u << (u & 31);
                const uint32_t old = atomicOr(&s_adj[v][u >> 5], bit);
                if (old & bit) atomicAdd(&s_ndup[v], 1);
                atomicAdd(&s_odeg[u], 1);
            }
        }
    }
    __syncthreads();
    if (tid < rows) {
        const int v = tid;
        const float eig_v = s_eig[v];
        const int nd = s_ndup[v];
        float wsum = 0.0f, abssum = 0.0f;
        for (int sb = 0; sb < 4; sb++) {
            uint32_t w = s_adj[v][sb];
            while (w) {
                const int u = 32 * sb + __ffs((int)w) - 1;
                w &= w - 1;
                int mult = 1;
                if (nd > 0) {  // how many copies of (u -> v) the caller listed: a scan over the tile's edges (rows with duplicates only)
                    mult = 0;
                    int run = 0;
                    for (int i = g0; i < g1; i++) {
                        const int gph = list ? list[i] : i;
                        const int n = b.nums_of_nodes[gph], base = list ? run : b.node_off[gph] - t0, e0 = b.edge_off[gph], ne = b.edge_off[gph + 1] - e0;
                        run += n;
                        if (v < base || v >= base + n) continue;
                        for (int e = 0; e < ne; e++) {
                            const int2 uv = reinterpret_cast<const int2*>(b.edge_list)[e0 + e];
                            int uu = uv.x, vv = uv.y;
                            if (!((uu >= 0) & (uu < n) & (vv >= 0) & (vv < n))) { uu = 0; vv = 0; }
                            mult += (uu + base == u) & (vv + base == v);
                        }
                    }
                }
                const float we = s_eig[u] - eig_v;
                for (int k = 0; k < mult; k++) { wsum += we; abssum += fabsf(we); }
            }
        }
        // this lane group's byte of every 32-source block: bit 8 s + e <-> source 32 s + 8 g + e (dgn_layer_mfma_kernel)
        uint32_t* ri = rowinfo + (size_t)(t0 + v) * (REC ? DGN_REC_DW : 8);
#pragma unroll
        for (int gq = 0; gq < 4; gq++) {
            uint32_t wg = 0;
#pragma unroll
            for (int sb = 0; sb < 4; sb++) wg |= ((s_adj[v][sb] >> (8 * gq)) & 0xFFu) << (8 * sb);
            ri[gq] = wg;
        }
        // (the out-degree rides in the record's fourth word: the layers read it a tile ahead with the rest instead of loading out_deg[node]
        // at the top of the tile, where its round trip stood in front of the row's 1 / deg)
        *reinterpret_cast<uint4*>(ri + 4) = make_uint4(__builtin_bit_cast(uint32_t, wsum), __builtin_bit_cast(uint32_t, abssum), (uint32_t)nd, (uint32_t)s_odeg[v]);
        if constexpr (REC) {
            uint32_t fw[3] = {0u, 0u, 0u};
            const int* nf = b.node_feature + (size_t)s_node[v] * ND_FEATURE;
#pragma unroll
            for (int k = 0; k < ND_FEATURE; k++) {
                int f = nf[k];
                if (f < 0 || f >= c_nd_card[k]) {
                    atomicMax(err, ERR_NODE_FEAT);
                    f = 0;
                }
                fw[k >> 2] |= (uint32_t)(c_nd_off[k] + f) << (8 * (k & 3));
            }
            *reinterpret_cast<uint4*>(ri + 8) = make_uint4(__builtin_bit_cast(uint32_t, eig_v), fw[0], fw[1], fw[2]);
        } else {
            out_deg[t0 + v] = s_odeg[v];
            if (nd > 0) atomicOr(dup_flag, 1);
        }
    }
}

// ginfo[node] = (graph, (node - graph's first node) | (graph's end - node) << 8) for the POOL epilogue above: one thread per graph
// (graphs of this path have <= 128 nodes)
__global__ __launch_bounds__(256) void dgn_graph_info_kernel(const int* __restrict__ node_off, int num_graphs, int2* __restrict__ ginfo) {
    const int gph = blockIdx.x * 256 + threadIdx.x;
    if (gph >= num_graphs) return;
    const int n0 = node_off[gph], n1 = node_off[gph + 1];
    for (int v = n0; v < n1; v++) ginfo[v] = make_int2(gph, ((v - n0) & 0xFF) | ((n1 - v) << 8));
}

// The head of DGN's readout on one graph's pooled row, one wavefront: 100 -> 50 (ReLU) -> 25 (ReLU) -> 25 products with the last
// layer's weights, summed over the lanes (finalize.cc:28-52; the caller adds the last bias).  s_hg [100] and s_o1 [50] are the wave's
// own LDS scratch, w1t [100][ld1] and w2t [50][ld2] the transposed weights in LDS (unit along the lanes).  Shared by the per-layer
// path's readout kernel and the graph-resident kernel's tail: the same instructions, the same bits.
__device__ __forceinline__ float dgn_head_wave(const float* s_hg, float* s_o1, const float* s_w1t, int ld1, const float* s_w2t, int ld2,
                                               float bias1, float bias2, float w3l, int lane) {
    // Each dot product as FOUR interleaved chains (inputs i = 0, 1, 2, 3 mod 4; the first starts from the bias), added as
    // (s0 + s1) + (s2 + s3): a single chain of 100 dependent FMAs is latency, one wave per graph has nothing to hide it with, and
    // the resident kernel pays that latency per tile.  The order is part of this function's definition: every caller rounds alike.
    if (lane < 50) {
        float s0 = bias1, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll 5
        for (int i = 0; i < DGN_D; i += 4) {
            const float4 x = *reinterpret_cast<const float4*>(s_hg + i);
            s0 = __builtin_fmaf(x.x, s_w1t[(i + 0) * ld1 + lane], s0);
            s1 = __builtin_fmaf(x.y, s_w1t[(i + 1) * ld1 + lane], s1);
            s2 = __builtin_fmaf(x.z, s_w1t[(i + 2) * ld1 + lane], s2);
            s3 = __builtin_fmaf(x.w, s_w1t[(i + 3) * ld1 + lane], s3);
        }
        s_o1[lane] = relu1((s0 + s1) + (s2 + s3));
    }
    __builtin_amdgcn_wave_barrier();
    float p = 0.f;
    if (lane < 25) {
        float s0 = bias2, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll 4
        for (int i = 0; i < 48; i += 4) {
            const float4 x = *reinterpret_cast<const float4*>(s_o1 + i);
            s0 = __builtin_fmaf(x.x, s_w2t[(i + 0) * ld2 + lane], s0);
            s1 = __builtin_fmaf(x.y, s_w2t[(i + 1) * ld2 + lane], s1);
            s2 = __builtin_fmaf(x.z, s_w2t[(i + 2) * ld2 + lane], s2);
            s3 = __builtin_fmaf(x.w, s_w2t[(i + 3) * ld2 + lane], s3);
        }
        s0 = __builtin_fmaf(s_o1[48], s_w2t[48 * ld2 + lane], s0);
        s1 = __builtin_fmaf(s_o1[49], s_w2t[49 * ld2 + lane], s1);
        p = relu1((s0 + s1) + (s2 + s3)) * w3l;
    }
    // the 25 products of the last layer: all-reduce inside each row of 16 lanes (DPP rotations 8, 4, 2, 1: lanes 25..31 hold zeros),
    // then row 0 + row 1 (six ds_bpermute shuffles cost ~600 clocks here)
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf" : "+v"(p));
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf" : "+v"(p));
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf" : "+v"(p));
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf" : "+v"(p));
    const int pb = __builtin_bit_cast(int, p);  // (readlane is an int builtin: a float argument would be CONVERTED)
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(pb, 0)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(pb, 16));
}

// readout of the POOL form: mean over the graph's nodes from the per-wave partial sums (added in wave order), then the 3-layer head
// of pool_mlp3_kernel (device_common.h) with the same arithmetic per graph.  Persistent workgroups, one wavefront per graph at a
// time; W1 and W2 are staged once per workgroup in LDS, transposed (unit along the lanes: conflict-free) -- read from global memory
// in [unit][input] order every lane of a step touches another cache line, and the head then costs more than the pooling it follows.
// PARTS false: the pooled row from the rows of h themselves (even rows | odd rows, then the two halves: pool_mlp3_kernel's order, which
// is also the graph-resident kernel's) -- the readout of the per-layer path when the last layer's rows are kept.
// EMB (flowgnn_set_embeddings): the instances that also store the pooled row to emb[g].
template <bool PARTS, bool EMB = false>
__global__ __launch_bounds__(256) void dgn_pool_part_mlp3_kernel(const float* __restrict__ part /* [G][8][100], or h [N][100] */, const int* __restrict__ cnt,
                                                                 const int* __restrict__ node_off, const float* __restrict__ w1,
                                                                 const float* __restrict__ b1, const float* __restrict__ w2,
                                                                 const float* __restrict__ b2, const float* __restrict__ w3,
                                                                 const float* __restrict__ b3, float* __restrict__ out, int num_graphs,
                                                                 float* __restrict__ emb = nullptr /* [G][100] pooled rows (EMB instances) */) {
    constexpr int D = DGN_D, H1 = 50, H2 = 25, P1 = H1 + 1, P2 = H2 + 2;
    __shared__ float s_w1t[D * P1];   // [input][unit]
    __shared__ float s_w2t[H1 * P2];  // [input][unit]
    __shared__ __attribute__((aligned(16))) float s_hg[4][D];
    __shared__ __attribute__((aligned(16))) float s_o1[4][H1 + 2];
    for (int i = threadIdx.x; i < H1 * D; i += 256) s_w1t[(i % D) * P1 + i / D] = w1[i];
    for (int i = threadIdx.x; i < H2 * H1; i += 256) s_w2t[(i % H1) * P2 + i / H1] = w2[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float bias1 = lane < H1 ? b1[lane] : 0.0f, bias2 = lane < H2 ? b2[lane] : 0.0f, w3l = lane < H2 ? w3[lane] : 0.0f, bias3 = b3[0];
    for (int gph = blockIdx.x * 4 + wv; gph < num_graphs; gph += gridDim.x * 4) {
        const int n0 = node_off[gph], n1 = node_off[gph + 1];
        const float n = (float)(n1 - n0);
        if constexpr (PARTS) {
            const int nw = cnt[gph];
            for (int c = lane; c < D; c += 64) {
                float sum = 0.0f;
                for (int k = 0; k < nw; k++) sum += part[((size_t)gph * 8 + k) * D + c];
                s_hg[wv][c] = sum / n;
            }
        } else {
            const int half = lane >> 5, c = lane & 31;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < DGN_C) pool_rows_in_order<DGN_C>(acc, part, n0 + half, n1, c);
            acc.x += __shfl_down(acc.x, 32, 64); acc.y += __shfl_down(acc.y, 32, 64);
            acc.z += __shfl_down(acc.z, 32, 64); acc.w += __shfl_down(acc.w, 32, 64);
            if (half == 0 && c < DGN_C) {
                s_hg[wv][4 * c + 0] = acc.x / n; s_hg[wv][4 * c + 1] = acc.y / n;
                s_hg[wv][4 * c + 2] = acc.z / n; s_hg[wv][4 * c + 3] = acc.w / n;
            }
        }
        __builtin_amdgcn_wave_barrier();
        if constexpr (EMB) {
            if (lane < DGN_C) reinterpret_cast<float4*>(emb + (size_t)gph * D)[lane] = *reinterpret_cast<const float4*>(&s_hg[wv][4 * lane]);
        }
        const float p = dgn_head_wave(s_hg[wv], s_o1[wv], s_w1t, P1, s_w2t, P2, bias1, bias2, w3l, lane);
        if (lane == 0) out[gph] = bias3 + p;
        __builtin_amdgcn_wave_barrier();  // s_hg / s_o1 are rewritten for the wave's next graph
    }
}

// ---------------------------------------------------------------- graph-resident DGN: load_graph to the logit without leaving the chip
// The FPGA holds one graph on chip from load_graph to the logit (DGN/src/DGN_compute.cc:44-104).  Here a persistent 8-wave workgroup
// (one per CU) holds a tile of WHOLE graphs (GraphTiles: <= 128 rows) across the encoder, all four layers and the readout:
//   tile build   dgn_tile_build_kernel (the launch in front): per row a 48-byte record from the caller's arrays -- adjacency mask,
//                wsum, abssum, duplicate count, out-degree (as dgn_rowinfo_kernel), eig1 and the nine encoder table rows as bytes;
//   loader       the tile's records come by LDS-DMA (6 KiB, requested a tile ahead); h_0 = the nine-term encoder sum
//                (load_inputs.cc:114-172) in atom_encoder_kernel's order out of the LDS-resident table, into REGISTERS: lane (j, g)
//                of wave w keeps features 16 t + 4 g .. + 3 (t < 7) of row 16 w + j in fp32 for the whole tile -- the accumulator layout
//                of the dense update, so the self term h[v] of a K-step and the residual never touch memory;
//   layers       the matrix-pipe aggregation of dgn_layer_mfma_kernel over the transposed f16-split rows s_ht (rebuilt from the
//                registers between layers, in place) with the adjacency operands built ONCE per tile; the dense update's weights
//                do not fit beside the encoder table (100 KB per layer), so they stream through two 14 KiB LDS slots, one K-step's
//                fragments each, across the 28 K-steps of the tile: one barrier per K-step (vmcnt(0) + s_barrier, then the request
//                for the next chunk).  (Waves 4..7 passing that barrier between their aggregation and their dense half -- the two
//                waves of a SIMD half a K-step apart, as in pna_layer_fused_kernel -- measured 2.23 ms against 2.17: not kept);
//   readout      h_4 goes to LDS as fp32 rows, then one wave per graph: pool_mlp3_kernel's sum order and head (finalize.cc:28-52).
// HBM traffic per row: the 48-byte record; per graph one logit.  Same operations in the same order as atom_encoder_kernel +
// dgn_rowinfo + 4 x dgn_layer_mfma_kernel<2, false> + pool_mlp3_kernel on the same tiles: the same bits.  (Like that path, the
// order of a row's in-edge sum depends on where its graph sits in the tile: toleranced under batch splits, tests/test_dgn_gpu.py.)
// Rows with duplicate in-edges (the mask has no multiplicities) add the extra copies from the caller's edge list: slow and rare.
constexpr int DGN_REC_TILE_BYTES = DGN_FT_ROWS * DGN_REC_DW * 4;  // 6 144: six DMA pieces
constexpr int DGN_CHUNK = DGN_OT * DGN_FRAGS * 1024;              // 14 336: the fragments of one K-step (single product: 7 168)
// the readout's head in one block (25 DMA pieces into the two weight slots, which are idle by then)
constexpr int DGN_HEAD_W2 = 100 * 50, DGN_HEAD_B1 = DGN_HEAD_W2 + 50 * 25, DGN_HEAD_B2 = DGN_HEAD_B1 + 50, DGN_HEAD_W3 = DGN_HEAD_B2 + 25,
              DGN_HEAD_B3 = DGN_HEAD_W3 + 25, DGN_HEAD_BYTES = 25 * 1024;
// the two weight slots; single product: two 7 KiB chunks are smaller than the head block that follows them there, so the region keeps the head's size
constexpr int DGN_WSLOT_BYTES = 2 * DGN_CHUNK < DGN_HEAD_BYTES ? DGN_HEAD_BYTES : 2 * DGN_CHUNK;
static_assert((DGN_HEAD_B3 + 1) * 4 <= DGN_HEAD_BYTES && DGN_HEAD_BYTES <= DGN_WSLOT_BYTES, "the head fits the two slots");

#ifdef FLOWGNN_DEV
#include "dev/dgn_timing_variants.h"  // development: timing variants (wrong results on purpose), selected by -DDGNR_TIMING=<bits>
#else
#define DGNR_SKIP(bit) false
#endif

struct DgnResidentArgs : DgnResidentLaunch {};  // the kernel's parameter: the same, in the namespace of this translation unit's kernel

__global__ __launch_bounds__(512, 2) void dgn_resident_kernel(const DgnResidentArgs a) {
    constexpr int OFF_W = 2 * DGN_HT_BYTES, OFF_TAB = OFF_W + DGN_WSLOT_BYTES, OFF_REC = OFF_TAB + ND_FEATURE_TOTAL * DGN_D * 4,
                  OFF_BIAS = OFF_REC + DGN_REC_TILE_BYTES, OFF_EIG = OFF_BIAS + DGN_L * 512, LDS_TOTAL = OFF_EIG + 4 * DGN_FT_ROWS;
    static_assert(OFF_W % 16 == 0 && OFF_TAB % 16 == 0 && OFF_REC % 16 == 0 && OFF_BIAS % 16 == 0 && OFF_EIG % 16 == 0, "alignment");
    static_assert(LDS_TOTAL <= 160 * 1024, "LDS of one CU");
    static_assert(DGN_FT_ROWS * DGN_D * 4 <= OFF_W, "the readout's fp32 rows take the place of s_ht");
    __shared__ __attribute__((aligned(16))) char s_all[LDS_TOTAL];
    uint16_t* s_ht_hi = reinterpret_cast<uint16_t*>(s_all);
    uint16_t* s_ht_lo = reinterpret_cast<uint16_t*>(s_all + DGN_HT_BYTES);
    char* s_w = s_all + OFF_W;
    const float4* s_tab = reinterpret_cast<const float4*>(s_all + OFF_TAB);
    const uint32_t* s_rec = reinterpret_cast<const uint32_t*>(s_all + OFF_REC);
    float* s_bias = reinterpret_cast<float*>(s_all + OFF_BIAS);
    float* s_eig = reinterpret_cast<float*>(s_all + OFF_EIG);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    int tile = blockIdx.x;
    if (tile >= a.n_tiles) return;
    auto issue_chunk = [&](int l, int k) {  // K-step k of layer l -> slot (l + k) & 1: fourteen 1 KiB pieces over eight waves
        const uint8_t* gsrc = a.wpk + (size_t)l * DGN_MP_LAYER_BYTES + (size_t)k * DGN_CHUNK;
        const uint32_t lb = lds_addr_of(s_w) + (uint32_t)(((l + k) & 1) * DGN_CHUNK);
        if constexpr (DGN_F16) {  // seven 1 KiB pieces: one each on waves 0..6
            if (wave < DGN_OT) lds_dma16(gsrc + wave * 1024, (uint32_t)lane * 16u, lb + wave * 1024);
            return;
        }
        lds_dma16(gsrc + wave * 1024, (uint32_t)lane * 16u, lb + wave * 1024);
        if (wave < 6) lds_dma16(gsrc + (wave + 8) * 1024, (uint32_t)lane * 16u, lb + (wave + 8) * 1024);
    };
    auto issue_rec = [&](int t) {  // a tile's records -> s_rec: six pieces, on the waves that carry one chunk piece only and four more
        if (wave >= 2) {
            const int piece = 7 - wave;
            lds_dma16(reinterpret_cast<const char*>(a.rec) + (size_t)a.tile_row[t] * (DGN_REC_DW * 4) + piece * 1024, (uint32_t)lane * 16u,
                      lds_addr_of(s_rec) + piece * 1024);
        }
    };
    auto issue_head = [&]() {  // the readout's head block -> the two slots (idle behind a tile's last K-step)
        const uint32_t lb = lds_addr_of(s_w);
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int piece = wave + 8 * p;
            if (piece < DGN_HEAD_BYTES / 1024) lds_dma16(reinterpret_cast<const char*>(a.head) + piece * 1024, (uint32_t)lane * 16u, lb + piece * 1024);
        }
    };
    issue_rec(tile);
    // once per workgroup: the encoder table and the four layers' bias vectors (pre-scaled, 112 floats + 1 / scale each)
    for (int i = tid; i < ND_FEATURE_TOTAL * DGN_C; i += 512)
        reinterpret_cast<float4*>(s_all + OFF_TAB)[i] = reinterpret_cast<const float4*>(a.table)[i];
    if (tid < DGN_L * 128) s_bias[tid] = *reinterpret_cast<const float*>(a.wpk + (size_t)(tid >> 7) * DGN_MP_LAYER_BYTES + DGN_MP_BIAS + (tid & 127) * 4);
    const int lr = 16 * wave + j;  // this lane's row of the tile (the four lanes g of a row share it)
    float hmax = 0.0f;  // single product: the largest |h| rounded into s_ht (joins vmax at the end: beyond 6e4 the range flag trips)
    auto put_row_piece = [&](int c, const float4_t& x) {  // features 4 c .. 4 c + 3 of row lr -> the transposed split rows
        if (c >= DGN_C) return;
        if constexpr (DGN_F16) {  // one rounding to nearest even per feature, no lo half
            const uint32_t r01 = dgn_pack_rne(x.x, x.y), r23 = dgn_pack_rne(x.z, x.w);
            hmax = __builtin_fmaxf(__builtin_fmaxf(hmax, __builtin_fabsf(x.x)), __builtin_fabsf(x.y));
            hmax = __builtin_fmaxf(__builtin_fmaxf(hmax, __builtin_fabsf(x.z)), __builtin_fabsf(x.w));
            uint16_t* pr = s_ht_hi + (4 * c) * DGN_HT_STRIDE + lr;
            pr[0] = (uint16_t)r01; pr[DGN_HT_STRIDE] = (uint16_t)(r01 >> 16); pr[2 * DGN_HT_STRIDE] = (uint16_t)r23; pr[3 * DGN_HT_STRIDE] = (uint16_t)(r23 >> 16);
            return;
        }
        uint32_t h01, l01, h23, l23;
        DS_SPLIT2(x.x, x.y, h01, l01);
        DS_SPLIT2(x.z, x.w, h23, l23);
        uint16_t* ph = s_ht_hi + (4 * c) * DGN_HT_STRIDE + lr;
        uint16_t* pl = s_ht_lo + (4 * c) * DGN_HT_STRIDE + lr;
        ph[0] = (uint16_t)h01; ph[DGN_HT_STRIDE] = (uint16_t)(h01 >> 16); ph[2 * DGN_HT_STRIDE] = (uint16_t)h23; ph[3 * DGN_HT_STRIDE] = (uint16_t)(h23 >> 16);
        pl[0] = (uint16_t)l01; pl[DGN_HT_STRIDE] = (uint16_t)(l01 >> 16); pl[2 * DGN_HT_STRIDE] = (uint16_t)l23; pl[3 * DGN_HT_STRIDE] = (uint16_t)(l23 >> 16);
    };
    float vmax = 0.0f;
    while (true) {
        const int t0 = a.tile_row[tile];
        int rows = a.tile_row[tile + 1] - t0;
        if (rows > DGN_FT_ROWS) rows = DGN_FT_ROWS;
        const int ntile = tile + gridDim.x;
        const bool has_next = ntile < a.n_tiles;
        issue_chunk(0, 0);  // slot 0: last read in K-step 26 of the previous tile, and every wave is past that step's barrier
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this tile's records (and the chunk)
        __syncthreads();                                  // ... of every wave; the previous tile's readout is over
        // ---- this lane's row: the stored in-edge pass, eig1, the encoder
        const bool valid = lr < rows;
        const uint32_t* rc = s_rec + lr * DGN_REC_DW;
        const uint32_t bits = valid ? rc[g] : 0u;
        const uint4 info = *reinterpret_cast<const uint4*>(rc + 4);
        const float wsum = valid ? __builtin_bit_cast(float, info.x) : 0.0f;
        const float abssum = valid ? __builtin_bit_cast(float, info.y) : 0.0f;
        const int ndup = valid ? (int)info.z : 0;
        const int odeg = valid ? (int)info.w : 0;
        const float eig_v = valid ? __builtin_bit_cast(float, rc[8]) : 0.0f;
        if (g == 0) s_eig[lr] = eig_v;  // rows beyond the tile's last: zeros (never NaN under a zero mask)
        float4_t hreg[DGN_OT];
        {
            const uint32_t f0 = rc[9], f1 = rc[10], f2 = rc[11];
            int trow[ND_FEATURE];
#pragma unroll
            for (int k = 0; k < ND_FEATURE; k++) trow[k] = (int)(((k < 4 ? f0 : (k < 8 ? f1 : f2)) >> (8 * (k & 3))) & 0xFFu) * DGN_C;
#pragma unroll
            for (int t = 0; t < DGN_OT; t++) {
                const int c = 4 * t + g;
                const int cc = c < DGN_C ? c : 0;
                float4 w[ND_FEATURE];
#pragma unroll
                for (int k = 0; k < ND_FEATURE; k++) w[k] = DGNR_SKIP(16) ? make_float4(0.f, 0.f, 0.f, (float)trow[k]) : s_tab[(valid ? trow[k] : 0) + cc];
                float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int k = 0; k < ND_FEATURE; k++) { s.x += w[k].x; s.y += w[k].y; s.z += w[k].z; s.w += w[k].w; }
                const bool on = valid && c < DGN_C;
                hreg[t] = (float4_t){on ? s.x : 0.f, on ? s.y : 0.f, on ? s.z : 0.f, on ? s.w : 0.f};
            }
        }
#pragma unroll
        for (int t = 0; t < DGN_OT; t++) put_row_piece(4 * t + g, hreg[t]);
        const float inv_abs = 1.0f / (abssum == 0.0f ? 1.0f / 8192.0f : abssum);  // epsilon of ap_fixed<16,3> (node_embedding.cc:125-128)
        const float inv_dg = odeg == 0 ? 0.0f : 1.0f / (float)odeg;
        const int ae = (int)((__builtin_bit_cast(uint32_t, abssum) >> 23) & 0xFFu) - 127;  // abssum in [2^ae, 2^(ae+1))
        const int aec = ae < -100 ? -100 : ae;
        const float wscale = __builtin_bit_cast(float, (uint32_t)(127 - aec) << 23);        // 2^-ae: w wscale in (-2, 2)
        const float inv_abs_s = inv_abs * __builtin_bit_cast(float, (uint32_t)(127 + aec) << 23);  // inv_abs / wscale (exact)
        const float wsum_s = wsum * wscale;
        // adjacency operands of the four source blocks (dgn_layer_mfma_kernel): once per TILE here, the four layers share them
        ds_uint4_t b_one[4], b_eh[4], b_el[4];
        bool blk[4];
#pragma unroll
        for (int sb = 0; sb < 4; sb++) {
            ds_uint4_t m;
#pragma unroll
            for (int pr = 0; pr < 4; pr++) {
                const uint32_t lo16 = (uint32_t)(-(int)((bits >> (8 * sb + 2 * pr)) & 1u)) & 0xFFFFu;
                const uint32_t hi16 = (uint32_t)(-(int)((bits >> (8 * sb + 2 * pr + 1)) & 1u)) & 0xFFFF0000u;
                m[pr] = lo16 | hi16;
            }
            blk[sb] = __any(((bits >> (8 * sb)) & 0xFFu) != 0);
            b_one[sb] = m & (ds_uint4_t){0x3C003C00u, 0x3C003C00u, 0x3C003C00u, 0x3C003C00u};
            b_eh[sb] = (ds_uint4_t){0u, 0u, 0u, 0u};
            b_el[sb] = b_eh[sb];
            if (blk[sb]) {
                float es[8];  // eig1 of sources 32 sb + 8 g .. + 7 (records of rows beyond the tile's last are never under a set bit)
#pragma unroll
                for (int i = 0; i < 8; i++) es[i] = __builtin_bit_cast(float, s_rec[(32 * sb + 8 * g + i) * DGN_REC_DW + 8]);
                ds_uint4_t eh, el = {0u, 0u, 0u, 0u};  // (single product: the one rounded weight, d_uv = rne_f16((eig[u] - eig[v]) wscale); no lo half)
                DGN_OPER2((es[0] - eig_v) * wscale, (es[1] - eig_v) * wscale, eh.x, el.x);
                DGN_OPER2((es[2] - eig_v) * wscale, (es[3] - eig_v) * wscale, eh.y, el.y);
                DGN_OPER2((es[4] - eig_v) * wscale, (es[5] - eig_v) * wscale, eh.z, el.z);
                DGN_OPER2((es[6] - eig_v) * wscale, (es[7] - eig_v) * wscale, eh.w, el.w);
                b_eh[sb] = m & eh;
                b_el[sb] = m & el;
            }
        }
        const bool dups = __any(ndup > 0);
        const int g0 = a.tile_graph[tile], g1 = a.tile_graph[tile + 1];
        // the first row (inside the tile) of each of the tile's first 63 graphs, one per lane; lane = graph count: the tile's rows.  For the
        // readout, 28 K-steps from here, and the rare rows with duplicate in-edges
        int my_noff;
        if (a.list) {  // a list of graphs: running sum of their node counts (inclusive scan over the lanes, shifted by one)
            const int cnt = g0 + lane < g1 ? a.b.nums_of_nodes[a.list[g0 + lane]] : 0;
            int incl = cnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(incl, d, 64);
                if (lane >= d) incl += o;
            }
            my_noff = incl - cnt;
        } else {
            my_noff = a.b.node_off[g0 + lane < g1 ? g0 + lane : g1] - t0;
        }
        // graph gl of the tile (wave-uniform): its id and its rows [n0, n1) inside the tile
        auto tile_graph_at = [&](int gl, int& n0, int& n1) {
            const int gph = a.list ? a.list[g0 + gl] : g0 + gl;
            if (gl < 63) {
                n0 = __builtin_amdgcn_readlane(my_noff, gl);
                n1 = gl + 1 < g1 - g0 ? __builtin_amdgcn_readlane(my_noff, gl + 1) : rows;
            } else if (!a.list) {
                n0 = a.b.node_off[gph] - t0;
                n1 = a.b.node_off[gph + 1] - t0;
            } else {  // beyond the lanes' reach (a tile of more than 63 graphs of one or two nodes): count again
                n0 = 0;
                for (int i = 0; i < gl; i++) n0 += a.b.nums_of_nodes[a.list[g0 + i]];
                n1 = n0 + a.b.nums_of_nodes[gph];
            }
            return gph;
        };
#pragma unroll 1
        for (int l = 0; l < DGN_L; l++) {
            const float oscale = s_bias[l * 128 + 112];
            float4_t acc[DGN_OT];
            // one K-step's barrier: this wave's pieces of the chunk have landed, then everybody's have -- and every wave is done with
            // the other slot, which the next chunk may now overwrite.  In K-step 0 it also orders the layer's s_ht stores before its reads.
            auto sync_step = [&](int k) {
                if (!DGNR_SKIP(2)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (!DGNR_SKIP(1) || k == 0) __syncthreads();
                if (DGNR_SKIP(2)) {}
                else if (k + 1 < DGN_FT_KS) issue_chunk(l, k + 1);
                else if (l + 1 < DGN_L) issue_chunk(l + 1, 0);
                if (l == 0 && k == 0 && has_next) issue_rec(ntile);  // every wave is done with this tile's records
            };
#pragma unroll
            for (int k = 0; k < DGN_FT_KS; k++) {
                sync_step(k);
                if (k == 0) {
#pragma unroll
                    for (int t = 0; t < DGN_OT; t++) {
                        const float4 bv = *reinterpret_cast<const float4*>(s_bias + l * 128 + 16 * t + 4 * g);
                        acc[t] = (float4_t){bv.x, bv.y, bv.z, bv.w};
                    }
                }
                // ---- aggregation of features 16 k .. 16 k + 15 on the matrix pipe (dgn_layer_mfma_kernel)
                const bool real = k < 6 || g == 0;
                const float4_t hv = hreg[k];
                const int frow = k < 6 ? 16 * k + j : 96 + (j & 3);
                const uint16_t* ah = s_ht_hi + frow * DGN_HT_STRIDE + 8 * g;
                const uint16_t* al = s_ht_lo + frow * DGN_HT_STRIDE + 8 * g;
                float4_t m1 = (float4_t){0.f, 0.f, 0.f, 0.f}, pp = m1;
#pragma unroll
                for (int sb = 0; sb < 4; sb++) {
                    if (blk[sb] && !DGNR_SKIP(4)) {
                        if constexpr (DGN_F16) {  // one product per aggregate and block
                            const ds_uint4_t fx = *reinterpret_cast<const ds_uint4_t*>(ah + 32 * sb);
                            m1 = DS_MFMA16(fx, b_one[sb], m1);
                            pp = DS_MFMA16(fx, b_eh[sb], pp);
                            continue;
                        }
                        const ds_uint4_t fh = *reinterpret_cast<const ds_uint4_t*>(ah + 32 * sb);
                        const ds_uint4_t fl = *reinterpret_cast<const ds_uint4_t*>(al + 32 * sb);
                        m1 = DS_MFMA16(fh, b_one[sb], m1);
                        pp = DS_MFMA16(fh, b_eh[sb], pp);
                        m1 = DS_MFMA16(fl, b_one[sb], m1);
                        pp = DS_MFMA16(fl, b_eh[sb], pp);
                        pp = DS_MFMA16(fh, b_el[sb], pp);
                    }
                }
                if (dups) {  // multiplicity > 1: the extra copies of a duplicate edge (the mask counted the first), from the caller's edge list --
                             // every copy after a row's first (u -> v) adds the split row of u (hi + lo) once more, as dgn_layer_mfma_kernel's walk
                             // over the CSR does (there in ascending u, here in list order: the same bits while a row repeats one source only)
                    const bool mine = ndup > 0 && real;
                    uint32_t seen0 = 0u, seen1 = 0u, seen2 = 0u, seen3 = 0u;
                    for (int gl = 0; gl < g1 - g0; gl++) {
                        int base, gend;
                        const int gph = tile_graph_at(gl, base, gend);
                        const int n = gend - base, e0 = a.b.edge_off[gph], ne = a.b.edge_off[gph + 1] - e0;
                        if (!__any(mine && lr >= base && lr < base + n)) continue;
                        for (int e = 0; e < ne; e++) {
                            int u = load_i32_rare(a.b.edge_list + 2 * (size_t)(e0 + e)), v = load_i32_rare(a.b.edge_list + 2 * (size_t)(e0 + e) + 1);
                            if (!((u >= 0) & (u < n) & (v >= 0) & (v < n))) { u = 0; v = 0; }  // as the tile build: a self-loop on the graph's node 0
                            u += base; v += base;
                            if (mine && v == lr && u < DGN_FT_ROWS) {
                                const uint32_t bit = 1u << (u & 31);
                                const int wi = u >> 5;
                                const uint32_t cur = wi == 0 ? seen0 : (wi == 1 ? seen1 : (wi == 2 ? seen2 : seen3));
                                if (cur & bit) {
                                    float eu = (s_eig[u] - eig_v) * wscale;  // the copy's (scaled) weight
                                    if constexpr (DGN_F16) eu = (float)(_Float16)eu;  // ... as the first copy's: rounded once
#pragma unroll
                                    for (int c = 0; c < 4; c++) {
                                        const int f = (k < 6 ? 16 * k : 96) + 4 * g + c;
                                        float x = (float)__builtin_bit_cast(_Float16, s_ht_hi[f * DGN_HT_STRIDE + u]);
                                        if constexpr (!DGN_F16) x += (float)__builtin_bit_cast(_Float16, s_ht_lo[f * DGN_HT_STRIDE + u]);
                                        m1[c] += x;
                                        pp[c] = __builtin_fmaf(x, eu, pp[c]);
                                    }
                                }
                                seen0 |= wi == 0 ? bit : 0u; seen1 |= wi == 1 ? bit : 0u; seen2 |= wi == 2 ? bit : 0u; seen3 |= wi == 3 ? bit : 0u;
                            }
                        }
                    }
                }
                // a1 = m1 / outdeg (x / 0 = 0), a2 = |(m2 - wsum h[v]) / abssum|   (node_embedding.cc:143-146); pp = m2 wscale
                float4 a1, a2;
                a1.x = m1.x * inv_dg; a1.y = m1.y * inv_dg; a1.z = m1.z * inv_dg; a1.w = m1.w * inv_dg;
                a2.x = fabsf(__builtin_fmaf(-wsum_s, hv.x, pp.x) * inv_abs_s);
                a2.y = fabsf(__builtin_fmaf(-wsum_s, hv.y, pp.y) * inv_abs_s);
                a2.z = fabsf(__builtin_fmaf(-wsum_s, hv.z, pp.z) * inv_abs_s);
                a2.w = fabsf(__builtin_fmaf(-wsum_s, hv.w, pp.w) * inv_abs_s);
                // lanes that hold K-slot padding (K-step 6, g != 0) contribute zeros.  Rows beyond the tile's last need no mask: their
                // adjacency bits, out-degree and sums are zero, so m1 = pp = 0 and a1 = a2 = +0 come out of the arithmetic above (with the
                // mask spelled out for every K-step hipcc kept an exec-mask region and eight v_mov per K-step: others-per-MFMA is what
                // this kernel is bound by, tools/coissue6.hip)
                if (!real) { a1 = make_float4(0.f, 0.f, 0.f, 0.f); a2 = a1; }
                ds_uint4_t b_hi, b_lo = {0u, 0u, 0u, 0u};
                DGN_OPER2(a1.x, a1.y, b_hi.x, b_lo.x);
                DGN_OPER2(a1.z, a1.w, b_hi.y, b_lo.y);
                DGN_OPER2(a2.x, a2.y, b_hi.z, b_lo.z);
                DGN_OPER2(a2.z, a2.w, b_hi.w, b_lo.w);
                asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(vmax) : "v"(a1.x), "v"(a1.y));
                asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(vmax) : "v"(a1.z), "v"(a1.w));
                asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(vmax) : "v"(a2.x), "v"(a2.y));
                asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(vmax) : "v"(a2.z), "v"(a2.w));
                asm volatile("" : "+v"(vmax));
                // ---- dense update, K-step k: 21 MFMAs on the chunk in slot (l + k) & 1
                const char* wb = s_w + ((l + k) & 1) * DGN_CHUNK;
                if (DGNR_SKIP(8)) { acc[0].x += __builtin_bit_cast(float, b_hi.x ^ b_lo.y); continue; }
                if constexpr (DGN_F16) {  // single product: seven fragments, seven MFMAs, one per accumulator
                    ds_uint4_t f7[DGN_OT];
#pragma unroll
                    for (int t = 0; t < DGN_OT; t++) f7[t] = *reinterpret_cast<const ds_uint4_t*>(wb + t * 1024 + lane * 16);
#pragma unroll
                    for (int t = 0; t < DGN_OT; t++) acc[t] = DS_MFMA16(f7[t], b_hi, acc[t]);
                    continue;
                }
                ds_uint4_t ff[2][4];  // the fragments of the NEXT pair of output tiles are requested before this pair's MFMAs issue
#pragma unroll
                for (int i = 0; i < 4; i++) ff[0][i] = *reinterpret_cast<const ds_uint4_t*>(wb + i * 1024 + lane * 16);
#pragma unroll
                for (int t0_ = 0; t0_ < DGN_OT; t0_ += 2) {
                    const int n = t0_ + 1 < DGN_OT ? 2 : 1;
                    const int n2 = t0_ + 3 < DGN_OT ? 2 : 1;
                    if (t0_ + 2 < DGN_OT) {
#pragma unroll
                        for (int i = 0; i < 2 * n2; i++) ff[((t0_ >> 1) + 1) & 1][i] = *reinterpret_cast<const ds_uint4_t*>(wb + (((t0_ + 2) * 2) + i) * 1024 + lane * 16);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    const ds_uint4_t (&f)[4] = ff[(t0_ >> 1) & 1];
#pragma unroll
                    for (int i = 0; i < n; i++) acc[t0_ + i] = DS_MFMA16(f[2 * i], b_hi, acc[t0_ + i]);
#pragma unroll
                    for (int i = 0; i < n; i++) acc[t0_ + i] = DS_MFMA16(f[2 * i], b_lo, acc[t0_ + i]);
#pragma unroll
                    for (int i = 0; i < n; i++) acc[t0_ + i] = DS_MFMA16(f[2 * i + 1], b_hi, acc[t0_ + i]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // ---- epilogue: h' = h + relu(b + W0 a1 + W1 a2) in the registers (node_embedding.cc:176-181)
#pragma unroll
            // (only the padding columns 100 .. 111 of the last output tile are masked.  Rows beyond the tile's last are left to run: they
            // are nobody's source -- no adjacency bit names them -- so what they hold only has to stay finite, and relu(bias) does; the
            // readout pools the graphs' rows.  One v_cndmask per value less in six of seven tiles.)
            for (int t = 0; t < DGN_OT; t++) {
                const bool on = 16 * t + 4 * g < DGN_D;
                const float4_t rr = acc[t] * oscale;
                hreg[t] = (float4_t){on ? hreg[t].x + relu1(rr.x) : 0.f, on ? hreg[t].y + relu1(rr.y) : 0.f,
                                     on ? hreg[t].z + relu1(rr.z) : 0.f, on ? hreg[t].w + relu1(rr.w) : 0.f};
            }
            __syncthreads();  // every wave is done with the layer's s_ht
            // (the graphs' rows only: a row beyond the tile's last keeps the zeros the loader wrote into its s_ht column -- its registers
            // grow by relu(bias) per layer and are never read by anybody else, its column is read by every MFMA of the tile, beside zeros)
            if (l + 1 < DGN_L && valid) {
#pragma unroll
                for (int t = 0; t < DGN_OT; t++) put_row_piece(4 * t + g, hreg[t]);  // (ordered before the next layer's reads by its K-step 0 barrier)
            }
        }
        if (DGNR_SKIP(32)) {
            if (valid && g == 0 && j == 0 && wave == 0) a.out[g0] = hreg[0].x;
            __syncthreads();
            __syncthreads();
        } else {
            // ---- readout: h_4 as fp32 rows where s_ht was, then one wave per graph of the tile -- pool_mlp3_kernel's pooling order, the
            // head of dgn_head_wave.  The head's weights come into the two weight slots (idle since the layer's last barrier) while
            // the rows are written and pooled: read from L2 by the graph's own wave they cost 0.23 ms of a 2.04 ms launch.
            issue_head();
            float* s_rows = reinterpret_cast<float*>(s_all);
            if (valid) {
#pragma unroll
                for (int t = 0; t < DGN_OT; t++)
                    if (16 * t + 4 * g < DGN_D)
                        *reinterpret_cast<float4*>(s_rows + lr * DGN_D + 16 * t + 4 * g) = make_float4(hreg[t].x, hreg[t].y, hreg[t].z, hreg[t].w);
            }
            __syncthreads();  // every row of h_4 is in place
            if constexpr (RESIDENT_ROWS) {
                // h_4 of the tile's graphs, as the fp32 rows the pool is about to read (they stay until the barrier that ends the readout).
                // A graph's rows are contiguous in the tile and in the caller's batch: one contiguous run of float4 stores per graph, dealt
                // over the whole workgroup (the readout itself occupies five waves).  A bin-packed tile is a list of graphs: the run
                // starts at node_off[graph], not at t0 + the graph's first row in the tile.  Rows past the tile's end belong to no graph.
                for (int gl = 0; gl < g1 - g0; gl++) {
                    int n0, n1;
                    const int gph = tile_graph_at(gl, n0, n1);
                    if (n1 > DGN_FT_ROWS) n1 = DGN_FT_ROWS;
                    float4* dst = reinterpret_cast<float4*>(a.node_emb + (size_t)a.b.node_off[gph] * DGN_D);
                    const float4* srcr = reinterpret_cast<const float4*>(s_rows + n0 * DGN_D);
                    for (int i = (int)threadIdx.x; i < (n1 - n0) * DGN_C; i += 512) dst[i] = srcr[i];
                }
            }
            constexpr int RW = 5;  // waves that read out (a tile holds two or three graphs; the scratch below has room for five)
            const float* s_head = reinterpret_cast<const float*>(s_w);
            float* s_hg = s_rows + DGN_FT_ROWS * DGN_D + (wave < RW ? wave : 0) * 160;  // behind the rows: [0, 100) pooled row, [100, 150) first hidden layer
            float* s_o1 = s_hg + DGN_D;
            static_assert((DGN_FT_ROWS * DGN_D + RW * 160) * 4 <= 2 * DGN_HT_BYTES, "readout scratch behind the rows");
            const int half = lane >> 5, c = lane & 31;
            auto pool = [&](int gl) {  // mean over the rows of the tile's graph gl -> s_hg (even rows | odd rows, then the two halves); -> its id
                int n0, n1;
                const int gph = tile_graph_at(gl, n0, n1);
                float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c < DGN_C) {
                    int v = n0 + half;
                    for (; v + 6 < n1; v += 8) {  // (four rows in flight; added in row order)
                        float4 x[4];
#pragma unroll
                        for (int i = 0; i < 4; i++) x[i] = *reinterpret_cast<const float4*>(s_rows + (v + 2 * i) * DGN_D + 4 * c);
#pragma unroll
                        for (int i = 0; i < 4; i++) { sum.x += x[i].x; sum.y += x[i].y; sum.z += x[i].z; sum.w += x[i].w; }
                    }
                    for (; v < n1; v += 2) {
                        const float4 x = *reinterpret_cast<const float4*>(s_rows + v * DGN_D + 4 * c);
                        sum.x += x.x; sum.y += x.y; sum.z += x.z; sum.w += x.w;
                    }
                }
                sum.x += __shfl_down(sum.x, 32, 64); sum.y += __shfl_down(sum.y, 32, 64);
                sum.z += __shfl_down(sum.z, 32, 64); sum.w += __shfl_down(sum.w, 32, 64);
                if (half == 0 && c < DGN_C) {
                    const float n = (float)(n1 - n0);
                    s_hg[4 * c + 0] = sum.x / n; s_hg[4 * c + 1] = sum.y / n;
                    s_hg[4 * c + 2] = sum.z / n; s_hg[4 * c + 3] = sum.w / n;
                }
                __builtin_amdgcn_wave_barrier();
                if constexpr (RESIDENT_EMB || RESIDENT_ROWS) {  // the pooled row the head is about to read, as it stands in LDS: 25 lanes, one float4 each
                    if ((RESIDENT_EMB || a.emb != nullptr) && lane < DGN_C) reinterpret_cast<float4*>(a.emb + (size_t)gph * DGN_D)[lane] = *reinterpret_cast<const float4*>(s_hg + 4 * lane);
                }
                return gph;
            };
            auto head = [&](int gi) {
                const float p = dgn_head_wave(s_hg, s_o1, s_head, 50, s_head + DGN_HEAD_W2, 25, lane < 50 ? s_head[DGN_HEAD_B1 + lane] : 0.0f,
                                              lane < 25 ? s_head[DGN_HEAD_B2 + lane] : 0.0f, lane < 25 ? s_head[DGN_HEAD_W3 + lane] : 0.0f, lane);
                if (lane == 0) a.out[gi] = s_head[DGN_HEAD_B3] + p;
                __builtin_amdgcn_wave_barrier();
            };
            int gl = wave, gi = 0;
            const bool have = wave < RW && gl < g1 - g0;
            if (have) gi = pool(gl);  // the wave's first graph is pooled while the head block travels
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // every wave's pieces of the head have landed
            if (have) {
                head(gi);
                for (gl += RW; gl < g1 - g0; gl += RW) { gi = pool(gl); head(gi); }
            }
            __syncthreads();  // the slots are the next tile's again (its first chunk request is its first statement)
        }
        if (!has_next) break;
        tile = ntile;
    }
    if constexpr (DGN_F16) vmax = __builtin_fmaxf(vmax, hmax);
    if (__any(!(vmax < 6.0e4f)) && !DGNR_SKIP(63)) {  // (a timing variant's garbage must not send the engine to the exact kernels)
        if (lane == 0) atomicOr(a.range_flag, 1);
    }
}

// host: W [100][2][100] (out, block, in), b [100] -> DGN_FT_LAYER_BYTES in the feature-major K order of dgn_layer_fused_kernel
#ifndef FG_RESIDENT_KERNEL_TU  // (host side: the model's own translation unit only)
// f16 (FLOWGNN_NUMERIC_F16): the stream of the single-product kernels -- the hi halves r(W s) alone (round to nearest even), [k][t] x 1 KiB,
// with the same bias block and 1 / scale behind them: DGN_F16_LAYER_BYTES
static void dgn_pack_fused_layer(const float* W, const float* b, uint8_t* out, bool f16 = false) {
    const int frags = f16 ? 1 : 2;
    const size_t bias_off = f16 ? DGN_F16_LAYER_BYTES - 512 : (size_t)DGN_FT_BIAS;
    std::memset(out, 0, f16 ? DGN_F16_LAYER_BYTES : DGN_FT_LAYER_BYTES);
    float m = 0.0f;
    for (size_t i = 0; i < (size_t)DGN_D * 2 * DGN_D; i++) m = std::fmax(m, std::fabs(W[i]));
    const float sc = (m > 0.0f && std::isfinite(m)) ? std::ldexp(1.0f, -std::ilogb(m)) : 1.0f;
    for (int k = 0; k < DGN_FT_KS; k++)
        for (int t = 0; t < DGN_OT; t++)
            for (int lane = 0; lane < 64; lane++) {
                const int i = lane & 15, gk = lane >> 4, o = 16 * t + i;
                uint8_t* f = out + (size_t)((k * DGN_OT + t) * frags) * 1024;
                for (int e = 0; e < 8; e++) {
                    const int feat = 16 * k + 4 * gk + (e & 3), blk = e >> 2;
                    const float v = (o < DGN_D && feat < DGN_D) ? W[((size_t)o * 2 + blk) * DGN_D + feat] * sc : 0.0f;
                    const _Float16 hi = (_Float16)v;
                    const _Float16 lo = (_Float16)(v - (float)hi);
                    std::memcpy(f + lane * 16 + e * 2, &hi, 2);
                    if (!f16) std::memcpy(f + 1024 + lane * 16 + e * 2, &lo, 2);
                }
            }
    for (int x = 0; x < 16 * DGN_OT; x++) {
        const float bb = x < DGN_D ? b[x] * sc : 0.0f;
        std::memcpy(out + bias_off + (size_t)x * 4, &bb, 4);
    }
    const float os = 1.0f / sc;
    std::memcpy(out + bias_off + 112 * 4, &os, 4);
}

class DgnModel : public Model {
public:
    ~DgnModel() override { free_all(); }
    int emb_dim() const override { return DGN_D; }
    int scratch_dim() const override { return 2 * DGN_D; }
    int aggregate_dim() const override { return qmode_ ? 0 : 2 * DGN_D; }  // fixed-point modes have no float aggregation kernel
    bool has_edge_attr() const override { return false; }
    int num_weight_tensors() const override { return 9; }
    bool weights_ready() const override { return ready_; }

    // host tensors (DGN/src/dcl.h:81-90): atom tables [9][119][100], layer W [4][100][200], b [4][100],
    // FC0 w [50][100] b [50], FC1 w [25][50] b [25], FC2 w [1][25] b [1]
    int set_numeric_mode(int mode) override {  // mode 1 = "the reference's own format": ap_fixed<16,3> for DGN (DGN/src/dcl.h:54-55)
        // mode 2 (FLOWGNN_NUMERIC_F16): the engine lets it through for flowgnn_set_model_numeric_mode alone
        if (mode != 0 && mode != 1 && mode != 2) return 8;
        qmode_ = mode == 1;
        f16_ = mode == 2;
        return 0;
    }

    int set_weights(const float* const* t) override {
        {   // ap_fixed<16,3> copies of every tensor for the bit-faithful mode (modelq.hip)
            static const size_t elems[9] = {9 * 119 * 100, 4 * 100 * 200, 4 * 100, 50 * 100, 50, 25 * 50, 25, 25, 1};
            if (int rc = q_.upload_all(9, t, elems, 13)) return rc;
        }
        // The reference indexes a dense [9][119][100] table (DGN/src/load_inputs.cc:124-137), but a feature k only takes values
        // below its cardinality (validated on the device): the 173 rows that can be addressed are gathered into the compact
        // [173][100] table the other models use (row = offset_k + value), which fits LDS (69 KB) -- the encoder then reads its nine
        // rows per node from LDS instead of L2 (0.37 -> 0.13 ms for 2^15 hep10k graphs).
        static const int nd_card[ND_FEATURE] = {119, 4, 12, 12, 10, 6, 6, 2, 2}, nd_off[ND_FEATURE] = {0, 119, 123, 135, 147, 157, 163, 169, 171};
        std::vector<float> v_emb((size_t)ND_FEATURE_TOTAL * DGN_D);
        for (int k = 0; k < ND_FEATURE; k++)
            for (int f = 0; f < nd_card[k]; f++)
                memcpy(&v_emb[(size_t)(nd_off[k] + f) * DGN_D], t[0] + ((size_t)k * DGN_TBL + f) * DGN_D, sizeof(float) * DGN_D);
        std::vector<float> v_w0(t[3], t[3] + 50 * 100), v_b0(t[4], t[4] + 50), v_w1(t[5], t[5] + 25 * 50), v_b1(t[6], t[6] + 25),
            v_w2(t[7], t[7] + 25), v_b2(t[8], t[8] + 1);
        std::vector<float> wf_all, wt_all, bp_all;
        std::vector<uint8_t> split_all, fused_all;
        std::vector<uint8_t> fused16_all((size_t)DGN_L * DGN_F16_LAYER_BYTES);  // beside them the single-product streams (FLOWGNN_NUMERIC_F16)
        std::vector<float> Wb((size_t)DGN_D * DGN_D), zero(DGN_D, 0.0f);
        for (int l = 0; l < DGN_L; l++) {
            const float* W = t[1] + (size_t)l * DGN_D * 2 * DGN_D;  // [out][2][in]
            std::vector<float> wf2, wt2;
            std::vector<float> bp;
            for (int b = 0; b < 2; b++) {
                for (int o = 0; o < DGN_D; o++)
                    for (int i = 0; i < DGN_D; i++) Wb[(size_t)o * DGN_D + i] = W[((size_t)o * 2 + b) * DGN_D + i];
                std::vector<float> wf, wt, bpp;
                pack_dense100(Wb.data(), b == 0 ? t[2] + (size_t)l * DGN_D : zero.data(), DGN_D, DGN_OT, wf, wt, bpp);
                wf2.insert(wf2.end(), wf.begin(), wf.end());
                wt2.insert(wt2.end(), wt.begin(), wt.end());
                if (b == 0) bp = bpp;
            }
            wf_all.insert(wf_all.end(), wf2.begin(), wf2.end());
            wt_all.insert(wt_all.end(), wt2.begin(), wt2.end());
            bp_all.insert(bp_all.end(), bp.begin(), bp.end());
            const size_t off = split_all.size();
            split_all.resize(off + dense200_split_bytes(DGN_OT));
            pack_dense200_split(W, t[2] + (size_t)l * DGN_D, DGN_D, DGN_OT, split_all.data() + off);
            const size_t foff = fused_all.size();
            fused_all.resize(foff + DGN_FT_LAYER_BYTES);
            dgn_pack_fused_layer(W, t[2] + (size_t)l * DGN_D, fused_all.data() + foff);
            dgn_pack_fused_layer(W, t[2] + (size_t)l * DGN_D, fused16_all.data() + (size_t)l * DGN_F16_LAYER_BYTES, true);
        }
        int rc;
        if ((rc = upload(&d_split_, split_all))) return rc;
        if ((rc = upload(&d_fused_, fused_all))) return rc;
        if ((rc = upload(&d_fused16_, fused16_all))) return rc;
        if ((rc = upload(&d_emb_, v_emb))) return rc;
        if ((rc = upload(&d_wf_, wf_all))) return rc;
        if ((rc = upload(&d_wt_, wt_all))) return rc;
        if ((rc = upload(&d_bp_, bp_all))) return rc;
        if ((rc = upload(&d_w0_, v_w0))) return rc;
        if ((rc = upload(&d_b0_, v_b0))) return rc;
        if ((rc = upload(&d_w1_, v_w1))) return rc;
        if ((rc = upload(&d_b1_, v_b1))) return rc;
        if ((rc = upload(&d_w2_, v_w2))) return rc;
        if ((rc = upload(&d_b2_, v_b2))) return rc;
        {   // the resident kernel's head reads w1 / w2 transposed (lane = output unit)
            std::vector<float> w1t(100 * 50), w2t(50 * 25);
            for (int o = 0; o < 50; o++)
                for (int i = 0; i < 100; i++) w1t[i * 50 + o] = v_w0[o * 100 + i];
            for (int o = 0; o < 25; o++)
                for (int i = 0; i < 50; i++) w2t[i * 25 + o] = v_w1[o * 50 + i];
            std::vector<float> head(DGN_HEAD_BYTES / 4, 0.0f);
            std::copy(w1t.begin(), w1t.end(), head.begin());
            std::copy(w2t.begin(), w2t.end(), head.begin() + DGN_HEAD_W2);
            std::copy(v_b0.begin(), v_b0.end(), head.begin() + DGN_HEAD_B1);
            std::copy(v_b1.begin(), v_b1.end(), head.begin() + DGN_HEAD_B2);
            std::copy(v_w2.begin(), v_w2.end(), head.begin() + DGN_HEAD_W3);
            head[DGN_HEAD_B3] = v_b2[0];
            if ((rc = upload(&d_head_, head))) return rc;
        }
        ready_ = true;
        return 0;
    }

    // DGN/src/host_load.cc:11-149: nine atom tables packed at 0, 11900, 12300, 13500, 14700, 15700, 16300, 16900,
    // 17100 into a [9][119][100] array; layer l at 17300 + 20100 l; head at 97700 ...
    int load_weights_dir(const char* dir) override {
        const char* f = "dgn_ep1_noBN_dim100.weights.all.bin";
        static const int card[9] = {119, 4, 12, 12, 10, 6, 6, 2, 2};
        static const size_t toff[9] = {0, 11900, 12300, 13500, 14700, 15700, 16300, 16900, 17100};
        std::vector<float> emb((size_t)9 * DGN_TBL * DGN_D, 0.0f), lw((size_t)4 * 20000), lb(400), w0(5000), b0(50), w1(1250),
            b1(25), w2(25), b2(1);
        int rc;
        for (int k = 0; k < 9; k++)
            if ((rc = read_floats(dir, f, toff[k], (size_t)card[k] * 100, &emb[(size_t)k * DGN_TBL * DGN_D]))) return rc;
        for (int l = 0; l < DGN_L; l++) {
            const size_t base = 17300 + 20100 * (size_t)l;
            if ((rc = read_floats(dir, f, base, 20000, &lw[(size_t)l * 20000]))) return rc;
            if ((rc = read_floats(dir, f, base + 20000, 100, &lb[l * 100]))) return rc;
        }
        if ((rc = read_floats(dir, f, 97700, 5000, w0.data()))) return rc;
        if ((rc = read_floats(dir, f, 102700, 50, b0.data()))) return rc;
        if ((rc = read_floats(dir, f, 102750, 1250, w1.data()))) return rc;
        if ((rc = read_floats(dir, f, 104000, 25, b1.data()))) return rc;
        if ((rc = read_floats(dir, f, 104025, 25, w2.data()))) return rc;
        if ((rc = read_floats(dir, f, 104050, 1, b2.data()))) return rc;
        const float* t[9] = {emb.data(), lw.data(), lb.data(), w0.data(), b0.data(), w1.data(), b1.data(), w2.data(), b2.data()};
        return set_weights(t);
    }

    // row tiles + (edge_scalar: the batch has an edge) eig1[src_e] per CSR entry of the standalone aggregation kernel, once per batch pass
    int prepare_aggregate(DeviceBatch& db, bool edge_scalar, Profiler& prof, hipStream_t s) {
        const int n = db.b.n_tot;
        if (int rc = make_tile_bounds(tiles_, db.b.node_off, db.b.num_graphs, n, tile_nominal_, tile_slack_, s)) return rc;
        if (edge_scalar) {
            if (int rc = esc_.reserve((size_t)db.b.e_tot)) return rc;
            ProfScope p(prof, "edge_scalar", s);
            DgnAggPolicy::Params prm{db.node_eigen, db.csr.out_deg, nullptr};
            edge_scalar_kernel<DgnAggPolicy><<<grid_for(db.b.e_tot, 256, 256 * 8), 256, 0, s>>>(prm, db.csr.src, esc_.p, db.b.e_tot);
        }
        agg_ready_ = true;
        return 0;
    }

    void launch_aggregate(const DeviceBatch& db, const float* hin, hipStream_t s) {
        DgnAggPolicy::Params prm{db.node_eigen, db.csr.out_deg, esc_.p};
        launch_tiled_aggregate<DgnAggPolicy>(prm, hin, db.scratch, db.csr, nullptr, db.b.n_tot, tiles_.p, tile_nominal_, s);
    }

    // fused layer kernel (dgn_layer_fused_kernel): whole graphs packed into tiles of <= 128 rows / 2 560 in-edges by flowgnn_set_batch
    void graph_tile_limits(int& rows, int& edges) const override {
        rows = fused_ ? DGN_FT_ROWS : 0;
        edges = fused_ ? DGN_FT_EDGES : 0;
    }

    // which kernels the next forward of this batch runs: decided in dgn_plan.h, from these values and nothing else
    DgnPlanInput plan_input() const {
        DgnPlanInput in;
        in.fused = fused_; in.split = split_; in.mfma_agg = mfma_agg_; in.fold_readout = fold_readout_; in.rowinfo_direct = rowinfo_direct_;
        in.resident = resident_; in.binpack = binpack_;
        in.qmode = qmode_; in.keep_h = keep_h_; in.exact = exact_; in.f16 = f16_;
        return in;
    }
    DgnPlan plan(const DeviceBatch& db) const {
        DgnPlanInput in = plan_input();
        in.nonempty = db.b.n_tot > 0; in.eigen = db.node_eigen != nullptr;
        in.tiles = db.gtiles.ok && db.gtiles.n_tiles > 0; in.fill = db.gtiles.fill; in.bp_lists = db.gtiles.bp_tiles > 0;
        in.edges = db.b.e_tot > 0; in.job_n = db.job_n; in.job_e = db.job_e; in.csr_built = db.csr_built;
        in.emb = db.emb != nullptr; in.node_emb = db.node_emb != nullptr;
        return dgn_plan(in);
    }
    bool needs_csr(const DeviceBatch& db) const override { return plan(db).needs_csr; }
    bool wants_packed_tile_lists() const override { return dgn_wants_packed_tile_lists(plan_input()); }

    // two launches per step: per-row records from the caller's arrays, then everything else
    int forward_resident(DeviceBatch& db, const DgnPlan& plan, Profiler& prof, hipStream_t s) {
        if (int rc = rec_.reserve(((size_t)db.b.n_tot + DGN_FT_ROWS) * DGN_REC_DW)) return rc;  // (a tile's DMA reads 128 records whatever its rows)
        // bin-packed tile lists when flowgnn_set_batch made them (option dgn_binpack): fewer, fuller tiles of the same graphs
        const GraphTiles::Tiles t = db.gtiles.tiles(plan.bin_packed);
        {
            ProfScope p(prof, "dgn_tile_build", s);
            dgn_rowinfo_kernel<true><<<t.n_tiles, 256, 0, s>>>(db.b, t.row, t.graph, t.n_tiles, db.node_eigen, reinterpret_cast<uint32_t*>(rec_.p),
                                                               nullptr, db.csr.err, nullptr, t.list);
        }
        DgnResidentLaunch a;
        a.rec = reinterpret_cast<const uint32_t*>(rec_.p); a.table = d_emb_; a.wpk = plan.single_product ? d_fused16_ : d_fused_; a.head = d_head_;
        a.tile_row = t.row; a.tile_graph = t.graph; a.list = t.list; a.n_tiles = t.n_tiles;
        a.b = db.b;
        a.out = db.out; a.emb = db.emb; a.node_emb = db.node_emb; a.range_flag = db.range_flag;
        const int grid = t.n_tiles < 256 ? t.n_tiles : 256;  // persistent: one 8-wave workgroup per CU (157 KB of LDS)
        if (plan.single_product) {  // FLOWGNN_NUMERIC_F16: the single-product instances, in a slot of their own
            ProfScope p(prof, "dgn_resident_f16", s);
            switch (plan.instance) {
            case DgnResidentInstance::Rows: launch_dgn_resident_f16_rows(a, grid, s); break;
            case DgnResidentInstance::Emb: launch_dgn_resident_f16_emb(a, grid, s); break;
            case DgnResidentInstance::Default: launch_dgn_resident_f16_default(a, grid, s); break;
            }
        } else {
            ProfScope p(prof, "dgn_resident", s);
            switch (plan.instance) {
            case DgnResidentInstance::Rows: launch_dgn_resident_rows(a, grid, s); break;  // the row-storing instance, embeddings or not
            case DgnResidentInstance::Emb: launch_dgn_resident_emb(a, grid, s); break;
            case DgnResidentInstance::Default: launch_dgn_resident_default(a, grid, s); break;
            }
        }
        db.final_h = 0;
        db.h_valid = false;  // no per-node tensor leaves the kernel: flowgnn_get_h repeats the pass on the per-layer kernels
        return 0;
    }

    int forward(DeviceBatch& db, Profiler& prof, hipStream_t s) override {
        const int n = db.b.n_tot;
        if (n <= 0) return 0;
        if (!db.node_eigen) return 1;
        const DgnPlan plan = this->plan(db);
        agg_ready_ = false;  // tiles_ / esc_ are rebuilt where the plan prepares the two-kernel layer; every other pass leaves none
        if (plan.path == DgnPath::FixedPoint) return dgnq_forward(q_, db, prof, s);
        db.h_valid = true;
        if (plan.path == DgnPath::Resident) return forward_resident(db, plan, prof, s);
        {
            ProfScope p(prof, "atom_encoder", s);
            atom_encoder_kernel<DGN_D><<<atom_encoder_grid(n, DGN_C), 512, 0, s>>>(db.b.node_feature, d_emb_, db.h[0], n, db.csr.err);
        }
        if (plan.prepare_aggregate)  // the fused layer takes eig1[src] from its own LDS tile: only the two-kernel layer needs these
            if (int rc = prepare_aggregate(db, plan.edge_scalar, prof, s)) return rc;
        int cur = 0;
        // matrix-pipe path without a CSR of this batch: the in-edge pass (adjacency masks, wsum, abssum, out-degrees) from the caller's
        // edge list, once per forward
        if (plan.rowinfo_from_edge_list) {
            if (int rc = rowinfo_.reserve((size_t)n * 8)) return rc;
            if (int rc = dupflag_.reserve(1)) return rc;
            ProfScope p(prof, "dgn_rowinfo", s);
            FG_HIP_TRY(hipMemsetAsync(dupflag_.p, 0, sizeof(int), s));
            dgn_rowinfo_kernel<false><<<db.gtiles.n_tiles, 256, 0, s>>>(db.b, db.gtiles.row_start, db.gtiles.graph_start, db.gtiles.n_tiles, db.node_eigen,
                                                                        reinterpret_cast<uint32_t*>(rowinfo_.p), db.csr.out_deg, db.csr.err, dupflag_.p);
            // the layer kernels' correction walk for duplicate edges reads the CSR: built only if the pass found one (device-side test)
            launch_build_csr(db.b, db.csr, false, db.max_nodes, db.max_edges, s, dupflag_.p);
        }
        for (int l = 0; l < DGN_L; l++) {
            // (node embeddings: the last layer writes h_4 straight into the caller's buffer, and the readout pools it from there)
            float* const hn = (l == DGN_L - 1 && db.node_emb) ? db.node_emb : db.h[cur ^ 1];
            if (plan.fused_layers) {
                ProfScope p(prof, plan.single_product ? "dgn_layer_mfma_f16" : "dgn_layer_fused", s);
                const int grid = db.gtiles.n_tiles < 256 ? db.gtiles.n_tiles : 256;  // persistent: one 8-wave workgroup per CU (153 KB of LDS)
                // dense tiles (kNN graphs: 16 in-edges per row, a third of a graph's block filled): both aggregates as MFMAs with the
                // tile's adjacency; sparse ones (molecules, ~2 in-edges per row): the in-edge walk is cheaper than 20 MFMAs per K-step
                if (plan.mfma_aggregation) {
                    if (int rc = rowinfo_.reserve((size_t)n * 8)) return rc;
                    uint32_t* ri = reinterpret_cast<uint32_t*>(rowinfo_.p);
#define DGN_MFMA_LAUNCH(I, P)                                                                                                                 \
    dgn_layer_mfma_kernel<I, P><<<grid, 512, 0, s>>>(db.h[cur], hn, db.csr.row_ptr, db.csr.src, db.csr.out_deg, db.node_eigen,       \
                                                     d_fused_ + (size_t)l * DGN_FT_LAYER_BYTES, db.gtiles.row_start, db.gtiles.n_tiles,       \
                                                     db.range_flag, ablate_, ri, reinterpret_cast<const int2*>(ginfo_.p), pool_part_.p,      \
                                                     pool_cnt_.p)
                    // without a stored pass the first layer's launch makes and stores it (adjacency mask, wsum, abssum per row), the
                    // others load it; the last one keeps h' on chip and hands the readout per-wave partial sums (POOL) unless the rows
                    // are asked for
                    const bool pool = l == DGN_L - 1 && plan.pooled_last;
                    if (pool) {
                        if (int rc = ginfo_.reserve((size_t)n * 2)) return rc;
                        if (int rc = pool_part_.reserve((size_t)db.b.num_graphs * 8 * DGN_D)) return rc;
                        if (int rc = pool_cnt_.reserve((size_t)db.b.num_graphs)) return rc;
                        dgn_graph_info_kernel<<<(db.b.num_graphs + 255) / 256, 256, 0, s>>>(db.b.node_off, db.b.num_graphs,
                                                                                          reinterpret_cast<int2*>(ginfo_.p));
                    }
                    if (plan.single_product) {  // FLOWGNN_NUMERIC_F16: the same three instances as single products, on the hi-only stream
                        const DgnLayerMfmaLaunch a{db.h[cur], hn, db.csr.row_ptr, db.csr.src, db.csr.out_deg, db.node_eigen,
                                                   d_fused16_ + (size_t)l * DGN_F16_LAYER_BYTES, db.gtiles.row_start, db.gtiles.n_tiles, db.range_flag,
                                                   ablate_, ri, reinterpret_cast<const int2*>(ginfo_.p), pool_part_.p, pool_cnt_.p};
                        launch_dgn_layer_mfma_f16(a, (l == 0 && plan.first_layer_makes_rowinfo) ? 1 : 2, pool, grid, s);
                    } else
                    if (l == 0 && plan.first_layer_makes_rowinfo) DGN_MFMA_LAUNCH(1, false); else if (pool) DGN_MFMA_LAUNCH(2, true); else DGN_MFMA_LAUNCH(2, false);
#undef DGN_MFMA_LAUNCH
                    cur ^= 1;
                    continue;
                }
                dgn_layer_fused_kernel<<<grid, 512, 0, s>>>(db.h[cur], hn, db.csr.row_ptr, db.csr.src, db.csr.out_deg, db.node_eigen,
                                                            d_fused_ + (size_t)l * DGN_FT_LAYER_BYTES, db.gtiles.row_start, db.gtiles.n_tiles,
                                                            db.range_flag, ablate_);
                cur ^= 1;
                continue;
            }
            {
                ProfScope p(prof, "dgn_aggregate", s);
                launch_aggregate(db, db.h[cur], s);
            }
            {
                ProfScope p(prof, "dgn_dense", s);
                const int waves = (int)ceil_div_ll(n, 16);
                if (plan.split_dense) {
                    const long long wgs = ceil_div_ll(n, 256);
                    dense200_res_relu_split_kernel<DGN_OT><<<(int)(wgs < 256 ? wgs : 256), 1024, 0, s>>>(
                        db.scratch, db.h[cur], hn, d_split_ + (size_t)l * dense200_split_bytes(DGN_OT), n, DGN_D, db.range_flag);
                } else
                dgn_dense_kernel<<<(waves + 3) / 4, 256, 0, s>>>(db.scratch, db.h[cur], hn,
                                                                  d_wf_ + (size_t)l * 2 * DGN_OT * 6 * 64 * 4,
                                                                  d_wt_ + (size_t)l * 2 * DGN_OT * 64, d_bp_ + (size_t)l * DGN_OT * 16, n);
            }
            cur ^= 1;
        }
        db.final_h = cur;
        db.h_valid = !plan.pooled_last && !db.node_emb;  // pooled: h[cur] was never written; flowgnn_get_h repeats the pass with the rows kept
        // the readout: from the last layer's per-wave partial sums, or from its rows; with the pooled rows stored too, or not
        using Readout = void (*)(const float*, const int*, const int*, const float*, const float*, const float*, const float*, const float*, const float*,
                                 float*, int, float*);
        static const Readout readout[2][2] = {{dgn_pool_part_mlp3_kernel<true, true>, dgn_pool_part_mlp3_kernel<false, true>},
                                              {dgn_pool_part_mlp3_kernel<true>, dgn_pool_part_mlp3_kernel<false>}};  // [!emb_readout][!pooled_last]
        const float* const rows = plan.pooled_last ? pool_part_.p : db.node_emb ? db.node_emb : db.h[cur];
        {
            ProfScope p(prof, "pool_mlp3", s);
            readout[!plan.emb_readout][!plan.pooled_last]<<<grid_for(db.b.num_graphs, 4, 256 * 4), 256, 0, s>>>(
                rows, plan.pooled_last ? pool_cnt_.p : nullptr, db.b.node_off, d_w0_, d_b0_, d_w1_, d_b1_, d_w2_, d_b2_, db.out, db.b.num_graphs, db.emb);
        }
        return 0;
    }

    void configure(const Options& o) override {
        tile_nominal_ = o.i("tile_nominal") > 0 ? o.i("tile_nominal") : kTileNominal;  // <= 0 / < 0: back to the model's defaults
        tile_slack_ = o.i("tile_slack") >= 0 ? o.i("tile_slack") : kTileSlack;
        split_ = o.i("dgn_mfma") != 32;
        fused_ = o.on("dgn_fused");
        mfma_agg_ = o.i("dgn_mfma_agg");
        fold_readout_ = o.on("dgn_fold_readout");
        rowinfo_direct_ = o.on("dgn_rowinfo_direct");
        resident_ = o.i("dgn_resident");
        binpack_ = o.on("dgn_binpack");
        ablate_ = FG_ABLATE(o.i("dgn_ablate"));
        agg_ready_ = false;
    }
    void set_exact(bool on) override { exact_ = on; }
    void set_keep_h(bool on) override { keep_h_ = on; }

    int aggregation_only(DeviceBatch& db, int layer, hipStream_t s) override {
        if (qmode_) return 8;  // FLOWGNN_ERR_UNSUPPORTED: the fixed-point forward never builds the float kernels' inputs (tiles, h rows)
        if (layer < 0 || layer >= DGN_L) return 1;
        if (!agg_ready_) {  // the last forward ran the fused layers
            Profiler none;
            if (int rc = prepare_aggregate(db, db.b.e_tot > 0, none, s)) return rc;
        }
        launch_aggregate(db, db.h[db.final_h], s);
        return 0;
    }

private:
    void free_all() {
        float** ptrs[] = {&d_emb_, &d_wf_, &d_wt_, &d_bp_, &d_w0_, &d_b0_, &d_w1_, &d_b1_, &d_w2_, &d_b2_, &d_head_};
        for (auto p : ptrs)
            if (*p) { (void)hipFree(*p); *p = nullptr; }
        esc_.release();
        tiles_.release();
        rowinfo_.release();
        rec_.release();
        ginfo_.release();
        dupflag_.release();
        pool_cnt_.release();
        pool_part_.release();
        q_.release();
        if (d_split_) { (void)hipFree(d_split_); d_split_ = nullptr; }
        if (d_fused_) { (void)hipFree(d_fused_); d_fused_ = nullptr; }
        if (d_fused16_) { (void)hipFree(d_fused16_); d_fused16_ = nullptr; }
    }
    bool ready_ = false;
    bool qmode_ = false;  // flowgnn_set_numeric_mode(FLOWGNN_NUMERIC_Q6_10): ap_fixed<16,3> arithmetic
    bool f16_ = false;    // flowgnn_set_model_numeric_mode(e, FLOWGNN_MODEL_DGN, FLOWGNN_NUMERIC_F16): the single-product kernels (dgn_f16.hip)
    QPack q_;
    GrowBufI tiles_;  // graph-aligned tile starts of the resident batch (tile_bounds_kernel)
    static constexpr int kTileNominal = 64, kTileSlack = 64;  // the model's defaults of the options tile_nominal / tile_slack
    int tile_nominal_ = kTileNominal, tile_slack_ = kTileSlack;
    // dgn_mfma=32 keeps the dense update on the fp32 matrix pipe (dgn_dense_kernel)
    bool split_ = true;
    // dgn_fused=0 keeps aggregation and dense update as two kernels per layer (A/B measurements, the aggregation roofline probe)
    bool agg_ready_ = false;  // tiles_ / esc_ describe the batch of the last forward
    GrowBufI rowinfo_;   // dgn_layer_mfma_kernel: 32 B per row of layer-independent in-edge pass results
    GrowBufI dupflag_;           // dgn_rowinfo_kernel: set on the device when the batch has duplicate edges
    bool rowinfo_direct_ = true;
    GrowBufI rec_;       // dgn_resident_kernel: 48 B per row (dgn_rowinfo_kernel<true>)
    int resident_ = 1;   // dgn_resident
    bool binpack_ = true;  // dgn_binpack: the resident kernel walks bin-packed tile lists (GraphTiles::bp_*)
    float* d_head_ = nullptr;  // the resident kernel's readout: head weights transposed + biases in one block (DGN_HEAD_BYTES)
    GrowBufI ginfo_, pool_cnt_;  // POOL form of the last layer: (graph, position) per node; partial rows per graph
    GrowBuf pool_part_;          //   [G][8][100] per-wave partial sums of h_4
    bool fold_readout_ = true, keep_h_ = false;
    int mfma_agg_ = -1;  // dgn_mfma_agg: 1 = aggregation on the matrix pipe (dgn_layer_mfma_kernel), 0 = in-edge walk, -1 = by density
    int ablate_ = 0;  // development aid (-DFLOWGNN_DEV builds only, option dgn_ablate): per-phase timing (scripts/dev/pna_ablate.sh)
    bool fused_ = true;
    uint8_t* d_fused_ = nullptr;  // feature-major weights of the fused layer kernel
    uint8_t* d_fused16_ = nullptr;  // the same as hi halves alone (FLOWGNN_NUMERIC_F16)
    bool exact_ = false;
    uint8_t* d_split_ = nullptr;
    GrowBuf esc_;
    float *d_emb_ = nullptr, *d_wf_ = nullptr, *d_wt_ = nullptr, *d_bp_ = nullptr, *d_w0_ = nullptr, *d_b0_ = nullptr,
          *d_w1_ = nullptr, *d_b1_ = nullptr, *d_w2_ = nullptr, *d_b2_ = nullptr;
};

Model* make_dgn_model() { return new DgnModel(); }
#endif  // FG_RESIDENT_KERNEL_TU

#ifdef FG_RESIDENT_KERNEL_TU
}  // namespace
#endif
#if DGN_SINGLE_PRODUCT && !defined(FG_RESIDENT_EMB_TU) && !defined(FG_RESIDENT_ROWS_TU)
// dgn_f16.hip: the per-layer matrix-pipe kernel's single-product instances
void launch_dgn_layer_mfma_f16(const DgnLayerMfmaLaunch& a, int info, bool pool, int grid, hipStream_t s) {
#define DGN_MFMA_F16_LAUNCH(I, P)                                                                                                            \
    dgn_layer_mfma_kernel<I, P><<<grid, 512, 0, s>>>(a.h, a.hout, a.row_ptr, a.src, a.out_deg, a.eig4, a.wpk, a.tile_row, a.n_tiles, a.range_flag, \
                                                     a.ablate, a.rowinfo, a.ginfo, a.pool_part, a.pool_cnt)
    if (info == 1) DGN_MFMA_F16_LAUNCH(1, false); else if (pool) DGN_MFMA_F16_LAUNCH(2, true); else DGN_MFMA_F16_LAUNCH(2, false);
#undef DGN_MFMA_F16_LAUNCH
}
#endif
// this translation unit's instance of dgn_resident_kernel, under the launcher's name that goes with it
#if DGN_SINGLE_PRODUCT && defined(FG_RESIDENT_EMB_TU)
void launch_dgn_resident_f16_emb(
#elif DGN_SINGLE_PRODUCT && defined(FG_RESIDENT_ROWS_TU)
void launch_dgn_resident_f16_rows(
#elif DGN_SINGLE_PRODUCT
void launch_dgn_resident_f16_default(
#elif defined(FG_RESIDENT_EMB_TU)
void launch_dgn_resident_emb(
#elif defined(FG_RESIDENT_ROWS_TU)
void launch_dgn_resident_rows(
#else
void launch_dgn_resident_default(
#endif
    const DgnResidentLaunch& a, int grid, hipStream_t s) {
    dgn_resident_kernel<<<grid, 512, 0, s>>>(DgnResidentArgs{a});
}

}  // namespace fg
