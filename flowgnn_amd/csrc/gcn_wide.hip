// GCN at OGB's default width (emb_dim 300): flowgnn_set_model_emb_dim(e, FLOWGNN_EMB_DIM_OGB) on a GCN engine.  DESIGN.md section 4.18.
//
// The model of gcn.hip's header with D in place of 100 (x_l = W_l a_l + b_l is ONE D x D product per layer):
//   x_0     = b_0 + W_0 h0, h0[v] = sum_{k<9} NodeEmb[off_k + feat_k(v)]
//   m_l[v]  = sum_{(u->v)} dinv[u] dinv[v] relu(x_l[u] + ecomb_l[code_e]), CSR order; dinv[i] = outdeg(i) > 0 ? 1/sqrt(outdeg(i)+1) : 0
//   pre_l   = BN_l(m_l + relu(x_l + root_l) / (outdeg + 1)), BN eval mode with sqrt(var + 2^-10), folded to one scale and one shift
//   a_{l+1} = relu(pre_l), x_{l+1} = W_{l+1} a_{l+1} + b_{l+1} (l < 4); readout: pool(pre_4), graph_pred_linear
//
// A model object of its own beside GcnModel, as GinWideModel is beside GinModel: one launch per stage, a tile is a run of rows.
//   x_0        the first product is linear in the nine looked-up rows: W_0 is applied to the 173-row table once (set_weights, in double)
//              and x_0 is the wide atom encoder on that table with b_0 as a tenth row (gw_atom_encoder_vn_kernel) -- no dense launch
//   l = 0..3   gcw_layer_kernel<D>: the scheme of gcn_layer_fused_kernel<false> (gcn.hip) carried to this width the way gw_layer_body
//              (gin_wide.hip) carried gin_layer_split_kernel.  A wave owns a 16-node column tile, walks its in-edges in CSR order into
//              the B-operand layout (lane (j, g) holds features 16 q + 4 g + r, q < Q; pieces at or beyond column D stay zero), loads
//              the node's own row after the walk, applies root, 1 / (deg + 1), the folded BatchNorm and ReLU in registers, splits with
//              DS_SPLIT2 and runs x_{l+1} as three f16 MFMAs per product.  K is padded with zero weights to whole K-steps: no fp32 tail.
//              The split weights (T output tiles x KS K-steps x hi/lo KiB) do not fit LDS: they stream L2 -> LDS by LDS-DMA as chunks of
//              TPC whole output tiles into two distinct LDS objects; s_waitcnt vmcnt(0) + a workgroup barrier per step, nothing counted.
//              A chunk's output tiles are stored as soon as its MFMAs are done, so TPC accumulators are live, not T.  The combined edge
//              table and the three epilogue vectors have LDS of their own beside the two buffers (the budget: GcwDims).
//   l = 4      gcw_final_kernel<D>: the walk and the epilogue without ReLU and without a product; rows pre_4
//   readout    GwReadout (wide_common.h), the one GinWideModel::forward ends in; set_weights packs with wide_common.h's gw_pack_tile,
//              gw_transpose and gw_edge_combos (DESIGN.md section 4.21 says what is shared and what is not)
// a beyond the f16 range raises *range_flag; the engine then repeats the pass with set_exact(true): gcw_aggregate_kernel (the same
// CSR order, the same FMAs, the same epilogue, one lane per node and float4 piece) and gw_dense_f32_kernel<D, D> once per stage.
//
// OGB's virtual node at this width (gcn-virtual; flowgnn_set_gcn_virtual_node_dim): the definition of
// gcn_ogbvn.h with D = 300.  The row the vector is added to and pooled over, a_l = relu(pre_{l-1}), exists in gcw_layer_kernel's
// registers alone, so the add and the per-graph sums are in that kernel's VN instance (gcw_layer_vn_kernel), as section 4.15 put them
// into gcn_layer_fused_kernel:
//   layer 0    vn_0 = E is a constant: b_0' = b_0 + W_0 E on the host, in double -- the encoder's tenth row, no new encoder kernel
//   t_0        gcw_vn_t0_kernel: sum_v h_0[v] + (n + 1) E from the unprojected table (this path never forms h_0), and node -> graph
//   s = 0..3   behind the walk a lane adds its pieces of vn_{s+1}[g(node)], in front of the range tracking and the split; s < 3: a
//              segmented scan along the 16 lanes of a tile, 16 columns at a time, leaves the partial rows of xin_{s+1}, one per
//              (16-node tile, graph) at slot graph + tile (gcn_ogbvn.h's rule); gcw_vn_t_kernel adds a graph's slots in order and vn
//   update     gin_wide.hip's gw_vn_update_kernel on the G rows t, its blob and its launcher (gin_wide_vn.h)
// The exact re-run adds and pools on the scratch rows between gcw_aggregate_kernel and the dense launch (gin_wide.hip's two kernels).
//
// OGB's residual=True and JK="sum" (flowgnn_set_model_jk_residual).  The rows OGB adds are the PRE-linear ones,
// x_l = h_l (+ vn_l[g]), which this path never stores: with either flag on they travel in up to two [N][D] buffers of the model's, as a
// second row stream through the EXT instances of the bodies (gcn_wide_body.h; the kernels and their launchers: gcn_wide_jk.hip).
//   x_0        one more launch of gw_atom_encoder_vn_kernel, on the UNPROJECTED table, tenth row E (virtual node) or zeros
//   s = 0..3   behind the walk: a += x_s (residual), the virtual node's add and partial rows as they are, then x_{s+1} = a is stored
//              (residual: the next stage's addend) and added to the running sum (JK sum)
//   s = 4      h_5 = pre_4 (+ x_4) to the ping-pong buffer, the sum (+ h_5) to the rows the readout pools
//   update     vn_{l+1} = vn_l + relu(..) under the residual (launch_gw_vn_update's vn_prev)
// With both flags off none of it exists: forward() takes the branches it took, and no launch comes from the new file.
//
// FLOWGNN_NUMERIC_F16 at this width (flowgnn_set_model_numeric_mode_dim): stages 0..3 run gcn_wide_f16.hip's
// kernels (one rounding of a and of W s to f16, one MFMA per product) on a hi-only stream that set_weights packs beside the split one
// whatever the mode is; stage 4, the virtual node's update, the readout and the exact re-run are the ones above.
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "gcn_ogbvn.h"
#include "gcn_wide_body.h"  // GcwDims, gcw_walk, gcw_step, gcw_vn_add_partials and the layer kernel's body, which gcn_wide_jk.hip instantiates as well (section 4.25)
#include "gcn_wide_f16.h"   // FLOWGNN_NUMERIC_F16 (section 4.27): the hi-only stream's layout and the launcher of gcn_wide_f16.hip's kernels
#include "gcn_wide_jk.h"    // flowgnn_set_model_jk_residual (section 4.25): the launchers of gcn_wide_jk.hip's instances
#include "gin_wide_jk.h"    // ... and the exact re-run's element-wise add (launch_gw_add_rows)
#include "gin_wide_vn.h"
#include "wide_common.h"

namespace fg {
namespace {

// (the depth: GcnWideModel::layers_, 5 unless flowgnn_set_num_layers said otherwise -- DESIGN.md section 4.30; no kernel knows it)

// dinv[src_e] per CSR entry (edge_scalar_kernel, device_common.h), the per-layer path's policy of gcn.hip restated: GcnAggPolicy
// itself lives in gcn.hip's translation units
struct GcwScalarPolicy {
    struct Params { const int* out_deg; };
    __device__ static float src_scalar(const Params& p, int u) {
        const int d = p.out_deg[u];
        return d > 0 ? 1.0f / sqrtf((float)(d + 1)) : 0.0f;
    }
};

// slots of the partial rows: gcn_ogbvn_part_floats's rule (slot = graph + tile) with rows of D floats
inline size_t gcw_vn_part_floats(int num_graphs, long long n_tot, int d) { return ((size_t)num_graphs + (size_t)((n_tot + 15) / 16)) * (size_t)d; }

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_layer_kernel(const float* __restrict__ x, float* __restrict__ xout,
                                                                  const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                  const uint8_t* __restrict__ ecode, const float* __restrict__ esc,
                                                                  const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                                  const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                  int n_tot, int* __restrict__ range_flag) {
    gcw_layer_body<D, false>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, GcwNoVnArgs{});
}

// the VN instance: stage s adds vn_{s+1} behind the walk and (s < 3) leaves the partial rows of xin_{s+1}
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_layer_vn_kernel(const float* __restrict__ x, float* __restrict__ xout,
                                                                     const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                     const uint8_t* __restrict__ ecode, const float* __restrict__ esc,
                                                                     const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                                     const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                     int n_tot, int* __restrict__ range_flag, GcwVnArgs vna) {
    gcw_layer_body<D, true>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, vna);
}

// t_0[g] = sum_{v in g} h_0[v] + (n + 1) E, h_0[v] the nine rows of the UNPROJECTED table in the encoder's order (every node's
// xin_0 = h_0 + E, and vn_0 = E once more): one lane per (graph, float4 piece), one chain per column in node order, so the value
// depends on the graph alone.  Also writes node_graph [N], for every forward, as gw_vn_pool_kernel does.  (A feature out of range
// reads row 0 here; the encoder of the same pass reports it.)
template <int D>
__global__ __launch_bounds__(256) void gcw_vn_t0_kernel(const int* __restrict__ node_feature, const float* __restrict__ table,
                                                        const int* __restrict__ node_off, const float* __restrict__ vn_e,
                                                        float* __restrict__ t, int* __restrict__ node_graph, int num_graphs) {
    constexpr int C = D / 4;
    const long long items = (long long)num_graphs * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const int gi = (int)(i / C);
        const int c = (int)(i - (long long)gi * C);
        const int n0 = node_off[gi], n1 = node_off[gi + 1];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int v = n0; v < n1; v++) {
            float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < ND_FEATURE; k++) {
                int f = node_feature[(long long)v * ND_FEATURE + k];
                if (f < 0 || f >= c_nd_card[k]) f = 0;
                const float4 w = reinterpret_cast<const float4*>(table)[(size_t)(c_nd_off[k] + f) * C + c];
                h.x += w.x; h.y += w.y; h.z += w.z; h.w += w.w;
            }
            acc.x += h.x; acc.y += h.y; acc.z += h.z; acc.w += h.w;
        }
        const float4 e = reinterpret_cast<const float4*>(vn_e)[c];
        const float m = (float)(n1 - n0 + 1);
        reinterpret_cast<float4*>(t)[i] =
            make_float4(__builtin_fmaf(e.x, m, acc.x), __builtin_fmaf(e.y, m, acc.y), __builtin_fmaf(e.z, m, acc.z), __builtin_fmaf(e.w, m, acc.w));
        for (int u = n0 + c; u < n1; u += C) node_graph[u] = gi;
    }
}

// t[g] = (the graph's partial rows, added in slot order) + vn[g]: one lane per (graph, float4 piece).  The rows are cut at the batch's
// 16-node tiles, so t is a function of the graph AND of where it stands in the batch (section 4.15)
template <int D>
__global__ __launch_bounds__(256) void gcw_vn_t_kernel(const float* __restrict__ part, const int* __restrict__ node_off,
                                                       const float* __restrict__ vn, float* __restrict__ t, int num_graphs) {
    constexpr int C = D / 4;
    const long long items = (long long)num_graphs * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const int gi = (int)(i / C);
        const int c = (int)(i - (long long)gi * C);
        const int n0 = node_off[gi], n1 = node_off[gi + 1];
        const long long lo = (long long)gi + (n0 >> 4), hi = (long long)gi + ((n1 - 1) >> 4);  // (a graph without nodes: hi < lo)
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n1 > n0)
            for (long long p = lo; p <= hi; p++) {
                const float4 x = reinterpret_cast<const float4*>(part)[(size_t)p * C + c];
                acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
            }
        const float4 w = reinterpret_cast<const float4*>(vn)[i];
        reinterpret_cast<float4*>(t)[i] = make_float4(acc.x + w.x, acc.y + w.y, acc.z + w.z, acc.w + w.w);
    }
}

// out[v] = pre_4[v]: stage 4, the walk and the epilogue without ReLU and without a product
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_final_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                  const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                  const uint8_t* __restrict__ ecode, const float* __restrict__ esc,
                                                                  const int* __restrict__ out_deg, const float* __restrict__ tab, int n_tot) {
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
    if (valid) {
        float* row = out + (size_t)node * D + 4 * g;
#pragma unroll
        for (int q = 0; q < M::Q; q++)
            if (16 * q + 4 * g < D) *reinterpret_cast<float4*>(row + 16 * q) = make_float4(a[4 * q + 0], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
    }
}

// ---------------------------------------------------------------- the exact (fp32) form of a stage: the same sums, plain FMAs
// a[v] = act(BN(m[v] + relu(x[v] + root) / (deg(v) + 1))), m[v] in CSR order; one lane per (node, float4 piece); tab in global memory
template <int D>
__global__ __launch_bounds__(256) void gcw_aggregate_kernel(const float* __restrict__ x, float* __restrict__ a, const int* __restrict__ row_ptr,
                                                            const int* __restrict__ src, const uint8_t* __restrict__ ecode,
                                                            const float* __restrict__ esc, const int* __restrict__ out_deg,
                                                            const float* __restrict__ tab, int n_tot, int relu_out) {
    using M = GcwDims<D>;
    constexpr int C = M::C;
    const float4* const ep = reinterpret_cast<const float4*>(tab + M::ECOMB_FLOATS);
    const long long items = (long long)n_tot * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const long long v = i / C;
        const int c = (int)(i - v * C);
        const int dv = out_deg[v];
        const float dinv_v = dv > 0 ? 1.0f / sqrtf((float)(dv + 1)) : 0.0f;
        const float idp1 = 1.0f / (float)(dv + 1);
        float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
        const int e1 = row_ptr[v + 1];
        for (int e = row_ptr[v]; e < e1; e++) {
            const float norm = esc[e] * dinv_v;
            const float4 xv = reinterpret_cast<const float4*>(x)[(size_t)src[e] * C + c];
            const float4 w = reinterpret_cast<const float4*>(tab)[(size_t)ecode[e] * C + c];
            m.x = __builtin_fmaf(norm, relu1(w.x + xv.x), m.x); m.y = __builtin_fmaf(norm, relu1(w.y + xv.y), m.y);
            m.z = __builtin_fmaf(norm, relu1(w.z + xv.z), m.z); m.w = __builtin_fmaf(norm, relu1(w.w + xv.w), m.w);
        }
        const float4 xs = reinterpret_cast<const float4*>(x)[(size_t)v * C + c];
        const float4 rt = ep[c], sc = ep[C + c], sh = ep[2 * C + c];
        float4 r;
        r.x = __builtin_fmaf(__builtin_fmaf(relu1(xs.x + rt.x), idp1, m.x), sc.x, sh.x);
        r.y = __builtin_fmaf(__builtin_fmaf(relu1(xs.y + rt.y), idp1, m.y), sc.y, sh.y);
        r.z = __builtin_fmaf(__builtin_fmaf(relu1(xs.z + rt.z), idp1, m.z), sc.z, sh.z);
        r.w = __builtin_fmaf(__builtin_fmaf(relu1(xs.w + rt.w), idp1, m.w), sc.w, sh.w);
        if (relu_out) { r.x = relu1(r.x); r.y = relu1(r.y); r.z = relu1(r.z); r.w = relu1(r.w); }
        reinterpret_cast<float4*>(a)[(size_t)v * C + c] = r;
    }
}

// w [D][D] (row-major [o][k], host), b [D] -> LAYER_BYTES of chunks and TAIL_FLOATS floats
template <int D>
void gcw_pack_layer(const float* w, const float* b, uint8_t* out, float* tail) {
    using M = GcwDims<D>;
    std::memset(out, 0, M::LAYER_BYTES);
    const float s = gw_pow2_scale(w, (size_t)D * D);
    for (int t = 0; t < M::T; t++) {
        uint8_t* tile = out + (size_t)(t / M::TPC) * M::CHUNK_BYTES + (size_t)(t % M::TPC) * M::TILE_BYTES;
        gw_pack_tile(w, D, D, 16 * t, s, 0, M::KS, tile, 2048);
    }
    for (int i = 0; i < M::TAIL_FLOATS; i++) tail[i] = 0.0f;
    for (int o = 0; o < D; o++) tail[o] = b[o] * s;
    tail[M::SCALE_AT] = 1.0f / s;
}

// FLOWGNN_NUMERIC_F16 (section 4.27): a layer's hi-only stream (GcwF16Dims, gcn_wide_f16.h) out of its split stream -- the hi
// fragments r(W s) as gcw_pack_layer left them, the lo fragments dropped; the tail is shared as it is
template <int D>
void gcw_pack_layer_f16(const uint8_t* split, uint8_t* out) {
    using M = GcwDims<D>;
    using F = GcwF16Dims<D>;
    static_assert(F::KS == M::KS && F::T == M::T && F::SCALE_AT == M::SCALE_AT, "the two streams cut a product into the same tiles, and share the tail");
    std::memset(out, 0, F::LAYER_BYTES);
    for (int t = 0; t < M::T; t++) {
        const uint8_t* tile = split + (size_t)(t / M::TPC) * M::CHUNK_BYTES + (size_t)(t % M::TPC) * M::TILE_BYTES;
        uint8_t* o = out + (size_t)(t / F::TPC) * F::CHUNK_BYTES + (size_t)(t % F::TPC) * F::TILE_BYTES;
        for (int ks = 0; ks < M::KS; ks++) std::memcpy(o + ks * 1024, tile + ks * 2048, 1024);
    }
}

template <int D>
class GcnWideModel : public Model {
    using M = GcwDims<D>;
    using F16 = GcwF16Dims<D>;

public:
    ~GcnWideModel() override { free_all(); }
    int emb_dim() const override { return D; }
    int scratch_dim() const override { return D; }
    bool has_edge_attr() const override { return true; }
    int num_weight_tensors() const override { return 11; }
    bool weights_ready() const override { return ready_; }
    void set_exact(bool on) override { exact_ = on; }
    int set_num_tasks(int t) override { return readout_.set_num_tasks(t, ready_); }
    // OGB's num_layer (flowgnn_set_num_layers, section 4.30): the bound of forward()'s stage loop and the leading dimension of the
    // per-layer tensors.  The weights are those of a depth: a change drops them, as a change of NUM_TASK does
    int set_num_layers(int n) override {
        if (n < FLOWGNN_MIN_NUM_LAYERS || n > FLOWGNN_MAX_NUM_LAYERS) return FLOWGNN_ERR_UNSUPPORTED;
        if (n != layers_) ready_ = false;
        layers_ = n;
        return 0;
    }
    // FLOWGNN_NUMERIC_F16 (flowgnn_set_model_numeric_mode_dim, section 4.27): stages 0..3 run gcn_wide_f16.hip's kernels on the hi-only
    // stream, which set_weights packs beside the split one whatever the mode is -- so the two calls come in either order
    int set_numeric_mode(int mode) override {
        if (mode != FLOWGNN_NUMERIC_F32 && mode != FLOWGNN_NUMERIC_F16) return FLOWGNN_ERR_UNSUPPORTED;
        f16_ = mode == FLOWGNN_NUMERIC_F16;
        return 0;
    }
    // OGB's virtual node (flowgnn_set_gcn_virtual_node_dim, section 4.19): the tensors' device form is gin_wide.hip's (gin_wide_vn.h) and
    // reaches forward() through DeviceBatch::ogb_vn; here the state, and E [D] for layer 0's folded bias -- in either order with
    // set_weights, and it holds across weight sets
    size_t ogb_vn_blob_bytes() const override { return gw_vn_blob_bytes(D, layers_ - 1); }
    void ogb_vn_pack(const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2, void* out) const override {
        gw_vn_blob_pack(D, layers_ - 1, vn_embedding, w1, b1, w2, b2, out);
    }
    int set_gcn_virtual_node(const float* vn_embedding) override {
        if (vn_embedding && gw_vn_blob_bytes(D, layers_ - 1) == 0) return 8;
        vn_on_ = vn_embedding != nullptr;
        if (vn_on_) vn_e_.assign(vn_embedding, vn_embedding + D);
        return ready_ ? upload_b0() : 0;
    }

    // host tensors, GcnModel's with D for 100 and the depth L for 5: node_emb[173][D], edge_emb[L][13][D], convs_weight[L][D][D],
    // convs_bias[L][D], root_emb[L][D], bn_weight/bias/mean/var[L][D], pred_w[NUM_TASK][D], pred_b[NUM_TASK]
    int set_weights(const float* const* t) override {
        const int L = layers_;
        const float *nemb = t[0], *eemb = t[1], *cw = t[2], *cb = t[3], *root = t[4], *bnw = t[5], *bnb = t[6], *bnm = t[7], *bnv = t[8],
                    *pw = t[9], *pb = t[10];
        std::vector<float> v_nemb(nemb, nemb + (size_t)ND_FEATURE_TOTAL * D);  // the virtual node's t_0 reads the unprojected table
        w0_.assign(cw, cw + (size_t)D * D);
        b0_.assign(cb, cb + D);
        std::vector<float> tab((size_t)L * M::TAB_FLOATS);
        std::vector<float> wt((size_t)(L - 1) * D * D), v_b(cb + D, cb + (size_t)L * D);  // the exact form: [K][O] copies of W_1 .. W_{L-1}
        std::vector<uint8_t> chunks((size_t)(L - 1) * M::LAYER_BYTES);
        std::vector<uint8_t> chunks16((size_t)(L - 1) * F16::LAYER_BYTES);
        std::vector<float> tails((size_t)(L - 1) * M::TAIL_FLOATS);
        for (int l = 0; l < L; l++) {
            float* tl = &tab[(size_t)l * M::TAB_FLOATS];
            gw_edge_combos(eemb + (size_t)l * ED_FEATURE_PER_LAYER * D, D, tl);
            float* e = tl + M::ECOMB_FLOATS;
            for (int d = 0; d < D; d++) {
                const double sv = std::sqrt((double)(bnv[l * D + d] + 1.0f / 1024.0f));
                const double scale = (double)bnw[l * D + d] / sv;
                e[0 * D + d] = root[l * D + d];
                e[1 * D + d] = (float)scale;
                e[2 * D + d] = (float)((double)bnb[l * D + d] - (double)bnm[l * D + d] * scale);
            }
            if (l == 0) continue;
            const float* W = cw + (size_t)l * D * D;
            gw_transpose(W, D, D, &wt[(size_t)(l - 1) * D * D]);
            gcw_pack_layer<D>(W, cb + (size_t)l * D, chunks.data() + (size_t)(l - 1) * M::LAYER_BYTES, tails.data() + (size_t)(l - 1) * M::TAIL_FLOATS);
            gcw_pack_layer_f16<D>(chunks.data() + (size_t)(l - 1) * M::LAYER_BYTES, chunks16.data() + (size_t)(l - 1) * F16::LAYER_BYTES);
        }
        // x_0 = b_0 + W_0 (sum_k NodeEmb[off_k + f_k]) = sum_k (W_0 NodeEmb[off_k + f_k]) + b_0: W_0 applied to the table once, in double
        // (GcnModel::set_weights); b_0 is the encoder's tenth row
        std::vector<float> proj((size_t)ND_FEATURE_TOTAL * D);
        for (int r = 0; r < ND_FEATURE_TOTAL; r++)
            for (int o = 0; o < D; o++) {
                double acc = 0.0;
                for (int i = 0; i < D; i++) acc += (double)cw[(size_t)o * D + i] * (double)nemb[(size_t)r * D + i];
                proj[(size_t)r * D + o] = (float)acc;
            }
        int rc;
        if ((rc = upload(&d_chunks_, chunks))) return rc;
        if ((rc = upload(&d_chunks16_, chunks16))) return rc;
        if ((rc = upload(&d_tails_, tails))) return rc;
        if ((rc = upload(&d_tab_, tab))) return rc;
        if ((rc = upload(&d_proj_, proj))) return rc;
        if ((rc = upload_b0())) return rc;
        if ((rc = upload(&d_nemb_, v_nemb))) return rc;
        if ((rc = upload(&d_zero_, std::vector<float>(D, 0.0f)))) return rc;
        if ((rc = upload(&d_wt_, wt))) return rc;
        if ((rc = upload(&d_b_, v_b))) return rc;
        if ((rc = readout_.upload_head(pw, pb))) return rc;
        ready_ = true;
        return 0;
    }

    // the reference's one file (GCN/src/host_load.cc) with this width in place of 100: node table at 0, layer l at 173 D + l (D^2 + 15 D)
    // (W, b, root, the 13 edge rows), BatchNorm l at 173 D + L (D^2 + 15 D) + l (4 D + 1), the head behind the last -- L the depth, the
    // reference's 5: every offset behind the layers moves with it, so a file of another depth is refused by its size, not read
    int load_weights_dir(const char* dir) override {
        const int L = layers_;
        const std::string name = "gcn_ep1_dim" + std::to_string(D) + ".weights.all.bin";
        const char* f = name.c_str();
        const size_t d = D, layer = d * d + 15 * d, bn0 = ND_FEATURE_TOTAL * d + L * layer, head = bn0 + L * (4 * d + 1);
        std::vector<float> nemb(ND_FEATURE_TOTAL * d), eemb(L * ED_FEATURE_PER_LAYER * d), cw(L * d * d), cb(L * d), root(L * d),
            bnw(L * d), bnb(L * d), bnm(L * d), bnv(L * d), pw((size_t)readout_.num_tasks * d), pb(readout_.num_tasks);
        int rc;
        if ((rc = check_layer_file(dir, f, nemb.size() + pw.size() + pb.size(), layer + 4 * d + 1, L))) return rc;
        if ((rc = read_floats(dir, f, 0, nemb.size(), nemb.data()))) return rc;
        for (int l = 0; l < L; l++) {
            const size_t base = ND_FEATURE_TOTAL * d + layer * (size_t)l;
            if ((rc = read_floats(dir, f, base, d * d, &cw[(size_t)l * d * d]))) return rc;
            if ((rc = read_floats(dir, f, base + d * d, d, &cb[l * d]))) return rc;
            if ((rc = read_floats(dir, f, base + d * d + d, d, &root[l * d]))) return rc;
            if ((rc = read_floats(dir, f, base + d * d + 2 * d, ED_FEATURE_PER_LAYER * d, &eemb[(size_t)l * ED_FEATURE_PER_LAYER * d]))) return rc;
            const size_t bn = bn0 + (4 * d + 1) * (size_t)l;  // 4 x D floats + one skipped counter per layer
            if ((rc = read_floats(dir, f, bn, d, &bnw[l * d]))) return rc;
            if ((rc = read_floats(dir, f, bn + d, d, &bnb[l * d]))) return rc;
            if ((rc = read_floats(dir, f, bn + 2 * d, d, &bnm[l * d]))) return rc;
            if ((rc = read_floats(dir, f, bn + 3 * d, d, &bnv[l * d]))) return rc;
        }
        if ((rc = read_floats(dir, f, head, pw.size(), pw.data()))) return rc;
        if ((rc = read_floats(dir, f, head + pw.size(), pb.size(), pb.data()))) return rc;
        const float* t[11] = {nemb.data(), eemb.data(), cw.data(), cb.data(), root.data(), bnw.data(), bnb.data(), bnm.data(), bnv.data(), pw.data(), pb.data()};
        return set_weights(t);
    }

    int forward(DeviceBatch& db, Profiler& prof, hipStream_t s) override {
        const int n = db.b.n_tot;
        if (n <= 0) return 0;
        const int G = db.b.num_graphs;
        const int L = layers_;  // (the depth: flowgnn_set_num_layers)
        const bool vn = db.ogb_vn != nullptr;
        if (vn != vn_on_) {
            set_last_error("flowgnn_run: the GCN model's virtual-node state and the engine's tensors disagree (flowgnn_set_gcn_virtual_node_dim)");
            return 8;
        }
        if (vn) {
            if (int rc = vn_t_.reserve((size_t)G * D)) return rc;
            if (int rc = vn_vec_[0].reserve((size_t)G * D)) return rc;
            if (int rc = vn_vec_[1].reserve((size_t)G * D)) return rc;
            if (int rc = node_graph_.reserve((size_t)n)) return rc;
            if (!exact_) {
                if (int rc = vn_part_.reserve(gcw_vn_part_floats(G, n, D))) return rc;
            } else {
                if (int rc = hid_.reserve((size_t)G * 2 * D)) return rc;
            }
        }
        // OGB's residual=True and JK="sum" (flowgnn_set_model_jk_residual, section 4.25): with either on, the fast path's stages are
        // gcn_wide_jk.hip's instances, under the slot of the ones they stand in for; in the default state nothing below differs
        const bool res_on = db.residual != 0, jk_on = db.jk == FLOWGNN_JK_SUM, ext_on = res_on || jk_on;
        if (res_on)
            if (int rc = res_.reserve((size_t)n * D)) return rc;
        if (jk_on)
            if (int rc = jk_.reserve((size_t)n * D)) return rc;
        if (int rc = readout_.reserve(db, exact_)) return rc;  // the attention readout (section 4.20): the gates [N] ...
        if (db.attn_pool && exact_)                    // ... and the exact form's hidden rows [N][2 D]
            if (int rc = hid_.reserve((size_t)(n > G ? n : G) * 2 * D)) return rc;
        if (db.b.e_tot > 0) {  // dinv[src_e] per CSR entry, once per pass, as on the 100-wide per-layer path
            if (int rc = esc_.reserve((size_t)db.b.e_tot)) return rc;
            ProfScope p(prof, "edge_scalar", s);
            GcwScalarPolicy::Params prm{db.csr.out_deg};
            edge_scalar_kernel<GcwScalarPolicy><<<grid_for(db.b.e_tot, 256, 256 * 8), 256, 0, s>>>(prm, db.csr.src, esc_.p, db.b.e_tot);
        }
        {
            ProfScope p(prof, "atom_encoder", s);  // x_0: nine rows of the projected table and b_0
            gw_atom_encoder_vn_kernel<D><<<grid_for((long long)n * M::C, 256, 256 * 8), 256, 0, s>>>(db.b.node_feature, d_proj_, db.h[0], n, db.csr.err, d_b0_);
        }
        if (ext_on) {  // x_0 = h_0 (+ E), the PRE-linear rows: the residual's first addend, or (JK sum alone) the sum's first term
            ProfScope p(prof, "gcn_wide_x0", s);
            gw_atom_encoder_vn_kernel<D><<<grid_for((long long)n * M::C, 256, 256 * 8), 256, 0, s>>>(db.b.node_feature, d_nemb_, res_on ? res_.p : jk_.p, n,
                                                                                                     db.csr.err, vn ? db.ogb_vn : d_zero_);
        }
        // the virtual node: vn_{l+1} (vn_vec_[l & 1]) is complete before stage l is launched -- vn_1 from t_0 here, vn_{l+2} behind stage l
        // (under the residual vn_{l+1} = vn_l + relu(..): the update's vn_prev, E with stride 0 for the first)
        if (vn) {
            {
                ProfScope p(prof, "gcn_wide_vn_t0", s);
                gcw_vn_t0_kernel<D><<<grid_for((long long)G * M::C, 256, 256 * 8), 256, 0, s>>>(db.b.node_feature, d_nemb_, db.b.node_off, db.ogb_vn, vn_t_.p,
                                                                                                node_graph_.p, G);
            }
            ProfScope p(prof, "gcn_wide_vn_update", s);
            if (int rc = launch_gw_vn_update(D, db.ogb_vn, L - 1, 0, vn_t_.p, vn_vec_[0].p, hid_.p, G, exact_, db.range_flag, res_on ? db.ogb_vn : nullptr, 0, s))
                return rc;
        }
        int cur = 0;
        for (int l = 0; l < L; l++) {
            const bool last = l == L - 1;
            // (node embeddings: the last stage writes pre_4 straight into the caller's buffer, and the readout reads it there)
            // (under JK sum the reverse: the rows the pool is taken over are the sum's, so the last stage's sum goes into the caller's
            // buffer and h_5 into the ping-pong buffer)
            float* const hn = (last && db.node_emb && !jk_on) ? db.node_emb : db.h[cur ^ 1];
            const float* tab = d_tab_ + (size_t)l * M::TAB_FLOATS;
            // the pre-linear rows (section 4.25): x_l in res_ (stage l rewrites it in place with x_{l+1}); the sum starts from x_0,
            // which the x_0 launch left in res_ when both flags are on and in jk_ itself otherwise
            float* const rres = res_on ? res_.p : nullptr;
            const float* const jk_in = !jk_on ? nullptr : (l == 0 && res_on) ? res_.p : jk_.p;
            float* const jk_out = !jk_on ? nullptr : (last && db.node_emb) ? db.node_emb : jk_.p;
            if (!exact_ && f16_ && !last) {  // FLOWGNN_NUMERIC_F16 (section 4.27): the four instances of gcn_wide_f16.hip, a slot of their own
                ProfScope p(prof, "gcn_wide_layer_f16", s);
                if (int rc = launch_gcw_layer_f16(D, db.h[cur], hn, db.csr.row_ptr, db.csr.src, db.csr.ecode, esc_.p, db.csr.out_deg, tab,
                                                  d_chunks16_ + (size_t)l * F16::LAYER_BYTES, d_tails_ + (size_t)l * M::TAIL_FLOATS, n, db.range_flag,
                                                  vn ? node_graph_.p : nullptr, vn ? vn_vec_[l & 1].p : nullptr,
                                                  vn && feeds_update(l) ? vn_part_.p : nullptr, rres, rres, jk_in, jk_out, s))
                    return rc;
            } else if (!exact_ && ext_on) {
                ProfScope p(prof, "gcn_wide_layer", s);
                int rc;
                if (!last)
                    rc = launch_gcw_layer_jk(D, db.h[cur], hn, db.csr.row_ptr, db.csr.src, db.csr.ecode, esc_.p, db.csr.out_deg, tab,
                                             d_chunks_ + (size_t)l * M::LAYER_BYTES, d_tails_ + (size_t)l * M::TAIL_FLOATS, n, db.range_flag,
                                             vn ? node_graph_.p : nullptr, vn ? vn_vec_[l & 1].p : nullptr,
                                             vn && feeds_update(l) ? vn_part_.p : nullptr, rres, rres, jk_in, jk_out, s);
                else
                    rc = launch_gcw_final_jk(D, db.h[cur], hn, db.csr.row_ptr, db.csr.src, db.csr.ecode, esc_.p, db.csr.out_deg, tab, n, rres, jk_in,
                                             jk_out, s);
                if (rc) return rc;
            } else if (!exact_) {
                ProfScope p(prof, "gcn_wide_layer", s);
                const int grid = (int)ceil_div_ll(n, GW_ROWS);
                if (!last && vn)
                    gcw_layer_vn_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(db.h[cur], hn, db.csr.row_ptr, db.csr.src, db.csr.ecode, esc_.p, db.csr.out_deg, tab,
                                                                          d_chunks_ + (size_t)l * M::LAYER_BYTES, d_tails_ + (size_t)l * M::TAIL_FLOATS,
                                                                          n, db.range_flag,
                                                                          GcwVnArgs{node_graph_.p, vn_vec_[l & 1].p, feeds_update(l) ? vn_part_.p : nullptr});
                else if (!last)
                    gcw_layer_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(db.h[cur], hn, db.csr.row_ptr, db.csr.src, db.csr.ecode, esc_.p, db.csr.out_deg, tab,
                                                                       d_chunks_ + (size_t)l * M::LAYER_BYTES, d_tails_ + (size_t)l * M::TAIL_FLOATS, n,
                                                                       db.range_flag);
                else
                    gcw_final_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(db.h[cur], hn, db.csr.row_ptr, db.csr.src, db.csr.ecode, esc_.p, db.csr.out_deg, tab, n);
            } else {
                ProfScope p(prof, "gcn_wide_layer_f32", s);
                gcw_aggregate_kernel<D><<<grid_for((long long)n * M::C, 256, 256 * 8), 256, 0, s>>>(
                    db.h[cur], last ? hn : db.scratch, db.csr.row_ptr, db.csr.src, db.csr.ecode, esc_.p, db.csr.out_deg, tab, n, last ? 0 : 1);
                // (the adds in the fast path's order: the residual, the virtual node's vector, the JK sum -- then the pool and the product)
                float* const rows = last ? hn : db.scratch;
                if (res_on)
                    if (int rc = launch_gw_add_rows(D, rows, rows, res_.p, D, n, s)) return rc;
                if (!last && vn)  // xin_{l+1} = a_{l+1} + vn_{l+1} on the scratch rows
                    if (int rc = launch_gw_vn_add(D, db.scratch, node_graph_.p, vn_vec_[l & 1].p, n, s)) return rc;
                if (jk_on)
                    if (int rc = launch_gw_add_rows(D, jk_out, jk_in, rows, D, n, s)) return rc;
                if (!last && res_on)  // x_{l+1}, the next stage's addend (behind the sum: at l = 0 jk_in is this buffer)
                    FG_HIP_TRY(hipMemcpyAsync(res_.p, db.scratch, (size_t)n * D * sizeof(float), hipMemcpyDeviceToDevice, s));
                if (!last && vn && feeds_update(l))  // ... and their per-graph sums
                    if (int rc = launch_gw_vn_pool(D, db.scratch, db.b.node_off, vn_vec_[l & 1].p, D, vn_t_.p, nullptr, G, s)) return rc;
                if (!last) launch_gw_dense_f32<D, D>(db.scratch, d_wt_ + (size_t)l * D * D, d_b_ + (size_t)l * D, hn, n, 0, s);
            }
            if (vn && feeds_update(l)) {  // t_{l+1} (the split form: from the partial rows stage l left) and vn_{l+2}
                if (!exact_) {
                    ProfScope p(prof, "gcn_wide_vn_t", s);
                    gcw_vn_t_kernel<D><<<grid_for((long long)G * M::C, 256, 256 * 8), 256, 0, s>>>(vn_part_.p, db.b.node_off, vn_vec_[l & 1].p, vn_t_.p, G);
                }
                ProfScope p(prof, "gcn_wide_vn_update", s);
                if (int rc = launch_gw_vn_update(D, db.ogb_vn, L - 1, l + 1, vn_t_.p, vn_vec_[(l + 1) & 1].p, hid_.p, G, exact_, db.range_flag,
                                                 res_on ? vn_vec_[l & 1].p : nullptr, res_on ? D : 0, s))
                    return rc;
            }
            cur ^= 1;
        }
        db.final_h = cur;
        db.h_valid = jk_on || !db.node_emb;
        return readout_.run(db, prof, s, db.node_emb ? db.node_emb : jk_on ? jk_.p : db.h[cur], exact_, hid_.p);
    }

private:
    // stage l (0 .. L - 2) adds vn_{l+1}; its rows xin_{l+1} feed update l + 1, which exists for l + 1 < L - 1 (at L = 2: for no stage)
    bool feeds_update(int l) const { return l + 1 < layers_ - 1; }
    // the encoder's tenth row: b_0, or with the virtual node on b_0' = b_0 + W_0 E, in double
    int upload_b0() {
        std::vector<float> b(b0_);
        if (vn_on_)
            for (int o = 0; o < D; o++) {
                double acc = (double)b0_[o];
                for (int i = 0; i < D; i++) acc += (double)w0_[(size_t)o * D + i] * (double)vn_e_[i];
                b[o] = (float)acc;
            }
        return upload(&d_b0_, b);
    }
    void free_all() {
        vn_t_.release();
        vn_vec_[0].release();
        vn_vec_[1].release();
        vn_part_.release();
        hid_.release();
        node_graph_.release();
        res_.release();
        jk_.release();
        float** ptrs[] = {&d_tails_, &d_tab_, &d_proj_, &d_b0_, &d_nemb_, &d_wt_, &d_b_, &d_zero_};
        for (auto p : ptrs)
            if (*p) { (void)hipFree(*p); *p = nullptr; }
        if (d_chunks_) { (void)hipFree(d_chunks_); d_chunks_ = nullptr; }
        if (d_chunks16_) { (void)hipFree(d_chunks16_); d_chunks16_ = nullptr; }
        esc_.release();
        readout_.release();
    }
    bool ready_ = false;
    bool exact_ = false;
    bool f16_ = false;  // flowgnn_set_model_numeric_mode_dim(FLOWGNN_NUMERIC_F16)
    int layers_ = FLOWGNN_NUM_LAYERS_DEFAULT;  // flowgnn_set_num_layers: L, what the per-layer buffers below were packed for while ready_
    GwReadout<D> readout_;         // the head's weights, NUM_TASK, the pooled rows and the gates (wide_common.h)
    uint8_t* d_chunks_ = nullptr;  // the weight streams of gcw_layer_kernel: W_1 .. W_{L-1}, LAYER_BYTES each
    uint8_t* d_chunks16_ = nullptr;  // FLOWGNN_NUMERIC_F16: the same L - 1 products as hi-only streams, F16::LAYER_BYTES each
    float* d_tails_ = nullptr;     // ... and per product b (pre-scaled, padded) and the output scale
    float* d_tab_ = nullptr;       // per layer: ecomb | root | BN scale | BN shift
    float *d_proj_ = nullptr, *d_b0_ = nullptr;  // W_0 applied to the node table, and b_0
    float *d_wt_ = nullptr, *d_b_ = nullptr;     // the exact form's W_1 .. W_{L-1} as [K][O], and b_1 .. b_{L-1}
    GrowBuf esc_;     // [E] dinv[src_e] in CSR order
    // OGB's virtual node (section 4.19)
    bool vn_on_ = false;              // flowgnn_set_gcn_virtual_node_dim is on (the tensors themselves: DeviceBatch::ogb_vn)
    std::vector<float> w0_, b0_, vn_e_;  // ... W_0, b_0 and E on the host, for b_0'
    float* d_nemb_ = nullptr;         // ... the unprojected node table [173][D] (gcw_vn_t0_kernel)
    GrowBuf vn_t_;                    // ... t [G][D], the update's input
    GrowBuf vn_vec_[2];               // ... vn_{l+1} and vn_{l+2} [G][D], alternating
    GrowBuf vn_part_;                 // ... the partial rows of xin (gcw_vn_part_floats)
    GrowBuf hid_;                     // ... the exact form's hidden rows of the update [G][2 D]
    GrowBufI node_graph_;             // ... node -> graph [N], written by the t_0 launch of every pass
    // OGB's residual and JK sum (section 4.25): the pre-linear rows, each reserved only while its flag is on; neither ping-pong buffer
    GrowBuf res_;                     // ... x_l [N][D], rewritten in place by stage l
    GrowBuf jk_;                      // ... the running sum of the rows [N][D]
    float* d_zero_ = nullptr;         // ... D zeros: the x_0 launch's tenth row without the virtual node
};

}  // namespace

Model* make_gcn_wide_model(int emb_dim) {
    if (emb_dim == 300) return new GcnWideModel<300>();  // FLOWGNN_EMB_DIM_OGB: the one instantiation
    return nullptr;
}

}  // namespace fg
