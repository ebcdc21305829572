// GIN at OGB's default width (emb_dim 300, hidden 600): flowgnn_set_emb_dim(e, FLOWGNN_EMB_DIM_OGB).  DESIGN.md section 4.16.
//
// A model of its own beside GinModel (gin.hip): the graph-resident kernel keeps 256 rows x 100 floats on chip and cannot be widened, so
// this width runs one launch per layer, where a tile is a run of consecutive rows and nothing depends on a graph fitting on chip.
//
// Layer kernel (gw_layer_kernel<D>, H = 2 D): the scheme of gin_layer_split_kernel (gin_split.hip) -- a wave owns one 16-node column
// tile, gathers a[v] = s_l h[v] + sum_e relu(h[src_e] + ecomb[code_e]) straight into the B-operand layout of the f16 matrix pipe, and
// runs both dense products as three f16 MFMAs per product (w_hi x_hi + w_hi x_lo + w_lo x_hi, fp32 accumulate, weights pre-scaled by a
// power of two and split on the host, activations split by DS_SPLIT2).  Per step it runs MLP1 of two hidden tiles and feeds them as ONE
// K-step of MLP2 into the T2 row accumulators: the C layout of one MFMA is the B layout of the next (the K permutation of
// dense_split.h), so the hidden layer never leaves the wave.  K is padded with zero weights (D -> 32 KS1, H -> 16 T1): no fp32 K tail.
// The weight stream (STEPS chunks per layer) goes L2 -> LDS by LDS-DMA, double buffered in two distinct LDS objects and shared by the
// eight waves of a 128-row workgroup; the only synchronisation is s_waitcnt vmcnt(0) + a workgroup barrier per step.
//   lane (j = lane & 15, g = lane >> 4); B operand of K-step ks, slot e (0..7): feature 16 (2 ks + (e >> 2)) + 4 g + (e & 3).
// Operands beyond the f16 range raise *range_flag; the engine then repeats the pass with set_exact(true), which runs the fp32 form of
// the layer (gw_aggregate_kernel + gw_dense_f32_kernel twice, plain FMAs, the same row order).
//
// OGB's virtual node at this width (flowgnn_set_ogb_virtual_node_dim): no launch rewrites the rows to add a
// vector.  x_0 = h_0 + E is formed by the encoder's VN instance, x_{l+1} = relu(layer l) + vn_{l+1}[g(v)] in the epilogue of the layer
// kernel's VN instance (vn_{l+1} depends on x_l alone, so it is complete before layer l is launched), t by gw_vn_pool_kernel (one read of
// the rows) and the update MLP by the layer kernel's own MLP on G "rows" t (gw_vn_update_kernel: the body with the gather compiled out).
//
// Where things live: this file has the layer's kernels, the virtual node's kernels and their three launchers
// (gin_wide_vn.h; forward() and gcn_wide.hip call the same ones), the weight stream's layout and the model object.  The readout, the
// fragment packer, the transpose, the edge table and the fp32 MLP launch are wide_common.h's, shared with gcn_wide.hip and wide_attn.hip.
// The layer kernel's body (GwDims, gw_step, gw_layer_body) is gin_wide_body.h's: gin_wide_jk.hip compiles it once more with OGB's
// residual=True and JK="sum" in the epilogue (flowgnn_set_jk_residual, section 4.24); forward() launches those instances while the
// setting is on and the ones below otherwise.
// FLOWGNN_NUMERIC_F16 at this width (flowgnn_set_numeric_mode_dim, section 4.22): the layer's two single-product kernels live in
// gin_wide_f16.hip behind gin_wide_f16.h's launcher; this file packs their hi-only weight stream and chooses between the launches.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "gin_wide_body.h"  // GwDims, gw_step and gw_layer_body: the layer kernel's body, which gin_wide_jk.hip instantiates as well (section 4.24)
#include "gin_wide_f16.h"  // FLOWGNN_NUMERIC_F16 at this width: the hi-only stream's layout and the launcher of gin_wide_f16.hip's kernels
#include "gin_wide_jk.h"  // flowgnn_set_jk_residual (section 4.24): the launchers of gin_wide_jk.hip's instances
#include "gin_wide_vn.h"  // the virtual node's launches, defined at the end of this file: forward() and gcn_wide.hip call them
#include "wide_common.h"  // GW_WAVES / GW_ROWS, gw_relu, the LDS-DMA issue, the encoder, pooling and fp32 dense kernels, the packer, the readout

namespace fg {
namespace {

// (the depth: GinWideModel::layers_, 5 unless flowgnn_set_num_layers said otherwise -- DESIGN.md section 4.30; no kernel knows it)

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_layer_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                 const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                 const uint8_t* __restrict__ ecode, const float* __restrict__ ecomb,
                                                                 const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                 int n_tot, int relu_out, float self_s, int* __restrict__ range_flag) {
    gw_layer_body<D, GW_PLAIN>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, relu_out, self_s, range_flag, nullptr, nullptr);
}

// the VN instance: x_{l+1}[v] = relu(layer l of x_l)[v] + vn_{l+1}[node_graph[v]] (always ReLU'd: every layer but the last)
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_layer_vn_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                    const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                    const uint8_t* __restrict__ ecode, const float* __restrict__ ecomb,
                                                                    const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                    int n_tot, float self_s, int* __restrict__ range_flag,
                                                                    const int* __restrict__ node_graph, const float* __restrict__ vn_add) {
    gw_layer_body<D, GW_VN>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, 1, self_s, range_flag, node_graph, vn_add);
}

// the update instance: vn_next[g] = relu(W2 relu(W1 t[g] + b1) + b2) for num_graphs "rows" t; a = fma(t, 1, 0) = t exactly
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_vn_update_kernel(const float* __restrict__ t, float* __restrict__ vn_next,
                                                                     const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                     int num_graphs, int* __restrict__ range_flag) {
    gw_layer_body<D, GW_UPDATE>(t, vn_next, nullptr, nullptr, nullptr, nullptr, wchunks, tailp, num_graphs, 1, 1.0f, range_flag, nullptr, nullptr);
}

// ---------------------------------------------------------------- the exact (fp32) form of the layer: the same sums, plain FMAs
// a[v] = fma(h[v], s_l, m[v]), m[v] the in-edge sum in CSR order; one lane per (node, float4 piece)
template <int D>
__global__ __launch_bounds__(256) void gw_aggregate_kernel(const float* __restrict__ h, float* __restrict__ a, const int* __restrict__ row_ptr,
                                                           const int* __restrict__ src, const uint8_t* __restrict__ ecode,
                                                           const float* __restrict__ ecomb, int n_tot, float self_s) {
    constexpr int C = D / 4;
    const long long items = (long long)n_tot * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const long long v = i / C;
        const int c = (int)(i - v * C);
        float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
        const int e1 = row_ptr[v + 1];
        for (int e = row_ptr[v]; e < e1; e++) {
            const float4 x = reinterpret_cast<const float4*>(h)[(size_t)src[e] * C + c];
            const float4 w = reinterpret_cast<const float4*>(ecomb)[(size_t)ecode[e] * C + c];
            m.x += relu1(w.x + x.x); m.y += relu1(w.y + x.y); m.z += relu1(w.z + x.z); m.w += relu1(w.w + x.w);
        }
        const float4 x = reinterpret_cast<const float4*>(h)[(size_t)v * C + c];
        reinterpret_cast<float4*>(a)[(size_t)v * C + c] =
            make_float4(__builtin_fmaf(x.x, self_s, m.x), __builtin_fmaf(x.y, self_s, m.y), __builtin_fmaf(x.z, self_s, m.z), __builtin_fmaf(x.w, self_s, m.w));
    }
}

// (gw_dense_f32_kernel, the atom encoder and gw_pool_rows_kernel at this width: wide_common.h)

// ---------------------------------------------------------------- OGB's virtual node at this width (section 4.17)
// t[g] = (the rows of graph g summed in node order, one chain per column as in gw_pool_rows_kernel) + vn[g]: one lane per (graph,
// float4 piece), four rows in flight, the adds in node order -- the value depends on the graph alone.  Reads the rows once, writes
// [G][D]; no atomics.  vn_stride (floats): D, or 0 for layer 0, where every graph's vector is E.  node_graph non-null (layer 0's
// launch): also writes the node -> graph array the VN layer instances and gw_vn_add_kernel read.
template <int D>
__global__ __launch_bounds__(256) void gw_vn_pool_kernel(const float* __restrict__ rows, const int* __restrict__ node_off,
                                                         const float* __restrict__ vn, int vn_stride, float* __restrict__ t,
                                                         int* __restrict__ node_graph, int num_graphs) {
    constexpr int C = D / 4;
    const long long items = (long long)num_graphs * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const int gi = (int)(i / C);
        const int c = (int)(i - (long long)gi * C);
        const int n0 = node_off[gi], n1 = node_off[gi + 1];
        const float4* p = reinterpret_cast<const float4*>(rows) + (size_t)n0 * C + c;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        int v = n0;
        for (; v + 3 < n1; v += 4, p += 4 * C) {
            const float4 x0 = p[0], x1 = p[C], x2 = p[2 * C], x3 = p[3 * C];
            acc.x += x0.x; acc.y += x0.y; acc.z += x0.z; acc.w += x0.w;
            acc.x += x1.x; acc.y += x1.y; acc.z += x1.z; acc.w += x1.w;
            acc.x += x2.x; acc.y += x2.y; acc.z += x2.z; acc.w += x2.w;
            acc.x += x3.x; acc.y += x3.y; acc.z += x3.z; acc.w += x3.w;
        }
        for (; v < n1; v++, p += C) {
            const float4 x = p[0];
            acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
        }
        const float4 w = reinterpret_cast<const float4*>(vn + (size_t)gi * vn_stride)[c];
        reinterpret_cast<float4*>(t)[i] = make_float4(acc.x + w.x, acc.y + w.y, acc.z + w.z, acc.w + w.w);
        if (node_graph)
            for (int u = n0 + c; u < n1; u += C) node_graph[u] = gi;
    }
}

// rows[v] += vn[node_graph[v]]: the exact (fp32) re-run's add on the dense kernel's output -- its speed is no goal
template <int D>
__global__ __launch_bounds__(256) void gw_vn_add_kernel(float* __restrict__ rows, const int* __restrict__ node_graph,
                                                        const float* __restrict__ vn, int n_tot) {
    constexpr int C = D / 4;
    const long long items = (long long)n_tot * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const long long v = i / C;
        const int c = (int)(i - v * C);
        const float4 w = reinterpret_cast<const float4*>(vn)[(size_t)node_graph[v] * C + c];
        float4 x = reinterpret_cast<float4*>(rows)[i];
        x.x += w.x; x.y += w.y; x.z += w.z; x.w += w.w;
        reinterpret_cast<float4*>(rows)[i] = x;
    }
}

// w1 [H][D], b1 [H], w2 [D][H], b2 [D] (row-major, host) -> LAYER_BYTES of chunks and TAIL_FLOATS floats
template <int D>
void gw_pack_layer(const float* w1, const float* b1, const float* w2, const float* b2, uint8_t* out, float* tail) {
    using M = GwDims<D>;
    std::memset(out, 0, M::LAYER_BYTES);
    const float s1 = gw_pow2_scale(w1, (size_t)M::H * D);
    const float s2 = gw_pow2_scale(w2, (size_t)D * M::H);
    for (int s = 0; s < M::STEPS; s++) {
        uint8_t* ck = out + (size_t)s * M::CHUNK_STRIDE;
        if (s < M::KS2)
            for (int tl = 0; tl < 2; tl++) {
                const int t = 2 * s + tl;
                gw_pack_tile(w1, M::H, D, 16 * t, s1, 0, M::KS1, ck + tl * 2048, 4096);
                for (int x = 0; x < 16; x++) {
                    const int o = 16 * t + x;
                    const float b = o < M::H ? b1[o] * s1 : 0.0f;
                    std::memcpy(ck + M::B1_OFF + tl * 64 + x * 4, &b, 4);
                }
            }
        if (s > 0)
            for (int t2 = 0; t2 < M::T2; t2++) gw_pack_tile(w2, D, M::H, 16 * t2, s2, s - 1, 1, ck + M::W2_OFF + t2 * 2048, 0);
    }
    for (int x = 0; x < M::TAIL_FLOATS; x++) tail[x] = 0.0f;
    for (int x = 0; x < D; x++) tail[x] = b2[x] * s1 * s2;
    tail[M::T2 * 16] = 1.0f / (s1 * s2);
}

// FLOWGNN_NUMERIC_F16 (section 4.22): a layer's hi-only stream (GwF16Dims, gin_wide_f16.h) out of its split stream -- the hi fragments
// r(W s) and the pre-scaled b1 as gw_pack_layer left them, the lo fragments dropped; the tail is shared as it is
template <int D>
void gw_pack_layer_f16(const uint8_t* split, uint8_t* out) {
    using M = GwDims<D>;
    using F = GwF16Dims<D>;
    static_assert(F::STEPS == M::STEPS && F::KS1 == M::KS1 && F::T2 == M::T2, "the two streams cut a layer into the same steps");
    std::memset(out, 0, F::LAYER_BYTES);
    for (int s = 0; s < M::STEPS; s++) {
        const uint8_t* ck = split + (size_t)s * M::CHUNK_STRIDE;
        uint8_t* o = out + (size_t)s * F::CHUNK_STRIDE;
        for (int f = 0; f < M::KS1 * 2; f++) std::memcpy(o + f * 1024, ck + f * 2048, 1024);
        for (int t2 = 0; t2 < M::T2; t2++) std::memcpy(o + F::W2_OFF + t2 * 1024, ck + M::W2_OFF + t2 * 2048, 1024);
        std::memcpy(o + F::B1_OFF, ck + M::B1_OFF, 2 * 16 * 4);
    }
}

// OGB's virtual node at this width (flowgnn_set_ogb_virtual_node_dim, section 4.17): the device form of the five tensors, a layout
// of this file's own (gin_ogbvn.h's is the 100-wide one).  In bytes, every part a multiple of 16:
//   E [D] floats | per update l (0 .. depth - 2): the weight stream of gw_pack_layer<D> (LAYER_BYTES) | its tail (TAIL_FLOATS floats)
//                                       | W1^T [D][H] | W2^T [H][D] | b1 [H] | b2 [D]     (the four fp32 parts: the exact form)
template <int D>
struct GwVnBlob {
    using M = GwDims<D>;
    static constexpr size_t E_BYTES = (size_t)D * 4;
    static constexpr size_t TAIL_OFF = M::LAYER_BYTES;
    static constexpr size_t W1T_OFF = TAIL_OFF + (size_t)M::TAIL_FLOATS * 4;
    static constexpr size_t W2T_OFF = W1T_OFF + (size_t)D * M::H * 4;
    static constexpr size_t B1_OFF = W2T_OFF + (size_t)M::H * D * 4;
    static constexpr size_t B2_OFF = B1_OFF + (size_t)M::H * 4;
    static constexpr size_t LAYER_STRIDE = B2_OFF + (size_t)D * 4;
    static constexpr size_t bytes(int n_updates) { return E_BYTES + (size_t)n_updates * LAYER_STRIDE; }
    static_assert(E_BYTES % 16 == 0 && TAIL_OFF % 16 == 0 && W1T_OFF % 16 == 0 && LAYER_STRIDE % 16 == 0, "the weight stream is read in 16-byte pieces");
};

// host tensors E [D], w1 [U][H][D], b1 [U][H], w2 [U][D][H], b2 [U][D], U = n_updates -> GwVnBlob<D>::bytes(U) bytes
template <int D>
void gw_vn_pack(int n_updates, const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2, uint8_t* out) {
    using B = GwVnBlob<D>;
    constexpr int H = 2 * D;
    std::memcpy(out, vn_embedding, B::E_BYTES);
    for (int l = 0; l < n_updates; l++) {
        uint8_t* o = out + B::E_BYTES + (size_t)l * B::LAYER_STRIDE;
        const float* W1 = w1 + (size_t)l * H * D;
        const float* W2 = w2 + (size_t)l * D * H;
        gw_pack_layer<D>(W1, b1 + (size_t)l * H, W2, b2 + (size_t)l * D, o, reinterpret_cast<float*>(o + B::TAIL_OFF));
        gw_transpose(W1, H, D, reinterpret_cast<float*>(o + B::W1T_OFF));
        gw_transpose(W2, D, H, reinterpret_cast<float*>(o + B::W2T_OFF));
        std::memcpy(o + B::B1_OFF, b1 + (size_t)l * H, (size_t)H * 4);
        std::memcpy(o + B::B2_OFF, b2 + (size_t)l * D, (size_t)D * 4);
    }
}

template <int D>
class GinWideModel : public Model {
    using M = GwDims<D>;
    using F16 = GwF16Dims<D>;
    static constexpr int H = M::H;

public:
    ~GinWideModel() override { free_all(); }
    int set_ogb_virtual_node(bool) override { return 0; }  // (the tensors: DeviceBatch::ogb_vn, in GwVnBlob's form)
    size_t ogb_vn_blob_bytes() const override { return GwVnBlob<D>::bytes(layers_ - 1); }
    void ogb_vn_pack(const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2, void* out) const override {
        gw_vn_pack<D>(layers_ - 1, vn_embedding, w1, b1, w2, b2, static_cast<uint8_t*>(out));
    }
    int emb_dim() const override { return D; }
    int scratch_dim() const override { return D; }
    bool has_edge_attr() const override { return true; }
    int num_weight_tensors() const override { return 8; }
    bool weights_ready() const override { return ready_; }
    void set_exact(bool on) override { exact_ = on; }
    // FLOWGNN_NUMERIC_F16 (flowgnn_set_numeric_mode_dim, section 4.22): the five layers run gin_wide_f16.hip's kernels on the hi-only
    // stream, which set_weights packs beside the split one whatever the mode is -- so the two calls come in either order
    int set_numeric_mode(int mode) override {
        if (mode != FLOWGNN_NUMERIC_F32 && mode != FLOWGNN_NUMERIC_F16) return FLOWGNN_ERR_UNSUPPORTED;
        f16_ = mode == FLOWGNN_NUMERIC_F16;
        return 0;
    }
    int set_num_tasks(int t) override { return readout_.set_num_tasks(t, ready_); }
    // OGB's num_layer (flowgnn_set_num_layers, section 4.30): the bound of forward()'s loop and the leading dimension of the per-layer
    // tensors.  The weights are those of a depth: a change drops them, as a change of NUM_TASK does
    int set_num_layers(int n) override {
        if (n < FLOWGNN_MIN_NUM_LAYERS || n > FLOWGNN_MAX_NUM_LAYERS) return FLOWGNN_ERR_UNSUPPORTED;
        if (n != layers_) ready_ = false;
        layers_ = n;
        return 0;
    }

    // host tensors, L = the depth: node_emb[173][D], edge_emb[L][13][D], w1[L][H][D], b1[L][H], w2[L][D][H], b2[L][D], pred_w[NUM_TASK][D], pred_b[NUM_TASK]
    int set_weights(const float* const* t) override {
        const int L = layers_;
        const float *nemb = t[0], *eemb = t[1], *w1 = t[2], *b1 = t[3], *w2 = t[4], *b2 = t[5], *pw = t[6], *pb = t[7];
        std::vector<float> v_nemb(nemb, nemb + (size_t)ND_FEATURE_TOTAL * D);
        std::vector<float> v_b1(b1, b1 + (size_t)L * H), v_b2(b2, b2 + (size_t)L * D);
        std::vector<float> ecomb((size_t)L * EDGE_COMBOS * D);
        std::vector<float> w1t((size_t)L * D * H), w2t((size_t)L * H * D);  // the exact form's [K][O] copies
        std::vector<uint8_t> chunks((size_t)L * M::LAYER_BYTES);
        std::vector<uint8_t> chunks16((size_t)L * F16::LAYER_BYTES);
        std::vector<float> tails((size_t)L * M::TAIL_FLOATS);
        for (int l = 0; l < L; l++) {
            gw_edge_combos(eemb + (size_t)l * ED_FEATURE_PER_LAYER * D, D, &ecomb[(size_t)l * EDGE_COMBOS * D]);
            const float* W1 = w1 + (size_t)l * H * D;
            const float* W2 = w2 + (size_t)l * D * H;
            gw_transpose(W1, H, D, &w1t[(size_t)l * D * H]);
            gw_transpose(W2, D, H, &w2t[(size_t)l * H * D]);
            gw_pack_layer<D>(W1, b1 + (size_t)l * H, W2, b2 + (size_t)l * D, chunks.data() + (size_t)l * M::LAYER_BYTES,
                             tails.data() + (size_t)l * M::TAIL_FLOATS);
            gw_pack_layer_f16<D>(chunks.data() + (size_t)l * M::LAYER_BYTES, chunks16.data() + (size_t)l * F16::LAYER_BYTES);
        }
        int rc;
        if ((rc = upload(&d_chunks_, chunks))) return rc;
        if ((rc = upload(&d_chunks16_, chunks16))) return rc;
        if ((rc = upload(&d_tails_, tails))) return rc;
        if ((rc = upload(&d_nemb_, v_nemb))) return rc;
        if ((rc = readout_.upload_head(pw, pb))) return rc;
        if ((rc = upload(&d_ecomb_, ecomb))) return rc;
        if ((rc = upload(&d_w1t_, w1t))) return rc;
        if ((rc = upload(&d_w2t_, w2t))) return rc;
        if ((rc = upload(&d_b1_, v_b1))) return rc;
        if ((rc = upload(&d_b2_, v_b2))) return rc;
        ready_ = true;
        return 0;
    }

    // the reference's file names (GIN/src/host_load.cc:24-58) with this width in place of 100
    int load_weights_dir(const char* dir) override {
        const int L = layers_;
        std::vector<float> w1((size_t)L * H * D), b1((size_t)L * H), w2((size_t)L * D * H), b2((size_t)L * D),
            nemb((size_t)ND_FEATURE_TOTAL * D), eemb((size_t)L * ED_FEATURE_PER_LAYER * D), pw((size_t)readout_.num_tasks * D), pb(readout_.num_tasks);
        const std::string sfx = "_dim" + std::to_string(D) + ".bin";
        int rc;
        if ((rc = read_layer_floats(dir, ("gin_ep1_mlp_1_weights" + sfx).c_str(), L, w1.size() / L, w1.data()))) return rc;
        if ((rc = read_layer_floats(dir, ("gin_ep1_mlp_1_bias" + sfx).c_str(), L, b1.size() / L, b1.data()))) return rc;
        if ((rc = read_layer_floats(dir, ("gin_ep1_mlp_2_weights" + sfx).c_str(), L, w2.size() / L, w2.data()))) return rc;
        if ((rc = read_layer_floats(dir, ("gin_ep1_mlp_2_bias" + sfx).c_str(), L, b2.size() / L, b2.data()))) return rc;
        if ((rc = read_floats(dir, ("gin_ep1_nd_embed" + sfx).c_str(), 0, nemb.size(), nemb.data()))) return rc;
        if ((rc = read_layer_floats(dir, ("gin_ep1_ed_embed" + sfx).c_str(), L, eemb.size() / L, eemb.data()))) return rc;
        if ((rc = read_floats(dir, ("gin_ep1_pred_weights" + sfx).c_str(), 0, pw.size(), pw.data()))) return rc;
        if ((rc = read_floats(dir, ("gin_ep1_pred_bias" + sfx).c_str(), 0, pb.size(), pb.data()))) return rc;
        const float* t[8] = {nemb.data(), eemb.data(), w1.data(), b1.data(), w2.data(), b2.data(), pw.data(), pb.data()};
        return set_weights(t);
    }

    int forward(DeviceBatch& db, Profiler& prof, hipStream_t s) override {
        const int n = db.b.n_tot;
        if (n <= 0) return 0;
        // OGB's virtual node (section 4.17): no launch rewrites the rows to add a vector -- x_0 = h_0 + E in the encoder, x_{l+1} in layer
        // l's epilogue; vn_{l+1} depends on x_l alone, so it is complete before layer l is launched (the launches: gin_wide_vn.h)
        const float* const vnb = db.ogb_vn;  // GwVnBlob's form; E is its first part
        const bool vn_on = vnb != nullptr;
        const int G = db.b.num_graphs;
        const int L = layers_;  // (the depth: flowgnn_set_num_layers)
        if (vn_on) {
            if (int rc = vn_t_.reserve((size_t)G * D)) return rc;
            if (int rc = vn_vec_[0].reserve((size_t)G * D)) return rc;
            if (int rc = vn_vec_[1].reserve((size_t)G * D)) return rc;
            if (int rc = node_graph_.reserve((size_t)n)) return rc;
        }
        // OGB's residual=True and JK="sum" (flowgnn_set_jk_residual, section 4.24): with either on, the fast paths' launches are
        // gin_wide_jk.hip's instances, under the slots of the ones they stand in for; in the default state nothing below differs
        const bool res_on = db.residual != 0, jk_on = db.jk == FLOWGNN_JK_SUM;
        if (jk_on)
            if (int rc = jk_.reserve((size_t)n * D)) return rc;
        if (int rc = readout_.reserve(db, exact_)) return rc;
        {
            ProfScope p(prof, "atom_encoder", s);
            const int grid = grid_for((long long)n * M::C, 256, 256 * 8);
            if (vn_on)
                gw_atom_encoder_vn_kernel<D><<<grid, 256, 0, s>>>(db.b.node_feature, d_nemb_, db.h[0], n, db.csr.err, vnb);
            else
                gw_atom_encoder_kernel<D><<<grid, 256, 0, s>>>(db.b.node_feature, d_nemb_, db.h[0], n, db.csr.err);
        }
        if (exact_)
            if (int rc = hid_.reserve((size_t)(n > G ? n : G) * H)) return rc;
        int cur = 0;
        for (int l = 0; l < L; l++) {
            // (node embeddings: the last layer writes h_L straight into the caller's buffer, and the readout reads it there)
            // (under JK sum the reverse: the rows the pool is taken over are the sum's, so the last layer's sum goes into the caller's
            // buffer and h_5 into the ping-pong buffer)
            float* const hn = (l == L - 1 && db.node_emb && !jk_on) ? db.node_emb : db.h[cur ^ 1];
            const float* const jk_in = !jk_on ? nullptr : l == 0 ? db.h[cur] : jk_.p;  // x_0 is layer 0's input
            float* const jk_out = !jk_on ? nullptr : (l == L - 1 && db.node_emb) ? db.node_emb : jk_.p;
            const float self_s = db.gin_eps_on ? db.gin_self_scale[l] : 1.0f;
            const float* ecomb = d_ecomb_ + (size_t)l * EDGE_COMBOS * D;
            const int relu_out = l != L - 1;
            const bool vn_next = vn_on && l < L - 1;  // this layer's output rows get vn_{l+1} added
            float* const vnn = vn_vec_[l & 1].p;            // vn_{l+1}; vn_l is vn_vec_[(l - 1) & 1] (l = 0: E, stride 0)
            if (vn_next) {
                {
                    ProfScope p(prof, "gin_wide_vn_pool", s);  // t = sum of x_l's rows + vn_l (a sum whatever the readout's pooling is)
                    if (int rc = launch_gw_vn_pool(D, db.h[cur], db.b.node_off, l == 0 ? vnb : vn_vec_[(l - 1) & 1].p, l == 0 ? 0 : D, vn_t_.p,
                                                   l == 0 ? node_graph_.p : nullptr, G, s))
                        return rc;
                }
                ProfScope p(prof, "gin_wide_vn_update", s);
                if (int rc = launch_gw_vn_update(D, vnb, L - 1, l, vn_t_.p, vnn, hid_.p, G, exact_, db.range_flag,
                                                 !res_on ? nullptr : l == 0 ? vnb : vn_vec_[(l - 1) & 1].p, l == 0 ? 0 : D, s))
                    return rc;
            }
            if (!exact_ && (res_on || jk_on)) {
                ProfScope p(prof, f16_ ? "gin_wide_layer_f16" : "gin_wide_layer", s);
                if (int rc = launch_gw_layer_jk(D, f16_, db.h[cur], hn, db.csr.row_ptr, db.csr.src, db.csr.ecode, ecomb,
                                                f16_ ? d_chunks16_ + (size_t)l * F16::LAYER_BYTES : d_chunks_ + (size_t)l * M::LAYER_BYTES,
                                                d_tails_ + (size_t)l * M::TAIL_FLOATS, n, relu_out, self_s, db.range_flag,
                                                vn_next ? node_graph_.p : nullptr, vn_next ? vnn : nullptr, res_on, jk_in, jk_out, s))
                    return rc;
            } else if (!exact_ && f16_) {
                ProfScope p(prof, "gin_wide_layer_f16", s);
                if (int rc = launch_gw_layer_f16(D, db.h[cur], hn, db.csr.row_ptr, db.csr.src, db.csr.ecode, ecomb,
                                                 d_chunks16_ + (size_t)l * F16::LAYER_BYTES, d_tails_ + (size_t)l * M::TAIL_FLOATS, n, relu_out,
                                                 self_s, db.range_flag, vn_next ? node_graph_.p : nullptr, vn_next ? vnn : nullptr, s))
                    return rc;
            } else if (!exact_) {
                ProfScope p(prof, "gin_wide_layer", s);
                const int grid = (int)ceil_div_ll(n, GW_ROWS);
                if (vn_next)
                    gw_layer_vn_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(
                        db.h[cur], hn, db.csr.row_ptr, db.csr.src, db.csr.ecode, ecomb, d_chunks_ + (size_t)l * M::LAYER_BYTES,
                        d_tails_ + (size_t)l * M::TAIL_FLOATS, n, self_s, db.range_flag, node_graph_.p, vnn);
                else
                    gw_layer_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(
                        db.h[cur], hn, db.csr.row_ptr, db.csr.src, db.csr.ecode, ecomb, d_chunks_ + (size_t)l * M::LAYER_BYTES,
                        d_tails_ + (size_t)l * M::TAIL_FLOATS, n, relu_out, self_s, db.range_flag);
            } else {
                ProfScope p(prof, "gin_wide_layer_f32", s);
                gw_aggregate_kernel<D><<<grid_for((long long)n * M::C, 256, 256 * 8), 256, 0, s>>>(db.h[cur], db.scratch, db.csr.row_ptr, db.csr.src,
                                                                                                   db.csr.ecode, ecomb, n, self_s);
                launch_gw_mlp_f32<D>(db.scratch, d_w1t_ + (size_t)l * D * H, d_b1_ + (size_t)l * H, d_w2t_ + (size_t)l * H * D, d_b2_ + (size_t)l * D,
                                     hid_.p, hn, n, relu_out, s);
                // (the adds in the fast path's order: the residual, the virtual node's vector, the JK sum)
                if (res_on)
                    if (int rc = launch_gw_add_rows(D, hn, hn, db.h[cur], D, n, s)) return rc;
                if (vn_next)
                    if (int rc = launch_gw_vn_add(D, hn, node_graph_.p, vnn, n, s)) return rc;
                if (jk_on)
                    if (int rc = launch_gw_add_rows(D, jk_out, jk_in, hn, D, n, s)) return rc;
            }
            cur ^= 1;
        }
        db.final_h = cur;
        db.h_valid = jk_on || !db.node_emb;
        return readout_.run(db, prof, s, db.node_emb ? db.node_emb : jk_on ? jk_.p : db.h[cur], exact_, hid_.p);
    }

private:
    void free_all() {
        float** ptrs[] = {&d_tails_, &d_nemb_, &d_ecomb_, &d_w1t_, &d_w2t_, &d_b1_, &d_b2_};
        for (auto p : ptrs)
            if (*p) { (void)hipFree(*p); *p = nullptr; }
        if (d_chunks_) { (void)hipFree(d_chunks_); d_chunks_ = nullptr; }
        if (d_chunks16_) { (void)hipFree(d_chunks16_); d_chunks16_ = nullptr; }
        hid_.release();
        readout_.release();
        vn_t_.release();
        vn_vec_[0].release();
        vn_vec_[1].release();
        node_graph_.release();
        jk_.release();
    }
    bool ready_ = false;
    bool exact_ = false;
    bool f16_ = false;  // flowgnn_set_numeric_mode_dim(FLOWGNN_NUMERIC_F16)
    int layers_ = FLOWGNN_NUM_LAYERS_DEFAULT;  // flowgnn_set_num_layers: L, what the per-layer buffers below were packed for while ready_
    GwReadout<D> readout_;         // the head's weights, NUM_TASK, the pooled rows and the gates (wide_common.h)
    uint8_t* d_chunks_ = nullptr;  // the weight stream of gw_layer_kernel: L x LAYER_BYTES
    uint8_t* d_chunks16_ = nullptr;  // the hi-only stream of gin_wide_f16.hip's kernels: L x GwF16Dims::LAYER_BYTES
    float* d_tails_ = nullptr;     // ... and per layer b2 (pre-scaled, padded) and the output scale (both streams)
    float *d_nemb_ = nullptr, *d_ecomb_ = nullptr;
    float *d_w1t_ = nullptr, *d_w2t_ = nullptr, *d_b1_ = nullptr, *d_b2_ = nullptr;  // the exact form's weights, [K][O]
    GrowBuf hid_;     // the exact form's hidden rows [N][H]
    GrowBuf vn_t_;        // OGB's virtual node: t [G][D], the update's input
    GrowBuf vn_vec_[2];    // ... vn_l and vn_{l+1} [G][D], alternating (both are live while layer l's update runs)
    GrowBufI node_graph_;  // ... and node -> graph [N], written by layer 0's pool launch of every pass
    GrowBuf jk_;           // JK sum (section 4.24): the running sum of the rows [N][D], reserved only while it is on; neither ping-pong buffer
};

constexpr int GW_VN_D = FLOWGNN_EMB_DIM_OGB;  // the launchers' one width: the public constant's (the literal stays in make_gin_wide_model)

}  // namespace

Model* make_gin_wide_model(int emb_dim) {
    if (emb_dim == 300) return new GinWideModel<300>();  // FLOWGNN_EMB_DIM_OGB: the one instantiation
    return nullptr;
}

// ---------------------------------------------------------------- gin_wide_vn.h: the virtual node's launches, the only ones in this
// file -- GinWideModel::forward goes through them, and so does gcn_wide.hip (section 4.19)
size_t gw_vn_blob_bytes(int emb_dim, int n_updates) { return emb_dim == GW_VN_D && n_updates > 0 ? GwVnBlob<GW_VN_D>::bytes(n_updates) : 0; }

void gw_vn_blob_pack(int emb_dim, int n_updates, const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2, void* out) {
    if (emb_dim == GW_VN_D) gw_vn_pack<GW_VN_D>(n_updates, vn_embedding, w1, b1, w2, b2, static_cast<uint8_t*>(out));
}

int launch_gw_vn_update(int emb_dim, const void* blob, int n_updates, int l, const float* t, float* vn_next, float* hid, int num_graphs, bool exact,
                        int* range_flag, const float* vn_prev, int vn_prev_stride, hipStream_t s) {
    if (emb_dim != GW_VN_D || l < 0 || l >= n_updates) return FLOWGNN_ERR_UNSUPPORTED;
    if (num_graphs <= 0) return 0;
    constexpr int D = GW_VN_D;
    using VB = GwVnBlob<D>;
    const uint8_t* const wl = static_cast<const uint8_t*>(blob) + VB::E_BYTES + (size_t)l * VB::LAYER_STRIDE;
    if (!exact && vn_prev)  // residual=True (section 4.24): the update instance of gin_wide_jk.hip, the add in its epilogue
        return launch_gw_vn_update_res(D, t, vn_next, wl, reinterpret_cast<const float*>(wl + VB::TAIL_OFF), num_graphs, range_flag, vn_prev,
                                       vn_prev_stride, s);
    if (!exact)
        gw_vn_update_kernel<D><<<(int)ceil_div_ll(num_graphs, GW_ROWS), GW_WAVES * 64, 0, s>>>(
            t, vn_next, wl, reinterpret_cast<const float*>(wl + VB::TAIL_OFF), num_graphs, range_flag);
    else
        launch_gw_mlp_f32<D>(t, reinterpret_cast<const float*>(wl + VB::W1T_OFF), reinterpret_cast<const float*>(wl + VB::B1_OFF),
                             reinterpret_cast<const float*>(wl + VB::W2T_OFF), reinterpret_cast<const float*>(wl + VB::B2_OFF), hid, vn_next,
                             num_graphs, 1, s);
    if (exact && vn_prev) return launch_gw_add_rows(D, vn_next, vn_next, vn_prev, vn_prev_stride, num_graphs, s);
    return 0;
}

int launch_gw_vn_pool(int emb_dim, const float* rows, const int* node_off, const float* vn, int vn_stride, float* t, int* node_graph,
                      int num_graphs, hipStream_t s) {
    if (emb_dim != GW_VN_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (num_graphs <= 0) return 0;
    constexpr int D = GW_VN_D;
    gw_vn_pool_kernel<D><<<grid_for((long long)num_graphs * GwDims<D>::C, 256, 256 * 8), 256, 0, s>>>(rows, node_off, vn, vn_stride, t, node_graph,
                                                                                                      num_graphs);
    return 0;
}

int launch_gw_vn_add(int emb_dim, float* rows, const int* node_graph, const float* vn, int n_tot, hipStream_t s) {
    if (emb_dim != GW_VN_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (n_tot <= 0) return 0;
    constexpr int D = GW_VN_D;
    gw_vn_add_kernel<D><<<grid_for((long long)n_tot * GwDims<D>::C, 256, 256 * 8), 256, 0, s>>>(rows, node_graph, vn, n_tot);
    return 0;
}

}  // namespace fg
