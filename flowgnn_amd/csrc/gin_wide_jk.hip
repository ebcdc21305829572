// GIN at OGB's default width with OGB's residual=True and JK="sum" (flowgnn_set_jk_residual).
//
// Neither option adds a parameter or a launch: both are fp32 adds on the 19 output tiles a lane holds at the end of the layer kernel.
//   residual   h_{l+1}[v] = act(layer l of x_l)[v] + x_l[v]: one more read of the node's own input row, which the kernel read earlier
//              for the self term, at the same float4 addresses (rows are 1200 B: every piece is 16-byte aligned); added after the ReLU
//              and before the virtual node's vector, the last layer included.  In the virtual node's update, vn_{l+1} = vn_l + relu(..).
//   JK sum     r[v] = ((((x_0 + x_1) + x_2) + x_3) + x_4) + h_5 -- six terms, left to right, the rows WITH the virtual node's vector
//              inside, as OGB's GNN_node_Virtualnode has them.  Layer 0 stores x_0[v] + x_1[v] into the sum's buffer, layers 1..4 add
//              what they store: a read-modify-write of the lane's own pieces (no atomics, no other workgroup touches those rows), in
//              layer order, so a graph's bits do not depend on where it stands in a batch.
// The kernels are instances of the bodies gin_wide.hip and gin_wide_f16.hip compile (gin_wide_body.h, gin_wide_f16_body.h) with
// EXT = true; which of the two adds a launch does is decided by its pointer arguments (wave-uniform branches in the epilogue), so
// there is one kernel per (numeric mode, virtual node), not one per setting.  They live here and not beside their parents so that
// those files' device code stays what it was, kernel for kernel.
#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "gin_wide_body.h"
#include "gin_wide_f16.h"
#include "gin_wide_f16_body.h"
#include "gin_wide_jk.h"
#include "wide_common.h"

namespace fg {
namespace {

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_layer_jk_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                    const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                    const uint8_t* __restrict__ ecode, const float* __restrict__ ecomb,
                                                                    const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                    int n_tot, int relu_out, float self_s, int* __restrict__ range_flag,
                                                                    int residual, const float* jk_in, float* jk_out) {
    gw_layer_body<D, GW_PLAIN, true>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, relu_out, self_s, range_flag, nullptr, nullptr,
                                     residual ? h : nullptr, D, jk_in, jk_out);
}

// the VN instance: x_{l+1}[v] = (relu(layer l of x_l)[v] (+ x_l[v])) + vn_{l+1}[node_graph[v]] (always ReLU'd: layers 0..3)
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_layer_vn_jk_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                       const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                       const uint8_t* __restrict__ ecode, const float* __restrict__ ecomb,
                                                                       const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                       int n_tot, float self_s, int* __restrict__ range_flag,
                                                                       const int* __restrict__ node_graph, const float* __restrict__ vn_add,
                                                                       int residual, const float* jk_in, float* jk_out) {
    gw_layer_body<D, GW_VN, true>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, 1, self_s, range_flag, node_graph, vn_add,
                                  residual ? h : nullptr, D, jk_in, jk_out);
}

// the update instance under residual=True: vn_next[g] = vn_prev[g * vn_prev_stride] + relu(W2 relu(W1 t[g] + b1) + b2)
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_vn_update_res_kernel(const float* __restrict__ t, float* __restrict__ vn_next,
                                                                         const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                         int num_graphs, int* __restrict__ range_flag,
                                                                         const float* __restrict__ vn_prev, int vn_prev_stride) {
    gw_layer_body<D, GW_UPDATE, true>(t, vn_next, nullptr, nullptr, nullptr, nullptr, wchunks, tailp, num_graphs, 1, 1.0f, range_flag, nullptr,
                                      nullptr, vn_prev, vn_prev_stride, nullptr, nullptr);
}

// FLOWGNN_NUMERIC_F16 (section 4.22): the same two epilogues on gin_wide_f16_body.h's body
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_layer_jk_f16_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                        const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                        const uint8_t* __restrict__ ecode, const float* __restrict__ ecomb,
                                                                        const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                        int n_tot, int relu_out, float self_s, int* __restrict__ range_flag,
                                                                        int residual, const float* jk_in, float* jk_out) {
    gwf_layer_body<D, false, true>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, relu_out, self_s, range_flag, nullptr, nullptr,
                                   residual ? h : nullptr, jk_in, jk_out);
}

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_layer_vn_jk_f16_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                           const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                           const uint8_t* __restrict__ ecode, const float* __restrict__ ecomb,
                                                                           const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                           int n_tot, float self_s, int* __restrict__ range_flag,
                                                                           const int* __restrict__ node_graph, const float* __restrict__ vn_add,
                                                                           int residual, const float* jk_in, float* jk_out) {
    gwf_layer_body<D, true, true>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, 1, self_s, range_flag, node_graph, vn_add,
                                  residual ? h : nullptr, jk_in, jk_out);
}

// out[v] = a[v] + b[v * b_stride]: one lane per (row, float4 piece); out may be a (a lane reads its piece before it writes it)
template <int D>
__global__ __launch_bounds__(256) void gw_add_rows_kernel(float* out, const float* a, const float* __restrict__ b, int b_stride, int n_rows) {
    constexpr int C = D / 4;
    const long long items = (long long)n_rows * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const long long v = i / C;
        const int c = (int)(i - v * C);
        const float4 x = reinterpret_cast<const float4*>(a)[i];
        const float4 w = *reinterpret_cast<const float4*>(b + (size_t)v * b_stride + 4 * c);
        reinterpret_cast<float4*>(out)[i] = make_float4(x.x + w.x, x.y + w.y, x.z + w.z, x.w + w.w);
    }
}

constexpr int GWJ_D = FLOWGNN_EMB_DIM_OGB;  // the launchers' one width: the public constant's

}  // namespace

int launch_gw_layer_jk(int emb_dim, bool f16, const float* h, float* hout, const int* row_ptr, const int* src, const uint8_t* ecode,
                       const float* ecomb, const uint8_t* wchunks, const float* tailp, int n_tot, int relu_out, float self_s, int* range_flag,
                       const int* node_graph, const float* vn_add, bool residual, const float* jk_in, float* jk_out, hipStream_t s) {
    if (emb_dim != GWJ_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (jk_out && (!jk_in || jk_out == hout)) return FLOWGNN_ERR_ARG;
    if (n_tot <= 0) return 0;
    constexpr int D = GWJ_D;
    const int grid = (int)ceil_div_ll(n_tot, GW_ROWS);
    const int res = residual ? 1 : 0;
    if (f16 && node_graph)
        gw_layer_vn_jk_f16_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, self_s, range_flag,
                                                                    node_graph, vn_add, res, jk_in, jk_out);
    else if (f16)
        gw_layer_jk_f16_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, relu_out, self_s,
                                                                 range_flag, res, jk_in, jk_out);
    else if (node_graph)
        gw_layer_vn_jk_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, self_s, range_flag,
                                                                node_graph, vn_add, res, jk_in, jk_out);
    else
        gw_layer_jk_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, relu_out, self_s,
                                                             range_flag, res, jk_in, jk_out);
    return 0;
}

int launch_gw_vn_update_res(int emb_dim, const float* t, float* vn_next, const uint8_t* wchunks, const float* tailp, int num_graphs,
                            int* range_flag, const float* vn_prev, int vn_prev_stride, hipStream_t s) {
    if (emb_dim != GWJ_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (!vn_prev || vn_prev == vn_next) return FLOWGNN_ERR_ARG;
    if (num_graphs <= 0) return 0;
    constexpr int D = GWJ_D;
    gw_vn_update_res_kernel<D><<<(int)ceil_div_ll(num_graphs, GW_ROWS), GW_WAVES * 64, 0, s>>>(t, vn_next, wchunks, tailp, num_graphs, range_flag,
                                                                                               vn_prev, vn_prev_stride);
    return 0;
}

int launch_gw_add_rows(int emb_dim, float* out, const float* a, const float* b, int b_stride, int n_rows, hipStream_t s) {
    if (emb_dim != GWJ_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (n_rows <= 0) return 0;
    constexpr int D = GWJ_D;
    gw_add_rows_kernel<D><<<grid_for((long long)n_rows * (D / 4), 256, 256 * 8), 256, 0, s>>>(out, a, b, b_stride, n_rows);
    return 0;
}

}  // namespace fg
