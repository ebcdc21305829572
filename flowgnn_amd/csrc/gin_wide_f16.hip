// GIN at OGB's default width in FLOWGNN_NUMERIC_F16 (flowgnn_set_numeric_mode_dim): the layer kernel of
// gin_wide.hip with every operand of the node MLP ONE f16 value, rounded to nearest even, and one MFMA per product.
//
// gw_layer_f16_kernel<D> / gw_layer_vn_f16_kernel<D> (H = 2 D): a wave owns one 16-node column tile and gathers
// a[v] = fma(h[v], s_l, sum_e relu(h[src_e] + ecomb[code_e])) in fp32, in CSR order, exactly as gw_layer_body does; a is then rounded
// pair by pair (one v_cvt_pk_f16_f32 each) into the B operands of MLP1 -- no lo registers.  Per step it runs MLP1 of two hidden tiles
// (2 KS1 MFMAs), rounds their ReLU'd values in the scaled domain (r(hid s1): the accumulator holds s1 (W1 a + b1)) and feeds them as
// one K-step of MLP2 into the T2 row accumulators (T2 MFMAs): 2 KS1 + T2 MFMAs per step where the split kernel issues three times
// that.  The weights are the hi halves of the split stream, r(W s), and nothing else: a chunk is half as long (gin_wide_f16.h), so the
// combined edge table no longer fits behind a weight buffer and has an LDS object of its own; with it out of the way chunk 1 is
// requested with chunk 0, in front of the gather.  The weight chunks go L2 -> LDS by LDS-DMA into two distinct LDS objects shared by the eight waves
// of a 128-row workgroup; the only synchronisation is s_waitcnt vmcnt(0) + a workgroup barrier per step.
//   lane (j = lane & 15, g = lane >> 4); B operand of K-step ks, slot e (0..7): feature 16 (2 ks + (e >> 2)) + 4 g + (e & 3).
// Everything else is fp32 and gin_wide.hip's: biases, 1 / (s1 s2), the ReLU, the virtual node's add in the epilogue, the range flag at
// 6e4 (the engine then repeats the pass on the fp32 exact path).  The body is the f16 mode's own copy (gin_wide_f16_body.h, which
// gin_wide_jk.hip instantiates as well): DESIGN.md section 4.21 records that sharing device code between the wide files moves their
// register allocation.
#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "gin_wide_f16.h"
#include "gin_wide_f16_body.h"  // GwfDims, gwf_step and gwf_layer_body
#include "wide_common.h"  // GW_WAVES / GW_ROWS, gw_relu, the LDS-DMA issue

namespace fg {
namespace {

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_layer_f16_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                     const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                     const uint8_t* __restrict__ ecode, const float* __restrict__ ecomb,
                                                                     const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                     int n_tot, int relu_out, float self_s, int* __restrict__ range_flag) {
    gwf_layer_body<D, false>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, relu_out, self_s, range_flag, nullptr, nullptr);
}

// the VN instance: x_{l+1}[v] = relu(layer l of x_l)[v] + vn_{l+1}[node_graph[v]] (always ReLU'd: layers 0..3)
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gw_layer_vn_f16_kernel(const float* __restrict__ h, float* __restrict__ hout,
                                                                        const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                        const uint8_t* __restrict__ ecode, const float* __restrict__ ecomb,
                                                                        const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                        int n_tot, float self_s, int* __restrict__ range_flag,
                                                                        const int* __restrict__ node_graph, const float* __restrict__ vn_add) {
    gwf_layer_body<D, true>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, 1, self_s, range_flag, node_graph, vn_add);
}

constexpr int GWF_D = FLOWGNN_EMB_DIM_OGB;  // the launcher's one width: the public constant's

}  // namespace

int launch_gw_layer_f16(int emb_dim, const float* h, float* hout, const int* row_ptr, const int* src, const uint8_t* ecode,
                        const float* ecomb, const uint8_t* wchunks, const float* tailp, int n_tot, int relu_out, float self_s,
                        int* range_flag, const int* node_graph, const float* vn_add, hipStream_t s) {
    if (emb_dim != GWF_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (n_tot <= 0) return 0;
    constexpr int D = GWF_D;
    const int grid = (int)ceil_div_ll(n_tot, GW_ROWS);
    if (node_graph)
        gw_layer_vn_f16_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, self_s, range_flag,
                                                                 node_graph, vn_add);
    else
        gw_layer_f16_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(h, hout, row_ptr, src, ecode, ecomb, wchunks, tailp, n_tot, relu_out, self_s,
                                                              range_flag);
    return 0;
}

}  // namespace fg
