// GCN at OGB's default width with OGB's residual=True and JK="sum" (flowgnn_set_model_jk_residual).
//
// gcn_wide.hip keeps the POST-linear rows W_l x_l + b_l in HBM; the rows OGB adds (h_list[l] = x_l) exist in the layer kernel's
// registers alone, behind the walk.  So both options are a second row stream through that kernel, fp32, on the lane's own pieces:
//   residual   a = relu(pre_s)[v] + x_s[v] (rin), in front of the virtual node's add -- the partial rows, and with them t, then hold
//              the residual, which is OGB's order -- and x_{s+1}[v] = a (+ vn_{s+1}[g(v)]) stored for the next stage (rout, in place)
//   JK sum     jk_out[v] = jk_in[v] + x_{s+1}[v]: a read-modify-write per stage, six terms in layer order, x_0 first
// x_0 is written by one more launch of the wide atom encoder on the unprojected table (GcnWideModel::forward); the final stage adds
// x_4 and leaves h_5, and the sum.  A lane reads its own pieces before it writes them and nobody else touches them: no atomics, and a
// graph's bits do not depend on where it stands in a batch (beyond what the partial rows already make of that, section 4.19).
// The kernels are instances of gcn_wide_body.h's bodies (the layer's with EXT = true); which adds a launch does is decided by null or non-null row
// pointers (wave-uniform branches), so there is one kernel per (virtual node), not one per setting.  They live here and not beside
// their parents so that gcn_wide.hip's device code stays what it was, kernel for kernel.
#include "../../include/flowgnn.h"
#include "common.h"
#include "dense_split.h"
#include "gcn_wide_body.h"
#include "gcn_wide_jk.h"
#include "wide_common.h"

namespace fg {
namespace {

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_layer_jk_kernel(const float* __restrict__ x, float* __restrict__ xout,
                                                                     const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                     const uint8_t* __restrict__ ecode, const float* __restrict__ esc,
                                                                     const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                                     const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                     int n_tot, int* __restrict__ range_flag, GcwExtArgs ext) {
    gcw_layer_body<D, false, true>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, GcwNoVnArgs{}, ext);
}

// the VN instance: x_{s+1}[v] = (relu(pre_s)[v] (+ x_s[v])) + vn_{s+1}[g(v)], and (s < 3) the partial rows of x_{s+1}
template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_layer_vn_jk_kernel(const float* __restrict__ x, float* __restrict__ xout,
                                                                        const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                        const uint8_t* __restrict__ ecode, const float* __restrict__ esc,
                                                                        const int* __restrict__ out_deg, const float* __restrict__ tab,
                                                                        const uint8_t* __restrict__ wchunks, const float* __restrict__ tailp,
                                                                        int n_tot, int* __restrict__ range_flag, GcwVnArgs vna, GcwExtArgs ext) {
    gcw_layer_body<D, true, true>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, vna, ext);
}

template <int D>
__global__ __launch_bounds__(GW_WAVES * 64) void gcw_final_jk_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                     const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                                     const uint8_t* __restrict__ ecode, const float* __restrict__ esc,
                                                                     const int* __restrict__ out_deg, const float* __restrict__ tab, int n_tot,
                                                                     GcwExtArgs ext) {
    gcw_final_jk_body<D>(x, out, row_ptr, src, ecode, esc, out_deg, tab, n_tot, ext);
}

constexpr int GCWJ_D = FLOWGNN_EMB_DIM_OGB;  // the launchers' one width: the public constant's

}  // namespace

int launch_gcw_layer_jk(int emb_dim, const float* x, float* xout, const int* row_ptr, const int* src, const uint8_t* ecode, const float* esc,
                        const int* out_deg, const float* tab, const uint8_t* wchunks, const float* tailp, int n_tot, int* range_flag,
                        const int* node_graph, const float* vn, float* part, const float* rin, float* rout, const float* jk_in, float* jk_out,
                        hipStream_t s) {
    if (emb_dim != GCWJ_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (jk_out && (!jk_in || jk_out == rin || jk_out == rout || jk_out == xout)) return FLOWGNN_ERR_ARG;
    if (rout && (rout == xout || rout == x)) return FLOWGNN_ERR_ARG;
    if (node_graph && !vn) return FLOWGNN_ERR_ARG;
    if (n_tot <= 0) return 0;
    constexpr int D = GCWJ_D;
    const int grid = (int)ceil_div_ll(n_tot, GW_ROWS);
    const GcwExtArgs ext{rin, rout, jk_in, jk_out};
    if (node_graph)
        gcw_layer_vn_jk_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag,
                                                                 GcwVnArgs{node_graph, vn, part}, ext);
    else
        gcw_layer_jk_kernel<D><<<grid, GW_WAVES * 64, 0, s>>>(x, xout, row_ptr, src, ecode, esc, out_deg, tab, wchunks, tailp, n_tot, range_flag, ext);
    return 0;
}

int launch_gcw_final_jk(int emb_dim, const float* x, float* out, const int* row_ptr, const int* src, const uint8_t* ecode, const float* esc,
                        const int* out_deg, const float* tab, int n_tot, const float* rin, const float* jk_in, float* jk_out, hipStream_t s) {
    if (emb_dim != GCWJ_D) return FLOWGNN_ERR_UNSUPPORTED;
    if (jk_out && (!jk_in || jk_out == out || jk_out == rin)) return FLOWGNN_ERR_ARG;
    if (n_tot <= 0) return 0;
    constexpr int D = GCWJ_D;
    gcw_final_jk_kernel<D><<<(int)ceil_div_ll(n_tot, GW_ROWS), GW_WAVES * 64, 0, s>>>(x, out, row_ptr, src, ecode, esc, out_deg, tab, n_tot,
                                                                                      GcwExtArgs{rin, nullptr, jk_in, jk_out});
    return 0;
}

}  // namespace fg
