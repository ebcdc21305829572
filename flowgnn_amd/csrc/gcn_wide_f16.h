// gcn_wide_f16.h -- GCN at OGB's default width in FLOWGNN_NUMERIC_F16 (flowgnn_set_model_numeric_mode_dim): the layout of
// the hi-only weight stream and the launcher of gcn_wide_f16.hip's four layer kernels.  The device code exists once, in that
// translation unit; GcnWideModel (gcn_wide.hip) packs the stream from the split one it already builds and calls the launcher under a
// profiler slot of its own, and only while the mode is on: in FLOWGNN_NUMERIC_F32 no launch comes from here.  emb_dim: the one
// instantiation's, FLOWGNN_EMB_DIM_OGB (anything else: FLOWGNN_ERR_UNSUPPORTED).
#pragma once
#include "common.h"

namespace fg {

// A layer's stream: STEPS chunks of TPC whole output tiles, hi halves only.  Chunk c, in 1 KiB fragments (64 lanes x 8 halves): output
// tile TPC c + tl, K-step ks: fragment tl KS + ks; tiles at or beyond T are zeros (their products are computed and dropped).  The
// per-layer tail (b pre-scaled and padded, then 1 / s) is the split stream's own (gcw_pack_layer) and is read as it is.
template <int D>
struct GcwF16Dims {
    static constexpr int KS = (D + 31) / 32;  // K-steps of the product (K padded to 32 KS)
    static constexpr int T = (D + 15) / 16;   // 16-row output tiles, the last one masked at column D
    static constexpr int TPC = 4;             // output tiles of a chunk
    static constexpr int STEPS = (T + TPC - 1) / TPC;
    static constexpr int TILE_BYTES = KS * 1024;
    static constexpr int CHUNK_BYTES = TPC * TILE_BYTES;
    static constexpr int PIECES = CHUNK_BYTES / 1024;
    static constexpr size_t LAYER_BYTES = (size_t)STEPS * CHUNK_BYTES;
    static constexpr int SCALE_AT = STEPS * TPC * 16;  // where the tail holds 1 / s: the split stream's place
};

// Stage s = 0..3 of gcn_wide.hip with a_{s+1} and W_{s+1} each ONE f16 value, rounded to nearest even, and one MFMA per product:
// gcw_layer_f16_kernel; node_graph non-null: the virtual-node instance (vn = vn_{s+1}, part may be null); any of rin / rout / jk_out
// non-null: the instance with OGB's residual and JK sum behind the walk (launch_gcw_layer_jk's contract, gcn_wide_jk.h -- the rows it
// stores are the unrounded a).  wchunks: the layer's GcwF16Dims stream; tailp: the split stream's tail of that layer.
int launch_gcw_layer_f16(int emb_dim, const float* x, float* xout, const int* row_ptr, const int* src, const uint8_t* ecode, const float* esc,
                         const int* out_deg, const float* tab, const uint8_t* wchunks, const float* tailp, int n_tot, int* range_flag,
                         const int* node_graph, const float* vn, float* part, const float* rin, float* rout, const float* jk_in, float* jk_out,
                         hipStream_t s);

}  // namespace fg
