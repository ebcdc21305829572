// gin_wide_f16.h -- GIN at width 300 in FLOWGNN_NUMERIC_F16 (flowgnn_set_numeric_mode_dim): the layout of the
// hi-only weight stream and the launchers of the two layer kernels of gin_wide_f16.hip.  The device code exists once, in that
// translation unit; GinWideModel (gin_wide.hip) packs the stream from the split one it already builds and calls the launcher under a
// profiler slot of its own.  emb_dim: 300, the one instantiation (anything else: FLOWGNN_ERR_UNSUPPORTED).
#pragma once
#include "common.h"

namespace fg {

// Chunk s of a layer's stream, in 1 KiB fragments (64 lanes x 8 halves), hi halves only:
//   [0, W2_OFF): W1 of hidden tiles 2s, 2s + 1: fragment (ks * 2 + tl)                     (zero for s = KS2)
//   [W2_OFF, B1_OFF): W2 of K-step s - 1: fragment t2                                        (zero for s = 0)
//   [B1_OFF, CHUNK_BYTES): b1 of the two hidden tiles, pre-scaled: 2 x 16 floats
// The per-layer tail (b2 pre-scaled and padded, then 1 / (s1 s2)) is the split stream's own: it is read from global memory as it is.
template <int D>
struct GwF16Dims {
    static constexpr int H = 2 * D;
    static constexpr int KS1 = (D + 31) / 32;
    static constexpr int KS2 = (H + 31) / 32;
    static constexpr int T2 = (D + 15) / 16;
    static constexpr int STEPS = KS2 + 1;
    static constexpr int W2_OFF = KS1 * 2 * 1024;
    static constexpr int B1_OFF = W2_OFF + T2 * 1024;
    static constexpr int CHUNK_BYTES = B1_OFF + 2 * 16 * 4;
    static constexpr int PIECES = (CHUNK_BYTES + 1023) / 1024;  // DMA pieces of 1 KiB, the last one partial
    static constexpr int LAST_LANES = (CHUNK_BYTES - (PIECES - 1) * 1024) / 16;
    static constexpr int CHUNK_STRIDE = PIECES * 1024;          // in global memory
    static constexpr size_t LAYER_BYTES = (size_t)STEPS * CHUNK_STRIDE;
};

// hout[v] = W2 relu(W1 a[v] + b1) + b2 with a, the hidden units and both matrices rounded to f16 (to nearest even), one MFMA per
// product: gw_layer_f16_kernel, or -- node_graph non-null -- gw_layer_vn_f16_kernel, which adds vn_add[node_graph[v]] to the ReLU'd
// row in its epilogue (relu_out is 1 there).  wchunks: the layer's GwF16Dims stream; tailp: the split stream's tail of that layer.
int launch_gw_layer_f16(int emb_dim, const float* h, float* hout, const int* row_ptr, const int* src, const uint8_t* ecode,
                        const float* ecomb, const uint8_t* wchunks, const float* tailp, int n_tot, int relu_out, float self_s,
                        int* range_flag, const int* node_graph, const float* vn_add, hipStream_t s);

}  // namespace fg
