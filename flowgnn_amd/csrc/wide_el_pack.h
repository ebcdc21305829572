// wide_el_pack.h -- OGB's linear edge encoder at width 300 (DESIGN.md sections 4.31 and 4.32): the device form of the encoder's two
// tensors and its host packer, shared by the two translation units whose walks run the encoder on the matrix pipe -- gin_wide_el.hip
// (GIN) and gcn_wide_el.hip (GCN).  Host code and compile-time offsets only; the slot table is at the head of gin_wide_el.hip.
#pragma once
#include <cstring>
#include <vector>

#include "common.h"
#include "wide_common.h"

namespace fg {
namespace {

// per layer, in bytes (every part a multiple of 16): T fragments of 1 KiB, the A operands of the encoder's MFMA, one per 16-column
// output tile | 1 / scale, padded to 16 bytes | w [D][F] | b [D]     (the two fp32 parts: the exact form)
template <int D>
struct GwElBlob {
    static constexpr int T = (D + 15) / 16;  // (GwDims<D>::T2, GcwDims<D>::T)
    static constexpr size_t INV_OFF = (size_t)T * 1024;
    static constexpr size_t W_OFF = INV_OFF + 16;
    static constexpr size_t b_off(int F) { return W_OFF + (size_t)D * F * 4; }
    static constexpr size_t layer_stride(int F) { return b_off(F) + (size_t)D * 4; }
    static_assert((D * 4) % 16 == 0, "every part is read in 16-byte pieces");
};

inline void gw_el_put(uint8_t* frag, int lane, int e, float v) {
    const _Float16 hv = (_Float16)v;
    std::memcpy(frag + lane * 16 + e * 2, &hv, 2);
}

// one layer: w [D][F], b [D] (row-major, host) -> the T fragments (the slot table at the head of gin_wide_el.hip), 1 / scale, and the
// fp32 copies
template <int D>
void gw_el_pack_layer(int F, const float* w, const float* b, uint8_t* out) {
    using B = GwElBlob<D>;
    std::memset(out, 0, B::layer_stride(F));
    // one power of two for the weights and the bias: they share the accumulator (max |.| times scale in [1, 2), far inside f16)
    std::vector<float> wb(w, w + (size_t)D * F);
    wb.insert(wb.end(), b, b + D);
    const float scale = gw_pow2_scale(wb.data(), wb.size());
    for (int t = 0; t < B::T; t++)
        for (int lane = 0; lane < 64; lane++) {
            const int o = 16 * t + (lane & 15), gk = lane >> 4;
            if (o >= D) continue;
            for (int e = 0; e < 8; e++) {
                const int kk = 16 * (e >> 2) + 4 * gk + (e & 3);
                float val = 0.0f;
                if (kk < 3 * F) {
                    const float ws = w[(size_t)o * F + kk % F] * scale;
                    const float hi = (float)(_Float16)ws;
                    val = kk < 2 * F ? hi : ws - hi;
                } else if (kk < 3 * F + 2) {
                    const float bs = b[o] * scale;
                    const float hi = (float)(_Float16)bs;
                    val = kk == 3 * F ? hi : bs - hi;
                }
                gw_el_put(out + (size_t)t * 1024, lane, e, val);
            }
        }
    const float inv = 1.0f / scale;
    std::memcpy(out + B::INV_OFF, &inv, 4);
    std::memcpy(out + B::W_OFF, w, (size_t)D * F * 4);
    std::memcpy(out + B::b_off(F), b, (size_t)D * 4);
}

}  // namespace
}  // namespace fg
