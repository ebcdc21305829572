// gin_wide_el_walk.h -- the in-edge walk of GIN's layer at width 300 with OGB's linear edge encoder on the matrix pipe (gw_el_walk;
// DESIGN.md section 4.31, the slot table at the head of gin_wide_el.hip).  The walk's arithmetic exists once, here; two translation
// units include it: gin_wide_el.hip (the default mode's layer, gw_layer_body with EL = true, which gin_wide_body.h declares it for) and
// gin_wide_el_f16.hip (the layer with the f16 node MLP behind the same walk, section 4.37).
#pragma once
#include "common.h"
#include "dense_split.h"
#include "gin_wide_body.h"
#include "wide_common.h"

namespace fg {
namespace {

// The walk.  K index of slot e (0..7) of lane group gk: 16 (e >> 2) + 4 gk + (e & 3), the map of gw_pack_tile.  What a lane's eight
// slots hold is fixed for the launch: which feature (el_foff), and per 32-bit word of the operand which halves take the hi part, the
// lo part or the constant 1 -- so a trip builds its column with eight cached loads, four splits and four mask merges.
template <int D>
__device__ __forceinline__ void gw_el_walk(const float* __restrict__ h, const int* __restrict__ src, const int* __restrict__ eid,
                                           const float* __restrict__ ef, int el_f, float el_inv, const char* s_frag, int e_cur, int e_end,
                                           int lane, float (&bq)[4 * GwDims<D>::Q], float& vmax) {
    using M = GwDims<D>;
    const int g = lane >> 4;
    int foff[8];
    uint32_t m_hi[4] = {0, 0, 0, 0}, m_lo[4] = {0, 0, 0, 0}, m_one[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int kk = 16 * (e >> 2) + 4 * g + (e & 3);
        const int part = kk < el_f ? 0 : kk < 2 * el_f ? 1 : 2;
        foff[e] = kk < 3 * el_f ? kk - part * el_f : 0;  // (a slot beyond 3 F reads feature 0 and masks it away)
        const int sh = 16 * (e & 1);
        if (kk < 3 * el_f) {
            if (part == 1) m_lo[e >> 1] |= 0xffffu << sh;
            else m_hi[e >> 1] |= 0xffffu << sh;
        } else if (kk < 3 * el_f + 2) {
            m_one[e >> 1] |= 0x3c00u << sh;  // f16 1.0: the bias slots
        }
    }
    // the trip count is the wave's longest row: the MFMAs are executed by all 64 lanes, a row with no edge left contributes a zero
    // column and drops what comes back
    while (__any(e_cur < e_end)) {
        const bool act = e_cur < e_end;
        int u = 0;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (act) {
            u = src[e_cur];
            const float* fr = ef + (size_t)eid[e_cur] * el_f;  // the four g groups of a row read the same 4 F bytes
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = fr[foff[e]];
        }
        e_cur++;
        ds_uint4_t b;
        uint32_t bw[4];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            // every feature is slot kk < F of some lane of its row: the range check sees all of them (NaN fails the compare too)
            vmax = (__builtin_fabsf(v[2 * w]) < 6.0e4f && __builtin_fabsf(v[2 * w + 1]) < 6.0e4f) ? vmax : __builtin_inff();
            uint32_t hi, lo;
            DS_SPLIT2(v[2 * w], v[2 * w + 1], hi, lo);
            bw[w] = act ? ((hi & m_hi[w]) | (lo & m_lo[w]) | m_one[w]) : 0u;
        }
        b.x = bw[0]; b.y = bw[1]; b.z = bw[2]; b.w = bw[3];
        const float* hr = h + (size_t)u * D + 4 * g;
#pragma unroll
        for (int q0 = 0; q0 < M::Q; q0 += M::KS1) {
            float4 x[M::KS1];
            if (act) {
#pragma unroll
                for (int q = 0; q < M::KS1; q++)
                    if (16 * (q0 + q) + 4 * g < D) x[q] = *reinterpret_cast<const float4*>(hr + 16 * (q0 + q));
            }
#pragma unroll
            for (int q = 0; q < M::KS1; q++) {
                const int t = q0 + q;
                if (t < M::T2) {  // (compile time: the pieces beyond the last tile do not exist)
                    const ds_uint4_t a = *reinterpret_cast<const ds_uint4_t*>(s_frag + t * 1024 + lane * 16);
                    const float4_t c = DS_MFMA16(a, b, ((float4_t){0.f, 0.f, 0.f, 0.f}));
                    if (act && 16 * t + 4 * g < D) {  // W_e e + b_e = c / scale, exactly; one rounding in the add, as the table path has
                        bq[4 * t + 0] += relu1(__builtin_fmaf(c.x, el_inv, x[q].x));
                        bq[4 * t + 1] += relu1(__builtin_fmaf(c.y, el_inv, x[q].y));
                        bq[4 * t + 2] += relu1(__builtin_fmaf(c.z, el_inv, x[q].z));
                        bq[4 * t + 3] += relu1(__builtin_fmaf(c.w, el_inv, x[q].w));
                    }
                }
            }
        }
    }
}

}  // namespace
}  // namespace fg
