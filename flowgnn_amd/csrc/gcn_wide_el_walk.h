// gcn_wide_el_walk.h -- the trips of GCN's in-edge walk at width 300 with OGB's linear edge encoder on the matrix pipe (gcw_el_trips;
// DESIGN.md section 4.32, the slot table at the head of gin_wide_el.hip).  The walk's arithmetic exists once, here; two translation
// units include it: gcn_wide_el.hip (the default mode's stages, gcw_layer_body and gcw_final_el_kernel with EL = true, which
// gcn_wide_body.h declares it for) and gcn_wide_el_f16.hip (the stage with the f16 product behind the same walk, section 4.38).
#pragma once
#include "common.h"
#include "dense_split.h"
#include "gcn_wide_body.h"
#include "wide_common.h"

namespace fg {
namespace {

// K index of slot s (0..7) of lane group g: 16 (s >> 2) + 4 g + (s & 3), the map of gw_pack_tile.  What a lane's eight slots hold is
// fixed for the launch: which feature, and per 32-bit word of the operand which halves take the hi part, the lo part or the
// constant 1 -- so a trip builds its column from eight floats with four splits and four mask merges.
template <int D>
__device__ __forceinline__ void gcw_el_trips(const float* __restrict__ x, const int* __restrict__ src, const float* __restrict__ esc,
                                             const GcwElArgs& el, const float* s_blk, int e, int e_end, float dinv_v, int g,
                                             float (&a)[4 * GcwDims<D>::Q]) {
    using M = GcwDims<D>;
    const int lane = threadIdx.x & 63;
    const int F = el.el_f;
    const char* const s_frag = reinterpret_cast<const char*>(s_blk);
    const float el_inv = s_blk[GcwElLds<D>::INV_FLOAT];
    int foff[8];
    uint32_t m_hi[4] = {0, 0, 0, 0}, m_lo[4] = {0, 0, 0, 0}, m_one[4] = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const int kk = 16 * (s >> 2) + 4 * g + (s & 3);
        const int part = kk < F ? 0 : kk < 2 * F ? 1 : 2;
        foff[s] = kk < 3 * F ? kk - part * F : 0;  // (a slot beyond 3 F reads feature 0 and masks it away)
        const int sh = 16 * (s & 1);
        if (kk < 3 * F) {
            if (part == 1) m_lo[s >> 1] |= 0xffffu << sh;
            else m_hi[s >> 1] |= 0xffffu << sh;
        } else if (kk < 3 * F + 2) {
            m_one[s >> 1] |= 0x3c00u << sh;  // f16 1.0: the bias slots
        }
    }
    // the straddling piece: gcw_walk's rule (lanes beyond column D read the row's last four columns; their W_e rows are zeros)
    constexpr int NQ = M::T;
    const int o_last = 16 * (NQ - 1) < D - 4 - 4 * g ? 16 * (NQ - 1) : D - 4 - 4 * g;
#define GCWE_OFF(q) (16 * (q) + 16 > D ? o_last : 16 * (q))
    // one CSR entry ahead: src, dinv[src] and the features; two ahead: eid.  (The four g groups of a row read the same 4 F bytes.)
    int u_nx = 0, id_nx = 0;
    float n_nx = 0.0f;
    float f_nx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (e < e_end) {
        u_nx = src[e];
        n_nx = esc[e];
        const float* fr = el.ef + (size_t)el.eid[e] * F;
#pragma unroll
        for (int s = 0; s < 8; s++) f_nx[s] = fr[foff[s]];
    }
    if (e + 1 < e_end) id_nx = el.eid[e + 1];
    float vmax = 0.0f;
    while (__any(e < e_end)) {
        const bool act = e < e_end;
        const int u = u_nx;
        const float norm = act ? n_nx * dinv_v : 0.0f;
        ds_uint4_t b;
        uint32_t bw[4];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            // every feature is slot kk < F of some lane of its row: the range check sees all of them (NaN fails the compare too).
            // A finished lane holds the features it checked on its last trip, or zeros
            vmax = (__builtin_fabsf(f_nx[2 * w]) < 6.0e4f && __builtin_fabsf(f_nx[2 * w + 1]) < 6.0e4f) ? vmax : __builtin_inff();
            uint32_t hi, lo;
            DS_SPLIT2(f_nx[2 * w], f_nx[2 * w + 1], hi, lo);
            bw[w] = act ? ((hi & m_hi[w]) | (lo & m_lo[w]) | m_one[w]) : 0u;
        }
        b.x = bw[0]; b.y = bw[1]; b.z = bw[2]; b.w = bw[3];
        e += act;
        if (e < e_end) {
            u_nx = src[e];
            n_nx = esc[e];
            const float* fr = el.ef + (size_t)id_nx * F;
#pragma unroll
            for (int s = 0; s < 8; s++) f_nx[s] = fr[foff[s]];
        }
        if (e + 1 < e_end) id_nx = el.eid[e + 1];
        const float* hr = x + (size_t)u * D + 4 * g;
#pragma unroll
        for (int q0 = 0; q0 < NQ; q0 += M::KS) {
            if (q0) __builtin_amdgcn_sched_barrier(0);  // (one half row in flight, not both)
            float4 xv[M::KS];
#pragma unroll
            for (int q = 0; q < M::KS; q++)
                if (q0 + q < NQ) xv[q] = *reinterpret_cast<const float4*>(hr + GCWE_OFF(q0 + q));
#pragma unroll
            for (int q = 0; q < M::KS; q++)
                if (q0 + q < NQ) {
                    const ds_uint4_t wf = *reinterpret_cast<const ds_uint4_t*>(s_frag + (q0 + q) * 1024 + lane * 16);
                    const float4_t c = DS_MFMA16(wf, b, ((float4_t){0.f, 0.f, 0.f, 0.f}));
                    float r0 = __builtin_fmaf(norm, relu1(__builtin_fmaf(c.x, el_inv, xv[q].x)), a[4 * (q0 + q) + 0]);
                    float r1 = __builtin_fmaf(norm, relu1(__builtin_fmaf(c.y, el_inv, xv[q].y)), a[4 * (q0 + q) + 1]);
                    float r2 = __builtin_fmaf(norm, relu1(__builtin_fmaf(c.z, el_inv, xv[q].z)), a[4 * (q0 + q) + 2]);
                    float r3 = __builtin_fmaf(norm, relu1(__builtin_fmaf(c.w, el_inv, xv[q].w)), a[4 * (q0 + q) + 3]);
                    asm volatile("" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3));  // (computed in this trip, not carried into the next)
                    a[4 * (q0 + q) + 0] = r0; a[4 * (q0 + q) + 1] = r1; a[4 * (q0 + q) + 2] = r2; a[4 * (q0 + q) + 3] = r3;
                }
        }
    }
#undef GCWE_OFF
    *el.vmax = vmax;
}

}  // namespace
}  // namespace fg
