// ogbvn_dense.h -- the two dense steps of OGB's virtual-node update, vn' = relu(W2 relu(W1 t + b1) + b2), for the OV_GPW graphs of one
// 256-thread workgroup: device code shared by gin_ogbvn_kernel (gin_ogbvn.hip) and gcn_ogbvn_update_kernel
// (gcn_ogbvn.hip).  The callers differ in how they form t; from s_t on they are the same instructions.
#pragma once
#include "gin_ogbvn.h"

namespace fg {
namespace ov {

constexpr int OV_D = GIN_OGBVN_D, OV_H = GIN_OGBVN_H, OV_C = OV_D / 4, OV_GPW = GIN_OGBVN_GPW;
constexpr int OV_SLAB = 4000;   // floats per weight slab: 20 k-rows of W1^T [k][200], or 40 k-rows of W2^T [k][100]
constexpr int OV_SLABS = 10;    // five of each
constexpr int OV_PRE = (OV_SLAB / 4 + 255) / 256;  // float4 per thread per slab

__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float ov_relu(float x) { return x > 0.0f ? x : 0.0f; }
__device__ __forceinline__ float4 ov_relu4(float4 a) { return make_float4(ov_relu(a.x), ov_relu(a.y), ov_relu(a.z), ov_relu(a.w)); }
__device__ __forceinline__ float4 ov_fma4(float4 w, float t, float4 a) {  // a + w t, one rounding each
    return make_float4(__builtin_fmaf(w.x, t, a.x), __builtin_fmaf(w.y, t, a.y), __builtin_fmaf(w.z, t, a.z), __builtin_fmaf(w.w, t, a.w));
}

// float4 number i of a thread's share of a slab (clamped: the threads past the slab's end load its last one again and store nothing)
__device__ __forceinline__ int ov_pre_index(int tid, int i) { return tid + 256 * i < OV_SLAB / 4 ? tid + 256 * i : OV_SLAB / 4 - 1; }

// hid = relu(W1 t + b1), vn' = relu(W2 hid + b2) for the workgroup's graphs g0 .. g0 + OV_GPW - 1; weights in ten 16 KB slabs.
// wl: one update's W1^T | W2^T | b1 | b2 (gin_ogbvn.h).  s_t [OV_GPW][100] is complete for every thread's share when this is entered
// (the first trip's barrier orders it); s_w [OV_SLAB], s_hid [OV_GPW][200] are the caller's LDS.  Called by all 256 threads.
// dense 1: thread (og, gq) = four hidden units 4 og .. 4 og + 3 of graphs 4 gq .. 4 gq + 3      (200 threads)
// dense 2: thread (og, gp) = four outputs 4 og .. 4 og + 3 of graphs 2 gp, 2 gp + 1             (200 threads)
__device__ __forceinline__ void ogbvn_dense_steps(const float* __restrict__ wl, float* s_w, const float* s_t, float* s_hid,
                                                  float* vn_out, int g0, int num_graphs, int tid) {
    const float* b1 = wl + 2 * OV_D * OV_H;
    const float* b2 = b1 + OV_H;
    const bool on = tid < 200;
    const int og1 = tid % 50, gq = tid / 50, og2 = tid % OV_C, gp = tid / OV_C;
    float4 a1[4], a2[2];  // (threads beyond the 200: a clamped bias, computed on nothing, never stored)
    {
        const float4 b = reinterpret_cast<const float4*>(b1)[on ? og1 : 0];
        const float4 bb = reinterpret_cast<const float4*>(b2)[og2];
#pragma unroll
        for (int g = 0; g < 4; g++) a1[g] = b;
#pragma unroll
        for (int g = 0; g < 2; g++) a2[g] = bb;
    }
    // a thread's share of a slab: four float4 (named, not an array: hipcc keeps an array that lives across the slab loop in scratch)
    static_assert(OV_PRE == 4, "four prefetch registers");
    const float4* wl4 = reinterpret_cast<const float4*>(wl);
    const int i0 = ov_pre_index(tid, 0), i1 = ov_pre_index(tid, 1), i2 = ov_pre_index(tid, 2), i3 = ov_pre_index(tid, 3);
    float4 p0 = wl4[i0], p1 = wl4[i1], p2 = wl4[i2], p3 = wl4[i3];
#pragma unroll 1
    for (int sl = 0; sl < OV_SLABS; sl++) {
        __syncthreads();  // the slab before is consumed (first trip: s_t is complete; sixth: s_hid is)
        float4* sw4 = reinterpret_cast<float4*>(s_w);
        sw4[i0] = p0; sw4[i1] = p1; sw4[i2] = p2; sw4[i3] = p3;  // (a clamped index: the same value to the same place)
        __syncthreads();
        if (sl + 1 < OV_SLABS) {  // the next slab's loads fly under this slab's FMAs
            const float4* nx = wl4 + (size_t)(sl + 1) * (OV_SLAB / 4);
            p0 = nx[i0]; p1 = nx[i1]; p2 = nx[i2]; p3 = nx[i3];
        }
        if (!on) continue;
        if (sl < 5) {
            const int k0 = sl * 20;
#pragma unroll 1
            for (int kk = 0; kk < 20; kk += 4) {
                float4 w[4];
#pragma unroll
                for (int j = 0; j < 4; j++) w[j] = reinterpret_cast<const float4*>(s_w + (kk + j) * OV_H)[og1];
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const float4 t = *reinterpret_cast<const float4*>(s_t + (4 * gq + g) * OV_D + k0 + kk);
                    // k ascending: one chain per (graph, unit)
                    a1[g] = ov_fma4(w[0], t.x, a1[g]); a1[g] = ov_fma4(w[1], t.y, a1[g]);
                    a1[g] = ov_fma4(w[2], t.z, a1[g]); a1[g] = ov_fma4(w[3], t.w, a1[g]);
                }
            }
            if (sl == 4) {
#pragma unroll
                for (int g = 0; g < 4; g++)
                    reinterpret_cast<float4*>(s_hid + (4 * gq + g) * OV_H)[og1] = ov_relu4(a1[g]);
            }
        } else {
            const int k0 = (sl - 5) * 40;
#pragma unroll 1
            for (int kk = 0; kk < 40; kk += 4) {
                float4 w[4];
#pragma unroll
                for (int j = 0; j < 4; j++) w[j] = reinterpret_cast<const float4*>(s_w + (kk + j) * OV_D)[og2];
#pragma unroll
                for (int g = 0; g < 2; g++) {
                    const float4 t = *reinterpret_cast<const float4*>(s_hid + (2 * gp + g) * OV_H + k0 + kk);
                    a2[g] = ov_fma4(w[0], t.x, a2[g]); a2[g] = ov_fma4(w[1], t.y, a2[g]);
                    a2[g] = ov_fma4(w[2], t.z, a2[g]); a2[g] = ov_fma4(w[3], t.w, a2[g]);
                }
            }
        }
    }
    if (on) {
#pragma unroll
        for (int g = 0; g < 2; g++) {
            const int gg = g0 + 2 * gp + g;
            if (gg < num_graphs) reinterpret_cast<float4*>(vn_out + (size_t)gg * OV_D)[og2] = ov_relu4(a2[g]);
        }
    }
}

}  // namespace ov
}  // namespace fg
