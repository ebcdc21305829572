// ingest.hip -- flowgnn_set_batch_device: a batch that is already in GPU memory, in PyG's layout, into the engine's int32 arrays.
//
// A PyG `Batch` on the device holds x int64 [N][9], edge_index int64 [2][E] with batch-global node ids and edge_attr int64 [E][3],
// the edges grouped by graph.  The model kernels read int32 [N][9], int32 [E][2] with ids local to each graph and int32 [E][3]
// (d_nf / d_el / d_ea) and validate them themselves (ERR_EDGE_RANGE / ERR_EDGE_ATTR / ERR_NODE_FEAT), so the ingest is one
// streaming pass that narrows, transposes and localises, and maps what it cannot represent to -1, which that validation refuses
// with the code a host caller would get.  It never reads memory by an id value: bad ids cannot make it fault.
// (The reference layout -- int32 arrays exactly as flowgnn_set_batch takes them -- needs no kernel: engine.hip copies it.)
#include "common.h"
#include <algorithm>

namespace fg {

constexpr int INGEST_THREADS = 256;
constexpr int INGEST_EDGES_PER_WAVE_STEP = 2 * WAVE;  // an edge pair per lane

__device__ inline int narrow_or_neg1(long long v, bool& bad) {
    const bool fits = v == (long long)(int)v;
    bad |= !fits;
    return fits ? (int)v : -1;
}

// int64 -> int32, element for element (x and edge_attr); a value outside int32 becomes -1, and sets *err to err_code when that is
// not 0.  vec: `in` is 16-B aligned, so four values per lane come in as two 16-B loads and leave as one 16-B store (`out` is the
// start of an engine allocation).
__device__ inline void ingest_narrow(const long long* __restrict__ in, int* __restrict__ out, long long n, bool vec, int* err,
                                     int err_code) {
    const long long tid = (long long)blockIdx.x * INGEST_THREADS + threadIdx.x;
    const long long stride = (long long)gridDim.x * INGEST_THREADS;
    bool bad = false;
    long long done = 0;
    if (vec) {
        const long long n4 = n / 4;
        for (long long q = tid; q < n4; q += stride) {
            const longlong2 a = reinterpret_cast<const longlong2*>(in)[2 * q];
            const longlong2 b = reinterpret_cast<const longlong2*>(in)[2 * q + 1];
            int4 o;
            o.x = narrow_or_neg1(a.x, bad);
            o.y = narrow_or_neg1(a.y, bad);
            o.z = narrow_or_neg1(b.x, bad);
            o.w = narrow_or_neg1(b.y, bad);
            reinterpret_cast<int4*>(out)[q] = o;
        }
        done = n4 * 4;
    }
    for (long long i = done + tid; i < n; i += stride) out[i] = narrow_or_neg1(in[i], bad);
    if (bad && err_code) atomicMax(err, err_code);
}

// edge_index [2][E] (global ids) -> [E][2] (ids local to the edge's graph; outside [noff[g], noff[g + 1]): -1).  Wave w owns the
// contiguous edges [w * span, (w + 1) * span) (span a multiple of 128) and walks them 128 at a time, lane l taking the pair
// 2l, 2l + 1 of each step: a lane finds its first edge's graph by one search in eoff and walks forward from there (a step moves
// 128 edges, two or three molecules).  vec: both rows 16-B aligned (E even), so a pair comes in as one 16-B load per row.
__device__ inline void ingest_edges(const long long* __restrict__ ei, int* __restrict__ el, const int* __restrict__ noff,
                                    const int* __restrict__ eoff, int G, long long E, long long span, bool vec) {
    const long long wave = ((long long)blockIdx.x * INGEST_THREADS + threadIdx.x) / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    const long long w0 = wave * span;
    const long long w1 = w0 + span < E ? w0 + span : E;
    const long long* __restrict__ src = ei;
    const long long* __restrict__ dst = ei + E;
    int g = -1;
    for (long long e0 = w0 + 2 * lane; e0 < w1; e0 += INGEST_EDGES_PER_WAVE_STEP) {
        const bool pair = e0 + 1 < w1;
        if (g < 0) {  // the last graph whose first edge is <= e0 (it has e0: eoff[G] = E > e0)
            int lo = 0, hi = G - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (eoff[mid] <= e0) lo = mid; else hi = mid - 1;
            }
            g = lo;
        }
        long long s0, d0, s1 = 0, d1 = 0;
        if (vec && pair) {
            const longlong2 s = *reinterpret_cast<const longlong2*>(src + e0);
            const longlong2 d = *reinterpret_cast<const longlong2*>(dst + e0);
            s0 = s.x; s1 = s.y; d0 = d.x; d1 = d.y;
        } else {
            s0 = src[e0]; d0 = dst[e0];
            if (pair) { s1 = src[e0 + 1]; d1 = dst[e0 + 1]; }
        }
        while (eoff[g + 1] <= e0) g++;
        long long lo = noff[g], hi = noff[g + 1];
        int2 a;
        a.x = s0 >= lo && s0 < hi ? (int)(s0 - lo) : -1;
        a.y = d0 >= lo && d0 < hi ? (int)(d0 - lo) : -1;
        if (pair) {
            while (eoff[g + 1] <= e0 + 1) g++;
            lo = noff[g]; hi = noff[g + 1];
            int4 o;
            o.x = a.x; o.y = a.y;
            o.z = s1 >= lo && s1 < hi ? (int)(s1 - lo) : -1;
            o.w = d1 >= lo && d1 < hi ? (int)(d1 - lo) : -1;
            reinterpret_cast<int4*>(el)[e0 / 2] = o;  // (e0 even: 16-B aligned in the engine's allocation)
        } else {
            reinterpret_cast<int2*>(el)[e0] = a;
        }
    }
}

// One launch, three streams of work one after the other in every thread: x, edge_index, edge_attr (ea / ea_out null: the model has
// no edge features).  x_err: the code an x value outside int32 sets in the engine's error word directly (GAT, whose features are raw
// numbers, for which -1 is valid input), 0: leave it to the model's own validation of the -1.
__global__ __launch_bounds__(INGEST_THREADS) void ingest_pyg_kernel(const long long* __restrict__ x, const long long* __restrict__ ei,
                                                                    const long long* __restrict__ ea, int* __restrict__ nf,
                                                                    int* __restrict__ el, int* __restrict__ ea_out,
                                                                    const int* __restrict__ noff, const int* __restrict__ eoff, int G,
                                                                    long long N, long long E, long long span, int vec_mask, int* err,
                                                                    int x_err) {
    ingest_narrow(x, nf, N * ND_FEATURE, vec_mask & 1, err, x_err);
    if (E > 0) ingest_edges(ei, el, noff, eoff, G, E, span, vec_mask & 2);
    if (ea && ea_out) ingest_narrow(ea, ea_out, E * EDGE_ATTR, vec_mask & 4, err, 0);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

void launch_ingest_pyg(const long long* x, const long long* ei, const long long* ea, int* nf, int* el, int* ea_out, const int* noff,
                       const int* eoff, int G, long long N, long long E, int* err, int x_err, int device, hipStream_t s) {
    if (N <= 0) return;  // (no graphs)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) { (void)hipGetLastError(); cus = 256; }
    // four blocks of 256 per CU (16 waves of 32: enough loads in flight for HBM), fewer when the batch has less work than that
    const long long work = std::max({N * ND_FEATURE / 4, E / 2, E * EDGE_ATTR / 4, 1LL});
    const long long blocks = std::min((long long)cus * 4, (work + INGEST_THREADS - 1) / INGEST_THREADS);
    const long long waves = blocks * (INGEST_THREADS / WAVE);
    const long long span = ceil_div_ll(ceil_div_ll(E, waves), INGEST_EDGES_PER_WAVE_STEP) * INGEST_EDGES_PER_WAVE_STEP;
    const int vec = (aligned16(x) ? 1 : 0) | (aligned16(ei) && E % 2 == 0 ? 2 : 0) | (ea && aligned16(ea) ? 4 : 0);
    ingest_pyg_kernel<<<(int)blocks, INGEST_THREADS, 0, s>>>(x, ei, ea, nf, el, ea_out, noff, eoff, G, N, E, span, vec, err, x_err);
}

}  // namespace fg
