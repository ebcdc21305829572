// eigen.hip -- flowgnn_laplacian_eigen*: DGN's node_eigen, the eigenvectors of the four smallest eigenvalues of every graph's
// normalised Laplacian L = I - D^-1/2 A D^-1/2, computed on the GPU from the caller's edge list.
//
// One workgroup per graph, a cyclic two-sided Jacobi iteration on L in LDS.  Three instances by padded size P = 32 / 64 / 128 (the
// host sorts the graph ids into the classes, engine.hip), 4 P threads each; L and the accumulated rotations V are [P][P + 1] floats.
// In the rotation pass a row of lanes runs along a step's pairs k: it reads V[i][p_k] on banks (i + p_k) mod 32 and A[p_k][p_l] on
// banks (p_k + p_l) mod 32, and the p (and the q) of a step are distinct, so the odd row stride keeps both the column and the row
// rotations free of bank conflicts inside a row of lanes.  Plain LDS loads and stores, no LDS-DMA.
//
// Rotation order: round-robin pairing of m = n rounded up to even players, m / 2 disjoint pairs per step, m - 1 steps per sweep;
// the odd graph's extra player is a padding row that no rotation touches (the bye).  The rotations of a step are computed once (lane k
// for pair k) and then applied by the whole workgroup to the columns of V and, as J_k^T (.) J_l on disjoint 2 x 2 blocks, to A.
// Pairs, steps and the order of every sum depend on n alone, so a graph's vectors are bit-identical wherever the graph stands in a
// batch.
#include "common.h"

namespace fg {

// stop when ||off(A)||_F <= EIGEN_TOL * ||L||_F, at the latest after EIGEN_MAX_SWEEPS sweeps (scripts/dev/eigen_sweeps.py, the
// float32 transcription of this rotation order: the float32 floor of the ratio is 1e-7 .. 2e-7, 8 sweeps were the most any graph needed)
constexpr float EIGEN_TOL = 5e-7f;
constexpr int EIGEN_MAX_SWEEPS = 16;
constexpr int EIGEN_OUT = 4;  // columns of node_eigen

// the sum of v over the workgroup, the same bits in every thread: a butterfly inside the wave (both partners of a stage add the same
// two numbers), then the waves' sums in wave order
template <int T>
__device__ inline float eigen_block_sum(float v, float* s_red) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if constexpr (T > WAVE) {
        __syncthreads();  // (the previous sum's readers are done)
        if ((threadIdx.x & (WAVE - 1)) == 0) s_red[threadIdx.x / WAVE] = v;
        __syncthreads();
        v = s_red[0];
#pragma unroll
        for (int w = 1; w < T / WAVE; w++) v += s_red[w];
    }
    return v;
}

// the items t = tid, tid + T, ... < rows * m as (t / m, t % m), without a division per item
#define EIGEN_FOR_ITEMS(rows, row, col)                                                      \
    for (int row = (int)threadIdx.x / m, col = (int)threadIdx.x % m; row < (rows);           \
         col += step_r, row += step_q + (col >= m ? 1 : 0), col -= (col >= m ? m : 0))

template <int P>
__global__ __launch_bounds__(4 * P) void laplacian_eigen_kernel(const int* __restrict__ list, const int* __restrict__ noff,
                                                                const int* __restrict__ eoff, const void* __restrict__ edges,
                                                                long long E, int pyg, float* __restrict__ out) {
    constexpr int T = 4 * P, S = P + 1;
    __shared__ float s_a[P * S], s_v[P * S];
    __shared__ __attribute__((aligned(16))) float4 s_rot[P / 2];  // a step's rotations: c, s, p, q
    __shared__ float s_d[P];
    __shared__ float s_red[T / WAVE];
    __shared__ int s_sel[EIGEN_OUT];
    const int tid = threadIdx.x;
    const int g = list[blockIdx.x];
    const int n0 = noff[g], n = noff[g + 1] - n0;
    if (n < 1 || n > P) return;  // (the host sorted the graphs by size: never taken)
    const int m = n + (n & 1);
    const int step_q = T / m, step_r = T % m;
    const int h = m / 2;                          // pairs per step
    const int lane_rows = T / h;                  // the rotation pass: lane groups of h threads, one per pair
    const int my_k = tid % h, my_0 = tid / h;     // this thread's pair, and its first row / partner pair

    for (int t = tid; t < m * S; t += T) { s_a[t] = 0.0f; s_v[t] = 0.0f; }
    if (tid < EIGEN_OUT) s_sel[tid] = 0;  // (a graph of fewer than four nodes fills only the first n)
    __syncthreads();
    // adjacency entries first: 1 for every edge u != v with both ends inside the graph, whatever the direction or the multiplicity
    const int e0 = eoff[g], e1 = eoff[g + 1];
    for (int e = e0 + tid; e < e1; e += T) {
        long long u, v;
        if (pyg) {
            const long long* ei = static_cast<const long long*>(edges);
            u = ei[e] - n0;
            v = ei[E + e] - n0;
        } else {
            const int2 uv = static_cast<const int2*>(edges)[e];
            u = uv.x;
            v = uv.y;
        }
        if (u != v && u >= 0 && u < n && v >= 0 && v < n) {
            s_a[(int)u * S + (int)v] = 1.0f;
            s_a[(int)v * S + (int)u] = 1.0f;
        }
    }
    if (tid < m) s_v[tid * S + tid] = 1.0f;
    __syncthreads();
    // degrees = row sums of the finished 0/1 matrix; the padding row gets 0, which keeps its off-diagonal at 0
    if (tid < m) {
        float deg = 0.0f;
        for (int j = 0; j < n; j++) deg += s_a[tid * S + j];
        s_d[tid] = tid < n ? 1.0f / sqrtf(fmaxf(deg, 1.0f)) : 0.0f;
    }
    __syncthreads();
    float part = 0.0f;
    EIGEN_FOR_ITEMS(m, i, j) {
        const float l = (i == j ? 1.0f : 0.0f) - s_d[i] * s_a[i * S + j] * s_d[j];
        s_a[i * S + j] = l;
        if (i < n && j < n) part += l * l;
    }
    const float fro2 = eigen_block_sum<T>(part, s_red);
    __syncthreads();

    for (int sweep = 0; sweep < EIGEN_MAX_SWEEPS; sweep++) {
        part = 0.0f;
        EIGEN_FOR_ITEMS(m, i, j) {
            const float a = s_a[i * S + j];
            part += i == j ? 0.0f : a * a;
        }
        const float off2 = eigen_block_sum<T>(part, s_red);  // the same bits in every thread: one decision for the workgroup
        if (off2 <= EIGEN_TOL * EIGEN_TOL * fro2) break;
        for (int r = 0; r < m - 1; r++) {
            if (tid < m / 2) {
                int p = r + tid, q = r - tid;
                if (p >= m - 1) p -= m - 1;
                if (q < 0) q += m - 1;
                if (tid == 0) p = m - 1;
                const float app = s_a[p * S + p], aqq = s_a[q * S + q], apq = s_a[p * S + q];
                // a zero or tiny pivot, or the bye: the identity rotation, by selects
                const bool skip = fabsf(apq) < 1e-30f || p >= n || q >= n;
                const float theta = (aqq - app) / (2.0f * (skip ? 1.0f : apq));
                float t = copysignf(1.0f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
                t = skip ? 0.0f : t;
                const float c = 1.0f / sqrtf(t * t + 1.0f);
                s_rot[tid] = make_float4(c, t * c, __int_as_float(p), __int_as_float(q));
            }
            __syncthreads();
            // One pass applies the step to V (columns) and to A (both sides).  A thread keeps ONE pair k for the whole kernel, so its
            // rotation is read once per step: lanes run along the pairs, rows / partner pairs along the lane groups.
            if (tid < lane_rows * h) {
                const float4 rk = s_rot[my_k];
                const float ck = rk.x, sk = rk.y;
                const int pk = __float_as_int(rk.z), qk = __float_as_int(rk.w);
                // V J_k: columns pk, qk of rows my_0, my_0 + lane_rows, ...; two rows per trip, their loads before the first store
                for (int i = my_0; i < m; i += 2 * lane_rows) {
                    const int i2 = i + lane_rows;
                    const bool two = i2 < m;
                    const int b0 = i * S, b1 = (two ? i2 : i) * S;
                    const float vp0 = s_v[b0 + pk], vq0 = s_v[b0 + qk], vp1 = s_v[b1 + pk], vq1 = s_v[b1 + qk];
                    s_v[b0 + pk] = ck * vp0 - sk * vq0;
                    s_v[b0 + qk] = sk * vp0 + ck * vq0;
                    if (two) {
                        s_v[b1 + pk] = ck * vp1 - sk * vq1;
                        s_v[b1 + qk] = sk * vp1 + ck * vq1;
                    }
                }
                // J_k^T A J_l on the 2 x 2 block (rows pk, qk; columns pl, ql) of partner pairs l = my_0, my_0 + lane_rows, ...: the
                // blocks are disjoint, so A's column and row rotations are one read and one write of every element
                for (int l = my_0; l < h; l += lane_rows) {
                    const float4 rl = s_rot[l];
                    const float cl = rl.x, sl = rl.y;
                    const int pl = __float_as_int(rl.z), ql = __float_as_int(rl.w);
                    const float a = s_a[pk * S + pl], b = s_a[pk * S + ql], c = s_a[qk * S + pl], d = s_a[qk * S + ql];
                    const float a1 = cl * a - sl * b, b1 = sl * a + cl * b, c1 = cl * c - sl * d, d1 = sl * c + cl * d;
                    s_a[pk * S + pl] = ck * a1 - sk * c1;
                    s_a[pk * S + ql] = ck * b1 - sk * d1;
                    s_a[qk * S + pl] = sk * a1 + ck * c1;
                    s_a[qk * S + ql] = sk * b1 + ck * d1;
                }
            }
            __syncthreads();
        }
    }

    // the four smallest diagonal entries, ascending, the index as tie-break
    __syncthreads();
    if (tid < n) s_d[tid] = s_a[tid * S + tid];
    __syncthreads();
    if (tid < n) {
        const float d = s_d[tid];
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const float o = s_d[j];
            rank += (o < d || (o == d && j < tid)) ? 1 : 0;
        }
        if (rank < EIGEN_OUT) s_sel[rank] = tid;
    }
    __syncthreads();
    float* const dst = out + (size_t)n0 * EIGEN_OUT;
    for (int t = tid; t < n * EIGEN_OUT; t += T) {  // consecutive lanes, consecutive addresses; columns k >= n are 0
        const int i = t / EIGEN_OUT, k = t % EIGEN_OUT;
        dst[t] = k < n ? s_v[i * S + s_sel[k]] : 0.0f;
    }
}
#undef EIGEN_FOR_ITEMS

// the graphs list[0 .. count) of size class cls (0: up to 32 nodes, 1: up to 64, 2: up to 128), one workgroup each
void launch_laplacian_eigen(int cls, const int* list, int count, const int* noff, const int* eoff, const void* edges, long long E,
                            bool pyg, float* out, hipStream_t s) {
    if (count <= 0) return;
    if (cls == 0) laplacian_eigen_kernel<32><<<count, 128, 0, s>>>(list, noff, eoff, edges, E, pyg ? 1 : 0, out);
    else if (cls == 1) laplacian_eigen_kernel<64><<<count, 256, 0, s>>>(list, noff, eoff, edges, E, pyg ? 1 : 0, out);
    else laplacian_eigen_kernel<128><<<count, 512, 0, s>>>(list, noff, eoff, edges, E, pyg ? 1 : 0, out);
}

}  // namespace fg
