// kmeans.hip.h -- k-means training of an IVF structure over the loaded index: Lloyd's algorithm on the matrix that is already in HBM.
// Included by retrieval.hip only.  The distance is knn.hip.h's knn_dist_step chain, argument order (row, centroid) as ivf_coarse_kernel uses (query, centroid), so
// the assignment training ends with is the exact argmin under the chain the probe walks.  The CSR of an assignment is ivf.hip.h's counting sort, called as it is.
#pragma once
#include "knn.hip.h"
#include "ivf.hip.h"

namespace rvc {

#define KM_TR 64                       // kmeans_assign_kernel: rows per workgroup ...
#define KM_TC 64                       // ... centroids per streamed tile (256 threads: a 4 x 4 block of (row, centroid) chains each) ...
#define KM_DC 32                       // ... dimensions per staged chunk
#define KM_RB 256                      // kmeans_objective_kernel: distances per partial

// ---- before training: the first row that holds a NaN or an Inf (a non-finite norm of install_index is only a hint: a finite row's norm can overflow) ----
static __global__ void kmeans_nonfinite_kernel(const float *index, const float *ynorm, int n, int dim, int *first)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || ynorm[i] - ynorm[i] == 0.f) return;
    const float *r = index + (long long)i * dim;
    for (int d = 0; d < dim; d++)
        if (!(r[d] - r[d] == 0.f)) { atomicMin(first, i); return; }
}

// ---- init: c_j = y_{rows[j]}, bit for bit ----
static __global__ void kmeans_gather_kernel(const float *index, int dim, const int *rows, float *cent)
{
    const int j = blockIdx.x;
    const unsigned *src = reinterpret_cast<const unsigned *>(index) + (long long)rows[j] * dim;
    unsigned *dst = reinterpret_cast<unsigned *>(cent) + (long long)j * dim;
    for (int c = threadIdx.x; c < dim; c += blockDim.x) dst[c] = src[c];
}

// ---- assign step: assign[i] = the j with the smallest (d(y_i, c_j), j); a non-finite distance compares as +inf ----
// A workgroup owns KM_TR rows and streams every tile of KM_TC centroids past them, KM_DC dimensions at a time: both tiles are staged in LDS with row-contiguous
// coalesced loads, the next chunk requested before the current one is consumed.  Thread (tr, tc) = (tid >> 4, tid & 15) walks the 16 chains of rows tr + 16 u and
// centroids tc + 16 v in ascending dimension, so one LDS read feeds four chains; each chain is the sequential knn_dist_step chain of the definition.  Behind a
// centroid tile the thread folds its four distances per row into a running best (d, j); behind the last tile the 16 threads that share a row merge in the (d, j)
// order.  No [n][nlist] matrix exists anywhere.  moved_wg[workgroup] = its rows whose list changed against prev (all of them when prev is null).
struct KmeansAssignP {
    const float *index; int n, dim;
    const float *cent; int nlist;
    const int *prev; int *assign; float *dist; int *moved_wg;
};
static __global__ __launch_bounds__(256) void kmeans_assign_kernel(KmeansAssignP p)
{
    __shared__ float sx[KM_TR][KM_DC + 1], sy[KM_TC][KM_DC + 1];
    __shared__ int s_moved;
    const int tid = threadIdx.x, tc = tid & 15, tr = tid >> 4;
    const int r0 = blockIdx.x * KM_TR;
    const int nch = (p.dim + KM_DC - 1) / KM_DC, ntile = (p.nlist + KM_TC - 1) / KM_TC, nstep = nch * ntile;
    if (tid == 0) s_moved = 0;
    float nx[8], ny[8];                                                      // this thread's share of the next chunk: element e = tid + 256 k -> (row e >> 5, dimension e & 31)
    auto fetch = [&](int step) {
        const int c0 = (step / nch) * KM_TC, d = (step % nch) * KM_DC + (tid & 31);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int r = (tid >> 5) + 8 * k;
            nx[k] = (r0 + r < p.n && d < p.dim) ? p.index[(long long)(r0 + r) * p.dim + d] : 0.f;
            ny[k] = (c0 + r < p.nlist && d < p.dim) ? p.cent[(long long)(c0 + r) * p.dim + d] : 0.f;
        }
    };
    float bd[4]; int bj[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { bd[u] = INFINITY; bj[u] = 0x7fffffff; }
    float acc[4][4];
    fetch(0);
    for (int step = 0; step < nstep; step++) {
        const int ch = step % nch, c0 = (step / nch) * KM_TC;
        if (ch == 0) {
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int v = 0; v < 4; v++) acc[u][v] = 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; k++) { sx[(tid >> 5) + 8 * k][tid & 31] = nx[k]; sy[(tid >> 5) + 8 * k][tid & 31] = ny[k]; }
        __syncthreads();
        if (step + 1 < nstep) fetch(step + 1);
        const int dn = p.dim - ch * KM_DC < KM_DC ? p.dim - ch * KM_DC : KM_DC;
#pragma unroll 4
        for (int c = 0; c < dn; c++) {
            float x[4], y[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { x[u] = sx[tr + 16 * u][c]; y[u] = sy[tc + 16 * u][c]; }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int v = 0; v < 4; v++) acc[u][v] = knn_dist_step(acc[u][v], x[u], y[v]);
        }
        if (ch == nch - 1) {
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int v = 0; v < 4; v++) {                                // (ascending j inside the thread)
                    const int j = c0 + tc + 16 * v;
                    const float d = acc[u][v] < INFINITY ? acc[u][v] : INFINITY;         // (a NaN or an Inf compares as +inf)
                    if (j < p.nlist && (d < bd[u] || (d == bd[u] && j < bj[u]))) { bd[u] = d; bj[u] = j; }
                }
        }
    }
    int moved = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        float d = bd[u]; int j = bj[u];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {                                    // the 16 threads of a row are 16 neighbouring lanes
            const float od = __shfl_xor(d, o, 64); const int oj = __shfl_xor(j, o, 64);
            if (od < d || (od == d && oj < j)) { d = od; j = oj; }
        }
        const int i = r0 + tr + 16 * u;
        if (tc == 0 && i < p.n) {
            p.assign[i] = j; p.dist[i] = d;
            moved += !p.prev || p.prev[i] != j;
        }
    }
    if (moved) atomicAdd(&s_moved, moved);
    __syncthreads();
    if (tid == 0) p.moved_wg[blockIdx.x] = s_moved;
}

// ---- objective: J = sum of dist[] in fp64, in a fixed order ----
// A workgroup's 256 values (or the partials of a stripe) are added by one binary tree over the thread number: t += t + 128, t += t + 64, ..., t += t + 1.
// kmeans_objective_kernel: part[b] = the tree over dist[256 b .. 256 b + 255] (values past n are 0).  kmeans_objective_final_kernel (one workgroup): thread t adds
// part[t], part[t + 256], ... in ascending order, then the same tree; it also adds the workgroups' moved counts (integers: any order).
__device__ __forceinline__ double kmeans_tree_sum(double v, double *s)
{
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) s[tid] = s[tid] + s[tid + h];
        __syncthreads();
    }
    return s[0];
}
static __global__ __launch_bounds__(256) void kmeans_objective_kernel(const float *dist, int n, double *part)
{
    __shared__ double s[256];
    const int i = blockIdx.x * KM_RB + threadIdx.x;
    const double v = kmeans_tree_sum(i < n ? (double)dist[i] : 0.0, s);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}
static __global__ __launch_bounds__(256) void kmeans_objective_final_kernel(const double *part, int nparts, const int *moved_wg, int nwg, double *obj, long long *moved)
{
    __shared__ double s[256];
    __shared__ long long s_m;
    if (threadIdx.x == 0) s_m = 0;
    double v = 0.0;
    for (int b = threadIdx.x; b < nparts; b += 256) v += part[b];
    const double total = kmeans_tree_sum(v, s);
    long long m = 0;
    for (int b = threadIdx.x; b < nwg; b += 256) m += moved_wg[b];
    if (m) atomicAdd((unsigned long long *)&s_m, (unsigned long long)m);
    __syncthreads();
    if (threadIdx.x == 0) { *obj = total; *moved = s_m; }
}

// ---- update step: c_j = fp32(sum of the list's rows in fp64 / count), rows in ascending row number (the CSR's order); an empty list keeps its centroid ----
// One workgroup per list, one thread per dimension (strided by 256): the threads of a wave read neighbouring floats of one row.  No atomics: the same bits every run.
static __global__ __launch_bounds__(256) void kmeans_update_kernel(const float *index, int dim, const int *offs, const int *perm, float *cent)
{
    const int l = blockIdx.x, lo = offs[l], hi = offs[l + 1];
    if (hi == lo) return;
    const double cnt = (double)(hi - lo);
    for (int c = threadIdx.x; c < dim; c += 256) {
        double acc = 0.0;
        for (int q = lo; q < hi; q++) acc += (double)index[(long long)perm[q] * dim + c];
        cent[(long long)l * dim + c] = (float)(acc / cnt);
    }
}

}  // namespace rvc
