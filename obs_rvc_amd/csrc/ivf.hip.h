// ivf.hip.h -- IVF-probed retrieval: the structure's device-side build at attach time and the two launches of the per-chunk section.
// Included by retrieval.hip only.  The distance, the block-level top-K and the blend are knn.hip.h's device functions: a probe of every list returns the
// flat search's bits.
#pragma once
#include "knn.hip.h"

namespace rvc {

#define IVF_MAX_NLIST 65536
#define IVF_MAX_NPROBE 64
#define IVF_TC 16                      // ivf_coarse_kernel: centroids per workgroup ...
#define IVF_TQ 16                      // ... queries per workgroup (256 threads: one (centroid, query) pair each) ...
#define IVF_DC 256                     // ... dimensions per staged chunk
#define IVF_TILE 16640                 // ivf_scan_blend_kernel: floats of its row tile: 64 rows x (256 + 1), 128 x (128 + 1) or 256 x (64 + 1)

// ---- attach time: CSR offsets and the row permutation, by counting sort on the device ----
static __global__ void ivf_count_kernel(const int *assign, int n, int *counts)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicAdd(&counts[assign[i]], 1);
}
// exclusive prefix sum of counts[nlist] into offs[nlist + 1]; one workgroup of 256
static __global__ __launch_bounds__(256) void ivf_offsets_kernel(const int *counts, int nlist, int *offs)
{
    __shared__ int part[256];
    const int tid = threadIdx.x, per = (nlist + 255) / 256;
    const int lo = tid * per < nlist ? tid * per : nlist, hi = lo + per < nlist ? lo + per : nlist;
    int s = 0;
    for (int j = lo; j < hi; j++) s += counts[j];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; t++) { const int v = part[t]; part[t] = run; run += v; }
        offs[nlist] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int j = lo; j < hi; j++) { offs[j] = run; run += counts[j]; }
}
// one wave per list walks `assign` in row order and compacts its rows: ascending row numbers inside every list, no atomics, the same permutation every time
static __global__ __launch_bounds__(256) void ivf_fill_kernel(const int *assign, int n, int nlist, const int *offs, int *perm)
{
    const int lane = threadIdx.x & 63, l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= nlist) return;
    int at = offs[l];
    const int end = offs[l + 1];
    for (int base = 0; base < n && at < end; base += 64) {
        const int i = base + lane;
        const bool m = i < n && assign[i] == l;
        const unsigned long long mask = __ballot(m);
        if (m) perm[at + __popcll(mask & ((1ull << lane) - 1ull))] = i;
        at += __popcll(mask);
    }
}

// ---- per chunk, launch 1: every (query, centroid) distance ----
// The B x nq unique raw frames of all streams are one flat list of queries, so the centroid table is walked by ONE launch (grid = centroid tiles x groups of 16
// queries; groups beyond the first find the table in the L2 / Infinity Cache).  A workgroup holds its 16 queries in LDS and stages 16 centroids x 256 dimensions at
// a time with coalesced row-contiguous loads (the next chunk is requested before the current one is consumed); thread (centroid, query) walks the sequential
// chain from LDS, so no lane ever strides the table by a row.
struct IvfCoarseP {
    const float *cent; int nlist, dim;
    const float *cv; int cv_cs; long long cv_bs; int first_raw, nq, Q;      // query f = stream f / nq, raw frame first_raw + f % nq
    float *D;                                                                // [Q][nlist]
};
__host__ __device__ inline int ivf_qs(int dim) { return dim | 1; }           // odd row stride of the queries in LDS
static __global__ __launch_bounds__(256) void ivf_coarse_kernel(IvfCoarseP p)
{
    extern __shared__ __attribute__((aligned(16))) float s_q[];              // [IVF_TQ][QS]
    __shared__ float tile[IVF_TC][IVF_DC + 1];
    const int tid = threadIdx.x, ci = tid & 15, qi = tid >> 4;
    const int c0 = blockIdx.x * IVF_TC, f0 = blockIdx.y * IVF_TQ;
    const int nqg = p.Q - f0 < IVF_TQ ? p.Q - f0 : IVF_TQ, QS = ivf_qs(p.dim);
    float nx[IVF_TC];                                                        // this thread's column of the next chunk, one element per centroid row
    auto fetch = [&](int d0) {
#pragma unroll
        for (int u = 0; u < IVF_TC; u++) {
            const int cj = c0 + u, d = d0 + tid;
            nx[u] = (cj < p.nlist && d < p.dim) ? p.cent[(long long)cj * p.dim + d] : 0.f;
        }
    };
    fetch(0);
    for (int i = tid; i < IVF_TQ * p.dim; i += 256) {
        const int r = i & 15, c = i >> 4;
        if (r < nqg) {
            const int f = f0 + r, b = f / p.nq, j = f - b * p.nq;
            s_q[r * QS + c] = p.cv[(long long)b * p.cv_bs + (long long)c * p.cv_cs + p.first_raw + j];
        }
    }
    const float *xq = s_q + (qi < nqg ? qi : 0) * QS;                        // (pairs past the last query repeat the first: never written)
    float acc = 0.f;
    for (int d0 = 0; d0 < p.dim; d0 += IVF_DC) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < IVF_TC; u++) tile[u][tid] = nx[u];
        __syncthreads();
        if (d0 + IVF_DC < p.dim) fetch(d0 + IVF_DC);
        const int dn = p.dim - d0 < IVF_DC ? p.dim - d0 : IVF_DC;
        const float *yr = &tile[ci][0], *xr = xq + d0;
#pragma unroll 8
        for (int c = 0; c < dn; c++) acc = knn_dist_step(acc, xr[c], yr[c]);
    }
    if (qi < nqg && c0 + ci < p.nlist) p.D[(long long)(f0 + qi) * p.nlist + c0 + ci] = acc;
}

// ---- per chunk, launch 2: probe selection, exact scan of the probed lists, hits, blend ----
// One workgroup per (query, stream).  The nprobe smallest (D, j) are found by nprobe rounds of a workgroup minimum "beyond the previous pick" over the query's
// row of D, kept in LDS (a non-finite distance is no candidate, as in the flat search).  The probed lists' rows -- whole contiguous rows of the row-major matrix, gathered by
// id through the CSR -- are staged in LDS tiles of up to 256 rows; thread r walks row r's chain and keeps a sorted list of K (4 or 8: the plan's k).  No margin, no overflow word,
// no hand-off: every probed row is scanned exactly.
struct IvfScanP {
    const float *D; int nlist, nprobe;
    const int *offs, *perm; const float *index; int dim;
    const float *cv; int cv_cs; long long cv_bs; int first_raw, nq;
    int skip_head, T, R; float rate;
    float *phone; int ph_cs; long long ph_bs;
    int *out_idx; float *out_dist;     // [B][R][K]
    int *scanned;                      // [B][nq]: rows this query's probe set held (rvc_profile_last_knn)
};
template <int K> __device__ __forceinline__ void ivf_scan_blend_body(const IvfScanP p)
{
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];            // row tile [IVF_TILE] | the query [dim]
    __shared__ int s_row[256];
    __shared__ int s_pl[IVF_MAX_NPROBE], s_ps[IVF_MAX_NPROBE + 1];           // the probed lists, nearest first, and the running sum of their lengths
    __shared__ float wd[4][K]; __shared__ int wi[4][K];
    __shared__ float sd[K]; __shared__ int si[K];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *tile = s_dyn, *s_x = s_dyn + IVF_TILE;
    const float *cvb = p.cv + (long long)b * p.cv_bs + p.first_raw + j;
    for (int c = tid; c < p.dim; c += 256) s_x[c] = cvb[(long long)c * p.cv_cs];
    // 1. the probe set
    // (the query's row of D is read nprobe times: it waits in the row tile, which is free until the scan, whenever it fits -- 16 640 lists)
    const float *Dq = p.D + ((long long)b * p.nq + j) * p.nlist;
    if (p.nlist <= IVF_TILE) {
        for (int l = tid; l < p.nlist; l += 256) tile[l] = Dq[l];
        Dq = tile;
    }
    __syncthreads();
    float pd = -INFINITY; int pj = -1, np = 0;
    for (int r = 0; r < p.nprobe; r++) {
        float md = INFINITY; int mi = 0x7fffffff;
        for (int l = tid; l < p.nlist; l += 256) {
            const float d = Dq[l];
            const bool beyond = d > pd || (d == pd && l > pj);
            if (beyond && d < INFINITY && (d < md || (d == md && l < mi))) { md = d; mi = l; }
        }
        wave_min_pair(md, mi);
        if (lane == 0) { wd[wave][0] = md; wi[wave][0] = mi; }
        __syncthreads();
        md = wd[0][0]; mi = wi[0][0];
#pragma unroll
        for (int w = 1; w < 4; w++) { const float od = wd[w][0]; const int oi = wi[w][0]; if (od < md || (od == md && oi < mi)) { md = od; mi = oi; } }
        __syncthreads();
        if (mi == 0x7fffffff) break;                                         // (fewer finite distances than nprobe; the same in every thread)
        if (tid == 0) s_pl[np] = mi;
        np++; pd = md; pj = mi;
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int k = 0; k < np; k++) { s_ps[k] = run; run += p.offs[s_pl[k] + 1] - p.offs[s_pl[k]]; }
        s_ps[np] = run;
        p.scanned[b * p.nq + j] = run;
    }
    __syncthreads();
    const int total = s_ps[np];
    // 2. exact distances of the probed rows
    float bd[K]; int bi[K];
#pragma unroll
    for (int k = 0; k < K; k++) { bd[k] = INFINITY; bi[k] = 0x7fffffff; }
    for (int base = 0; base < total; base += 256) {
        const int nr = total - base < 256 ? total - base : 256;
        const int sh = nr <= 64 ? 8 : nr <= 128 ? 7 : 6, SD = 1 << sh, RS = SD + 1;      // dimensions per staged chunk: the fewer rows, the longer their pieces
        __syncthreads();
        int row = 0;
        if (tid < nr) {
            const int pos = base + tid;
            int k = 0;
            while (k + 1 < np && s_ps[k + 1] <= pos) k++;
            row = p.perm[p.offs[s_pl[k]] + pos - s_ps[k]];
        }
        s_row[tid] = row;
        float acc = 0.f;
        for (int d0 = 0; d0 < p.dim; d0 += SD) {
            __syncthreads();
            if ((p.dim & 3) == 0) {
                // (eight 16-byte loads in flight per thread: what a single workgroup pulls through its CU is bounded by the bytes it keeps in flight)
                const int cnt = nr << (sh - 2);
                for (int i0 = tid; i0 < cnt; i0 += 8 * 256) {
                    f32x4 y[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const int i = i0 + u * 256, r = i >> (sh - 2), c = (i & ((SD >> 2) - 1)) << 2;
                        if (i < cnt && d0 + c < p.dim) y[u] = *reinterpret_cast<const f32x4 *>(p.index + (long long)s_row[r] * p.dim + d0 + c);
                    }
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const int i = i0 + u * 256, r = i >> (sh - 2), c = (i & ((SD >> 2) - 1)) << 2;
                        if (i < cnt && d0 + c < p.dim) { float *t = tile + r * RS + c; t[0] = y[u][0]; t[1] = y[u][1]; t[2] = y[u][2]; t[3] = y[u][3]; }
                    }
                }
            } else {
                for (int i = tid; i < nr << sh; i += 256) {
                    const int r = i >> sh, c = i & (SD - 1);
                    if (d0 + c < p.dim) tile[r * RS + c] = p.index[(long long)s_row[r] * p.dim + d0 + c];
                }
            }
            __syncthreads();
            if (tid < nr) {
                const int dn = p.dim - d0 < SD ? p.dim - d0 : SD;
                const float *yr = tile + tid * RS, *xr = s_x + d0;
#pragma unroll 8
                for (int c = 0; c < dn; c++) acc = knn_dist_step(acc, xr[c], yr[c]);
            }
        }
        if (tid < nr && acc < INFINITY) {                                    // (a non-finite distance is no candidate)
            float cd = acc; int ci = row;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const bool sw = cd < bd[k] || (cd == bd[k] && ci < bi[k]);
                const float t0 = sw ? bd[k] : cd; const int t1 = sw ? bi[k] : ci;
                bd[k] = sw ? cd : bd[k]; bi[k] = sw ? ci : bi[k];
                cd = t0; ci = t1;
            }
        }
    }
    // 3. the K smallest (d, i) of the workgroup
    knn_block_topk(bd, bi, wd, wi, sd, si);
    // 4. hits and blend for the sliced frames that duplicate this raw frame; fewer than K hits: the frame keeps its raw feature
    const bool full = si[K - 1] != 0x7fffffff;
    float wn[K];
    knn_blend_weights(sd, wn);
    const int raw = j + p.first_raw;
    int r_lo = 2 * raw - p.skip_head, r_hi = raw >= p.T - 1 ? p.R : 2 * raw + 2 - p.skip_head;
    r_lo = r_lo < 0 ? 0 : r_lo; r_hi = r_hi > p.R ? p.R : r_hi;
    float *ph = p.phone + (long long)b * p.ph_bs;
    for (int c = tid; c < p.dim; c += 256) {
        const float val = full ? knn_blend_channel(p.index, p.dim, c, si, wn, p.rate, s_x[c]) : s_x[c];
        for (int r = r_lo; r < r_hi; r++) ph[(long long)c * p.ph_cs + r] = val;
    }
    if (tid < K)
        for (int r = r_lo; r < r_hi; r++) {
            p.out_idx[((long long)b * p.R + r) * K + tid] = si[tid] == 0x7fffffff ? -1 : si[tid];
            p.out_dist[((long long)b * p.R + r) * K + tid] = sd[tid];
        }
}
// the entry points: K = 4 under the kernel's own name (profiles and rvc_profile_last_knn know it), K = 8 beside it; the plan's k picks one (retrieval.hip)
static __global__ __launch_bounds__(256) void ivf_scan_blend_kernel(IvfScanP p) { ivf_scan_blend_body<KNN_K>(p); }
static __global__ __launch_bounds__(256) void ivf_scan_blend_k8_kernel(IvfScanP p) { ivf_scan_blend_body<KNN_KMAX>(p); }

}  // namespace rvc
