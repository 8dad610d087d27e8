// knn.hip.h -- the kernels of the flat-L2 retrieval: index layouts, the scan / merge pair, the one-launch scan + select, the matrix-core candidate search.
// Included by retrieval.hip only (KNN_K: state.hip.h); ivf.hip.h builds on its distance and blend device functions.
#pragma once
#include "igemm_common.hip.h"
#include "state.hip.h"
#include "reduce.hip.h"

namespace rvc {

// ------------------------------------------------------------------------------------
// flat-L2 retrieval (rvc.rs:159 is a TODO; definition in SURVEY.md Appendix A.4).
// Stage 1: every thread owns one index vector (transposed index [dim][n] -> coalesced) and
// accumulates exact sequential-fmaf distances to all queries of its stream; each workgroup
// keeps its own top-K per query (K = 4, or 8: the plan's k; every kernel body here is template <int K>, instantiated for both behind two plain entry points, one of which the plan picks).  Stage 2 merges the per-workgroup candidates
// (ascending (distance, index)), forms w = (1/d)^2 and blends.
// ------------------------------------------------------------------------------------
// The engine's exact distance d(x, y) (tests/knn_ref.py): an fp32 sequential fmaf chain over the rounded differences (x[c] - y[c]) in
// ascending c.  knn_dist_step is one link of it; every kernel that owes the definition's bits (the exhaustive scan, the exact re-rank, the IVF coarse and
// fine scans of ivf.hip.h) goes through it, whatever it stages its operands in.
__device__ __forceinline__ float knn_dist_step(float acc, float x, float y) { const float df = x - y; return fmaf(df, df, acc); }
__device__ __forceinline__ float knn_dist_exact(const float *x, const float *y, int dim)
{
    float acc = 0.f;
    for (int d = 0; d < dim; d++) acc = knn_dist_step(acc, x[d], y[d]);
    return acc;
}
// The blend: w = (1/d)^2 normalised over the K hits (K = 4, or upstream's 8: rvc_set_index_k), feat = rate * sum w_k y_k + (1 - rate) * x,
// the sum accumulated by fmaf in ascending hit order.  A hit without a row (-1 or the 0x7fffffff sentinel: a non-finite query) contributes nothing.  One
// definition for every blend kernel, so that they agree bit for bit.
template <int K> __device__ __forceinline__ void knn_blend_weights(const float *sd, float (&wn)[K])
{
    float ws = 0.f;
#pragma unroll
    for (int k = 0; k < K; k++) { const float inv = 1.0f / sd[k]; wn[k] = inv * inv; ws += wn[k]; }
#pragma unroll
    for (int k = 0; k < K; k++) wn[k] = wn[k] / ws;
}
template <int K> __device__ __forceinline__ float knn_blend_channel(const float *index, int dim, int c, const int *si, const float (&wn)[K], float rate, float x)
{
    float y[K];
#pragma unroll
    for (int k = 0; k < K; k++) y[k] = (si[k] >= 0 && si[k] != 0x7fffffff) ? index[(long long)si[k] * dim + c] : 0.f;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < K; k++) if (si[k] >= 0 && si[k] != 0x7fffffff) acc = fmaf(wn[k], y[k], acc);
    return fmaf(rate, acc, (1.0f - rate) * x);      // (explicit fmaf: no contraction choice is left to the compiler)
}

// Element `pos` of a sorted register list, `none` past its end: a chain of selects under static indices (a dynamic index would put the list in scratch memory).
template <int K, typename T> __device__ __forceinline__ T knn_pick(const T (&a)[K], int pos, T none)
{
    T v = none;
#pragma unroll
    for (int q = K - 1; q >= 0; q--) v = pos == q ? a[q] : v;
    return v;
}

// The K smallest (distance, index) pairs of a 256-thread workgroup whose threads each hold a sorted list of K (+inf / 0x7fffffff = no entry): per wave by
// K rounds of a minimum over the lanes' heads, then one thread merges the four waves' lists into sd / si (sorted; visible to every thread on return).
template <int K> __device__ __forceinline__ void knn_block_topk(const float (&ld)[K], const int (&li)[K], float (&wd)[4][K], int (&wi)[4][K], float (&sd)[K], int (&si)[K])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int pos = 0;
    for (int k = 0; k < K; k++) {
        float md = knn_pick(ld, pos, INFINITY);
        int mi = knn_pick(li, pos, 0x7fffffff);
        const float d0 = md; const int i0 = mi;
        wave_min_pair(md, mi);
        if (d0 == md && i0 == mi && mi != 0x7fffffff) pos++;
        if (lane == 0) { wd[wave][k] = md; wi[wave][k] = mi; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int ps[4] = {0, 0, 0, 0};
        for (int k = 0; k < K; k++) {
            float md = INFINITY; int mi = 0x7fffffff, mw = 0;
            for (int w = 0; w < 4; w++) if (ps[w] < K) {
                float od = wd[w][ps[w]]; int oi = wi[w][ps[w]];
                if (od < md || (od == md && oi < mi)) { md = od; mi = oi; mw = w; }
            }
            ps[mw]++;
            sd[k] = md; si[k] = mi;
        }
    }
    __syncthreads();
}

#define KNN_MAXQ 16
struct KnnP {
    const float *indexT;     // [dim][n] (or nullptr: the scan walks the row-major index, v_stride = dim, d_stride = 1)
    const float *index;      // [n][dim]
    long long v_stride, d_stride;   // element (vector i, dimension d) of the scanned copy = base[i * v_stride + d * d_stride]
    int n, dim;
    const float *q;          // unique queries, stream stride q_bs
    long long q_bs, cand_bs;
    int nq;
    float *cand_d; int *cand_i;   // [B][nq][nblk][K]
    int nblk;
    const int *overflow;     // when set: run only for streams whose candidate set overflowed (exhaustive fallback)
};

template <int K> __device__ __forceinline__ void knn_scan_body(const KnnP &p)
{
    if (p.overflow && p.overflow[blockIdx.y] == 0) return;
    __shared__ float bd[KNN_MAXQ][4][K];
    __shared__ int bi[KNN_MAXQ][4][K];
    const int b = blockIdx.y;
    // the queries are wave-uniform: read through the scalar cache (s_load) so they cost no LDS/VALU bandwidth
    const float *__restrict__ smem = p.q + (long long)b * p.q_bs;
    const int i = blockIdx.x * 256 + threadIdx.x;
    float acc[KNN_MAXQ];
#pragma unroll
    for (int j = 0; j < KNN_MAXQ; j++) acc[j] = 0.f;
    if (i < p.n) {
        // HBM-streaming loop: 8 independent coalesced loads in flight per thread, then the FMAs in ascending-d order
        // (the distance stays a sequential fmaf chain over d, bit-identical to the reference definition)
        // (transposed copy: coalesced across the threads; without one -- a single stream, where this scan only runs for degenerate
        // data -- every thread streams its own row of the row-major index: same arithmetic, same order, bit-identical distances)
        const float *col = (p.indexT ? p.indexT : p.index) + (long long)i * p.v_stride;
        int d = 0;
        for (; d + 8 <= p.dim; d += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = __builtin_nontemporal_load(col + (long long)(d + u) * p.d_stride);
#pragma unroll
            for (int u = 0; u < 8; u++) {
#pragma unroll
                for (int j = 0; j < KNN_MAXQ; j++) if (j < p.nq) acc[j] = knn_dist_step(acc[j], smem[j * p.dim + d + u], v[u]);
            }
        }
        for (; d < p.dim; d++) {
            float v = col[(long long)d * p.d_stride];
#pragma unroll
            for (int j = 0; j < KNN_MAXQ; j++) if (j < p.nq) acc[j] = knn_dist_step(acc[j], smem[j * p.dim + d], v);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // per query: wave-level top-K by repeated argmin over (distance, index)
    for (int j = 0; j < p.nq; j++) {
        const bool ok = i < p.n && acc[j] < INFINITY;     // (a non-finite distance -- a NaN or an Inf in the query -- is no candidate: the definition's `acc < best` never holds for it, and the other paths report -1)
        float d = ok ? acc[j] : INFINITY; int id = ok ? i : 0x7fffffff;
        for (int k = 0; k < K; k++) {
            float md = d; int mi = id;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                float od = __shfl_xor(md, o, 64); int oi = __shfl_xor(mi, o, 64);
                if (od < md || (od == md && oi < mi)) { md = od; mi = oi; }
            }
            if (lane == 0) { bd[j][wave][k] = md; bi[j][wave][k] = mi; }
            if (id == mi) { d = INFINITY; id = 0x7fffffff; }
        }
    }
    __syncthreads();
    // merge the 4 waves' lists: thread j (< nq) does a tiny selection
    if (threadIdx.x < p.nq) {
        const int j = threadIdx.x;
        int pos[4] = {0, 0, 0, 0};
        for (int k = 0; k < K; k++) {
            float md = INFINITY; int mi = 0x7fffffff, mw = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) if (pos[w] < K) {
                float od = bd[j][w][pos[w]]; int oi = bi[j][w][pos[w]];
                if (od < md || (od == md && oi < mi)) { md = od; mi = oi; mw = w; }
            }
#pragma unroll
            for (int w = 0; w < 4; w++) pos[w] += w == mw ? 1 : 0;
            long long o = (long long)b * p.cand_bs + ((long long)j * p.nblk + blockIdx.x) * K + k;
            p.cand_d[o] = md; p.cand_i[o] = mi;
        }
    }
}
// the entry points: K = 4 under the kernel's own name (profiles and rvc_profile_last_knn know it), K = 8 beside it; the plan's k picks one (retrieval.hip)
static __global__ __launch_bounds__(256) void knn_scan_kernel(KnnP p) { knn_scan_body<KNN_K>(p); }
static __global__ __launch_bounds__(256) void knn_scan_k8_kernel(KnnP p) { knn_scan_body<KNN_KMAX>(p); }

struct KnnBlendP {
    const float *cand_d; const int *cand_i; int nblk, nq;
    const float *index; int dim;
    const float *q;        // unique queries [B][nq][dim]
    int skip_head, T, R, first_raw;   // sliced frame r uses unique query min((skip_head+r)/2, T-1) - first_raw
    float rate;
    float *phone; int ph_cs; long long ph_bs;
    int *out_idx; float *out_dist;   // [B][R][K]
    const int *overflow;
};

// one workgroup per (unique query, stream): merge candidates, then blend every sliced frame that maps to it
template <int K> __device__ __forceinline__ void knn_merge_blend_body(const KnnBlendP &p)
{
    __shared__ float sd[K]; __shared__ int si[K];
    __shared__ float wd[4][K]; __shared__ int wi[4][K];
    const int j = blockIdx.x, b = blockIdx.y;
    if (p.overflow && p.overflow[b] == 0) return;
    const long long base = ((long long)b * p.nq + j) * p.nblk * K;
    const int total = p.nblk * K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // each thread keeps a sorted local top-K of its strided candidates (sorted insert by (distance, index) under static indices: the lists stay in registers)
    float ld[K]; int li[K];
#pragma unroll
    for (int k = 0; k < K; k++) { ld[k] = INFINITY; li[k] = 0x7fffffff; }
    for (int c = threadIdx.x; c < total; c += 256) {
        float cd = p.cand_d[base + c]; int ci = p.cand_i[base + c];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const bool sw = cd < ld[k] || (cd == ld[k] && ci < li[k]);
            const float t0 = sw ? ld[k] : cd; const int t1 = sw ? li[k] : ci;
            ld[k] = sw ? cd : ld[k]; li[k] = sw ? ci : li[k];
            cd = t0; ci = t1;
        }
    }
    knn_block_topk(ld, li, wd, wi, sd, si);
    float w[K];
    knn_blend_weights(sd, w);
    const float *qv = p.q + ((long long)b * p.nq + j) * p.dim;
    for (int r = 0; r < p.R; r++) {
        int s = (p.skip_head + r) / 2; s = s < p.T - 1 ? s : p.T - 1;
        if (s - p.first_raw != j) continue;
        if (threadIdx.x < K) {
            p.out_idx[((long long)b * p.R + r) * K + threadIdx.x] = si[threadIdx.x] == 0x7fffffff ? -1 : si[threadIdx.x];
            p.out_dist[((long long)b * p.R + r) * K + threadIdx.x] = sd[threadIdx.x];
        }
        for (int c = threadIdx.x; c < p.dim; c += 256)
            p.phone[(long long)b * p.ph_bs + (long long)c * p.ph_cs + r] = knn_blend_channel(p.index, p.dim, c, si, w, p.rate, qv[c]);
    }
}
// the entry points: K = 4 under the kernel's own name (profiles and rvc_profile_last_knn know it), K = 8 beside it; the plan's k picks one (retrieval.hip)
static __global__ __launch_bounds__(256) void knn_merge_blend_kernel(KnnBlendP p) { knn_merge_blend_body<KNN_K>(p); }
static __global__ __launch_bounds__(256) void knn_merge_blend_k8_kernel(KnnBlendP p) { knn_merge_blend_body<KNN_KMAX>(p); }

// ---- HBM-roofline retrieval: approximate distances on the matrix cores, exact re-rank of a provably sufficient candidate set ----
// Stage A for one stream / few streams lives in knn_scan_select_kernel (below); with many streams it is one implicit GEMM (retrieval.hip).
// compare-exchange of two (distance, index) pairs, ascending, ties by index (deterministic)
__device__ __forceinline__ void knn_cx(float &d0, int &i0, float &d1, int &i1)
{
    const bool sw = d1 < d0 || (d1 == d0 && i1 < i0);
    const float td = sw ? d1 : d0, ud = sw ? d0 : d1; const int ti = sw ? i1 : i0, ui = sw ? i0 : i1;
    d0 = td; i0 = ti; d1 = ud; i1 = ui;
}
// bitonic clean-up of N = 4 or 8 pairs in registers (a bitonic sequence in, ascending out): strides N/2 .. 1
template <int N> __device__ __forceinline__ void knn_bitonic_clean(float (&d)[N], int (&i)[N])
{
#pragma unroll
    for (int st = N / 2; st >= 1; st >>= 1) {
#pragma unroll
        for (int a = 0; a < N; a++) if ((a & st) == 0) knn_cx(d[a], i[a], d[a + st], i[a + st]);
    }
}
// the N smallest of two ascending lists of N, ascending, into a: min(a[r], b[N - 1 - r]) by (distance, index) is bitonic, then the clean-up
template <int N> __device__ __forceinline__ void knn_merge_low(float (&ad)[N], int (&ai)[N], const float (&bd)[N], const int (&bi)[N])
{
#pragma unroll
    for (int r = 0; r < N; r++) {
        const bool tk = bd[N - 1 - r] < ad[r] || (bd[N - 1 - r] == ad[r] && bi[N - 1 - r] < ai[r]);
        ad[r] = tk ? bd[N - 1 - r] : ad[r]; ai[r] = tk ? bi[N - 1 - r] : ai[r];
    }
    knn_bitonic_clean(ad, ai);
}
// One stream / few streams: the WHOLE retrieval as one launch (round 4; before: knn_queries + knn_dot + knn_select_blend + two idle
// fallback launches = 116 us of kernels for a 307 MB scan).
//  * scan: a workgroup owns tiles of 16 consecutive index vectors (a contiguous 16*dim*4-byte block of HBM in MFMA-fragment order, read
//    exactly once; tiles blockIdx.x, + gridDim.x, ...) against up to 16 queries; its four waves split the K range of every tile (dot
//    products on v_mfma_f32_16x16x4_f32, each wave streams its 12 KB of the tile with the NEXT tile's fragments requested as the slots
//    free up), the partial 16 x 16 tiles meet in LDS and one wave (in turn) forms approx = |y|^2 - 2 x.y and keeps a running top-K per
//    query.  Splitting K instead of handing whole tiles to waves makes the unit of work a quarter as long: 6 250 tiles over 768
//    workgroups is 8 or 9 each, where 3 072 waves had 2 or 3 (the last third of the launch ran at 3 % occupancy).  The queries are
//    gathered straight from the ContentVec output; NO approximate distance is written: the workgroup publishes K {distance, index}
//    granules per query (agent-scope stores, no cache maintenance), then takes a ticket;
//  * select: the last S = min(queries, workgroups) arrivals stay, wait until every list of their stream is published and each runs
//    stages 1-4 of knn_select_blend_kernel for its query: the global top-K of the approximations is in the union of the workgroups'
//    lists; a workgroup whose K-th entry is inside the margin may hide a (K + 1)-th candidate ("flagged"): ALL of its vectors become candidates,
//    so no approximation array and no second pass exist, and nothing can overflow (a degenerate index costs exact distances for the
//    flagged workgroups' vectors, 8 per round).  Same candidate superset, same exact re-rank, same hits as the three-launch form.
struct KnnFusedP {
    const float *indexF, *index, *ynorm; int n, dim;
    const float *cv; int cv_cs; long long cv_bs; int first_raw, nq, q0;
    unsigned long long *lists;         // [B][16][gridDim.x][K] granules: low word = distance bits, high word = index
    unsigned *ticket;                  // [B][2]: arrivals, selectors done; zero between launches
    unsigned spin_limit;               // polls of the arrival counter before a selector gives up (ST_KNN_TIMEOUT)
    int test_lose;                     // test hook RVC_KNN_LOSE_TICKET: workgroup 0 of every stream never takes its ticket (a hand-off that cannot complete)
    int skip_head, T, R; float rate;
    float *phone; int ph_cs; long long ph_bs;
    int *out_idx; float *out_dist;
    int *status; int status_stride;
#ifdef RVC_KNN_STAMPS
    long long *stamps;                 // tests/tools/knn_probe.hip: [gridDim.x][16] wall-clock stamps of thread 0
#endif
};
#ifdef RVC_KNN_STAMPS
#define KNN_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.y == 0) p.stamps[blockIdx.x * 16 + (i)] = (long long)wall_clock64(); } while (0)
#else
#define KNN_STAMP(i) do { } while (0)
#endif
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));      // a 16-byte global load from a dword-aligned address
// minimum over the 64 lanes without LDS-crossbar shuffles: four DPP row rotations (every lane then holds its 16-lane row's minimum), the four
// rows' values through v_readlane.  No NaN may come in.
__device__ __forceinline__ float wave_min_dpp(float v)
{
    v = fminf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false)));      // row_ror:1
    v = fminf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false)));      // row_ror:2
    v = fminf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false)));      // row_ror:4
    v = fminf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false)));      // row_ror:8
    const int iv = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 48));
    return fminf(fminf(r0, r1), fminf(r2, r3));
}
#define KNN_FUSED_MAXG 1024            // workgroups per stream (a selector thread looks at 4 workgroup lists: all in registers at K = 4, two at a time at K = 8)
// Candidate rows staged per round of the exact re-rank.  <= 16 for every K: thread r < KNN_FUSED_ROWS keeps the sorted K smallest of the rows IT walked, so the
// final K are in the union of those lists, and the K rounds of a minimum that extract them exchange over xor 8 .. 1, i.e. among lanes 0..15.  K does not enter:
// a deeper list costs registers in those lanes (2 K), not lanes.
#define KNN_FUSED_ROWS 10
// dynamic LDS, in floats: scan = query rows + two buffers of partial tiles; select = query row + candidate ids (<= K - 1 per unflagged workgroup) + staged rows
__host__ __device__ inline size_t knn_fused_lds_floats(int dim, int nqg, int G, int K)
{
    const size_t QS = (size_t)dim + 4, scan = (size_t)nqg * QS + 2 * 4 * 256, sel = QS + (((size_t)(K - 1) * G + 3) & ~(size_t)3) + (size_t)KNN_FUSED_ROWS * QS;
    return scan > sel ? scan : sel;
}
template <int K> __device__ __forceinline__ void knn_scan_select_body(const KnnFusedP &p)
{
    constexpr int D = 12;
    extern __shared__ __attribute__((aligned(16))) float s_q[];
    __shared__ float wl_d[4][16][K]; __shared__ int wl_i[4][16][K];
    __shared__ __attribute__((aligned(16))) float wd[4][K];
    __shared__ float sd[K]; __shared__ int si[K];
    __shared__ float s_red[4];
    __shared__ int s_role, s_cnt, s_dead;
    __shared__ unsigned s_flag[KNN_FUSED_MAXG / 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, G = gridDim.x;
    const int QS = p.dim + 4, nc = p.dim >> 4;
    const int li = lane & 15, kq = lane >> 4;
    const int nqg = p.nq - p.q0 < 16 ? p.nq - p.q0 : 16;
    const int F0 = wave * nc / 4, F = (wave + 1) * nc / 4 - F0;          // this wave's fragments of every tile
    const long long ntile = ((long long)p.n + 15) >> 4;
    long long t = blockIdx.x;
    KNN_STAMP(0);
    // the first tile's fragments are requested before the queries are gathered
    f32x4 a_st[D];
    {
        const float *ar = p.indexF + (t * nc + F0) * 256 + lane * 4;
#pragma unroll
        for (int s = 0; s < D; s++)
            if (s < F && t < ntile) a_st[s] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(ar + s * 256));
    }
    // queries: s_q[r][c] = cv[c][first_raw + q0 + r], r < nqg.  A lane takes 4 consecutive queries of one channel -- one dword-aligned
    // 16-byte load where all four exist --, 16 channels per wave instruction; LDS writes conflict-free
    const float *cvb = p.cv + (long long)b * p.cv_bs + p.first_raw;
    {
        const int r0 = (lane & 3) * 4;
        const bool whole = r0 + 3 < nqg;
        for (int c = (tid >> 2); c < p.dim; c += 64) {
            const float *src = cvb + (long long)c * p.cv_cs + p.q0;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (whole) v = *reinterpret_cast<const f32x4u *>(src + r0);
            else {
#pragma unroll
                for (int i = 0; i < 4; i++) if (r0 + i < nqg) v[i] = src[r0 + i];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) if (r0 + i < nqg) s_q[(r0 + i) * QS + c] = v[i];
        }
    }
    float *part = s_q + (size_t)nqg * QS;                                 // [2][4 waves][64 lanes][4]
    __syncthreads();
    KNN_STAMP(1);
    float rd[K]; int ri[K];
#pragma unroll
    for (int k = 0; k < K; k++) { rd[k] = INFINITY; ri[k] = 0x7fffffff; }
    // (query columns past the last query of the group repeat it: their results are never read)
    const float *br = s_q + (li < nqg ? li : nqg - 1) * QS + kq * 4;
    for (int it = 0; t < ntile; t += G, it++) {
        const float *ar = p.indexF + (t * nc + F0) * 256 + lane * 4;
        const bool more = t + G < ntile;
        const float *an = p.indexF + ((t + G) * nc + F0) * 256 + lane * 4;
        const int ew = it & 3;                                            // the wave that ranks this tile
        const long long i0 = t * 16;
        // |y|^2 of the lane's four vectors: requested now, consumed behind the dot products
        float yn[4] = {0.f, 0.f, 0.f, 0.f};
        if (wave == ew) {
#pragma unroll
            for (int r = 0; r < 4; r++) { const long long v = i0 + kq * 4 + r; yn[r] = v < p.n ? p.ynorm[v] : 0.f; }
        }
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < F; c += D) {
#pragma unroll
            for (int s = 0; s < D; s++) {
                if (c + s < F) {
                    const f32x4 bq = *reinterpret_cast<const f32x4 *>(br + (F0 + c + s) * 16);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_st[s][0], bq[0], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_st[s][1], bq[1], acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_st[s][2], bq[2], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_st[s][3], bq[3], acc1, 0, 0, 0);
                    // the wave's fragment stream continues into the workgroup's next tile: after its last use in this tile, slot s takes fragment s of the next
                    if (c + s + D < F) a_st[s] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(ar + (c + s + D) * 256));
                    else if (more) a_st[s] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(an + s * 256));
                }
            }
        }
        float *pb = part + (it & 1) * 1024;
        {
            f32x4 a01;
#pragma unroll
            for (int r = 0; r < 4; r++) a01[r] = acc0[r] + acc1[r];
            *reinterpret_cast<f32x4 *>(pb + wave * 256 + lane * 4) = a01;
        }
        __syncthreads();        // (one barrier per tile: buffer it & 1 is rewritten two tiles later, behind the next barrier, which the ranking wave reaches after reading it)
        if (wave == ew) {
            // D layout: row (index vector) = (lane >> 4) * 4 + r, column (query) = lane & 15; partial tiles summed in wave order
            const f32x4 p0 = *reinterpret_cast<const f32x4 *>(pb + lane * 4), p1 = *reinterpret_cast<const f32x4 *>(pb + 256 + lane * 4);
            const f32x4 p2 = *reinterpret_cast<const f32x4 *>(pb + 512 + lane * 4), p3 = *reinterpret_cast<const f32x4 *>(pb + 768 + lane * 4);
            float vd[4]; int vi[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const long long v = i0 + kq * 4 + r;
                const float a = yn[r] - 2.0f * (((p0[r] + p1[r]) + p2[r]) + p3[r]);
                vd[r] = (v < p.n && a == a) ? a : INFINITY;            // (a NaN never is a candidate; as +inf it cannot upset the sorting networks either)
                vi[r] = v < p.n ? (int)v : 0x7fffffff;
            }
            // the lane's 4 sorted; the column's other 12 rows are in lanes ^ 16, ^ 32
            knn_cx(vd[0], vi[0], vd[1], vi[1]); knn_cx(vd[2], vi[2], vd[3], vi[3]); knn_cx(vd[0], vi[0], vd[2], vi[2]);
            knn_cx(vd[1], vi[1], vd[3], vi[3]); knn_cx(vd[1], vi[1], vd[2], vi[2]);
            if constexpr (K == 4) {
                // the tile's 4 smallest per query column: two bitonic merges with the lanes holding the column's other rows
#pragma unroll
                for (int o = 16; o <= 32; o <<= 1) {
                    float od[4]; int oi[4];
#pragma unroll
                    for (int r = 0; r < 4; r++) { od[r] = __shfl_xor(vd[r], o, 64); oi[r] = __shfl_xor(vi[r], o, 64); }
                    knn_merge_low(vd, vi, od, oi);
                }
                // ... merged into the wave's running list (both sorted: min(a[k], b[3 - k]) keeps the 4 smallest, then the bitonic clean-up)
                knn_merge_low(rd, ri, vd, vi);
            } else {
                // the tile's 8 smallest per query column: the lane's 4 ascending and lane ^ 16's 4 descending are a bitonic 8 (all of the pair's rows: nothing
                // is dropped yet), sorted by the clean-up in both lanes of the pair; one merge with lane ^ 32's sorted 8 keeps the 8 smallest of the 16
                float ed[8]; int ei[8];
#pragma unroll
                for (int r = 0; r < 4; r++) { ed[r] = vd[r]; ei[r] = vi[r]; ed[4 + r] = __shfl_xor(vd[3 - r], 16, 64); ei[4 + r] = __shfl_xor(vi[3 - r], 16, 64); }
                knn_bitonic_clean(ed, ei);
                float od[8]; int oi[8];
#pragma unroll
                for (int r = 0; r < 8; r++) { od[r] = __shfl_xor(ed[r], 32, 64); oi[r] = __shfl_xor(ei[r], 32, 64); }
                knn_merge_low(ed, ei, od, oi);
                // ... merged into the wave's running list
                knn_merge_low(rd, ri, ed, ei);
            }
        }
    }
    if (kq == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) { wl_d[wave][li][k] = rd[k]; wl_i[wave][li][k] = ri[k]; }
    }
    __syncthreads();
    KNN_STAMP(2);
    // the workgroup's list per query: merge of its four waves' lists, published as K granules; then the ticket (same wave: program order)
    if (tid < 16) {
        int pos[4] = {0, 0, 0, 0};
        unsigned long long *out = p.lists + (((long long)b * 16 + tid) * G + blockIdx.x) * K;
#pragma unroll
        for (int k = 0; k < K; k++) {
            float md = INFINITY; int mi = 0x7fffffff, mw = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int pw = pos[w] < K ? pos[w] : K - 1;
                const float od = wl_d[w][tid][pw]; const int oi = wl_i[w][tid][pw];
                if (pos[w] < K && (od < md || (od == md && oi < mi))) { md = od; mi = oi; mw = w; }
            }
#pragma unroll
            for (int w = 0; w < 4; w++) pos[w] += (w == mw && mi != 0x7fffffff) ? 1 : 0;
            __hip_atomic_store(out + k, ((unsigned long long)(unsigned)mi << 32) | (unsigned long long)__float_as_uint(md), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (wave == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the granules have left (write-through) before the ticket is taken
        // release: the granule stores above are ordered before the ticket; the selectors' acquire load below pairs with it
        if (tid == 0) s_role = (p.test_lose && blockIdx.x == 0) ? 0 : (int)__hip_atomic_fetch_add(p.ticket + b * 2, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    KNN_STAMP(3);
    const int S = nqg < G ? nqg : G;
    if (s_role >= 0 && s_role < G - S) return;
    // A role outside [0, G): the counters were left behind by a launch that timed out (they are NOT re-armed on that path, so every later launch on
    // them fails fast here instead of assigning selector roles from stale counts).  The host re-arms them (engine.hip recover_retrieval / plan rebuild).
    const bool stale = s_role < 0 || s_role >= G;
    const int sel = stale ? 0 : s_role - (G - S);
    if (tid == 0) {
        unsigned spins = 0; int dead = stale ? 1 : 0;
        while (!dead && __hip_atomic_load(p.ticket + b * 2, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)G) {
            if (++spins > p.spin_limit) { dead = 1; break; }
            __builtin_amdgcn_s_sleep(2);
        }
        if (dead) {
            atomicOr(&p.status[b * p.status_stride], (int)ST_KNN_TIMEOUT);
            // poison the arrival counter: whatever is launched on it before the host has re-armed it sees a role beyond G and stops here
            __hip_atomic_store(p.ticket + b * 2, 0x40000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        s_dead = dead;
    }
    __syncthreads();
    KNN_STAMP(4);
    // select-phase layout of the dynamic LDS: query row | candidate ids (<= K - 1 per unflagged workgroup) | KNN_FUSED_ROWS staged rows
    float *s_x = s_q;
    int *cand = reinterpret_cast<int *>(s_q + QS);
    float *s_rows = s_q + QS + (((K - 1) * G + 3) & ~3);
    // A selector thread looks at the lists of workgroups tid + 256 u, u < 4.  K = 4: all four in registers, loaded once.  K = 8: four lists are 64 granules
    // (128 registers, live from the loads to the candidate collection, on top of the re-rank's 64): two rounds of two lists, fetched again (from the L2) for the
    // collection, keep the kernel at the K = 4 register budget and out of scratch
    constexpr int LPR = K == 4 ? 4 : 2, NLR = 4 / LPR;
    const int nv = p.dim >> 2;
    for (int jq = sel; jq < nqg && !s_dead; jq += S) {
        const int j = p.q0 + jq;
        __syncthreads();
        // the query (exact arithmetic below reads it from LDS) and |x|^2 (only scales the error margin): still in the scan's LDS rows for
        // the selector's first query, gathered again for further ones (the select-phase layout has overwritten them)
        float xn = 0.f;
        if (jq == sel) {
            for (int c = tid; c < p.dim; c += 256) { const float v = s_q[jq * QS + c]; if (jq) s_x[c] = v; xn += v * v; }     // (row jq -> row 0: disjoint)
        } else {
            for (int c = tid; c < p.dim; c += 256) { const float v = cvb[(long long)c * p.cv_cs + j]; s_x[c] = v; xn += v * v; }
        }
        xn = wave_sum(xn);
        if (lane == 0) s_red[wave] = xn;
        if (tid < KNN_FUSED_MAXG / 32) s_flag[tid] = 0u;
        if (tid == 0) s_cnt = 0;
        // this thread's workgroup lists: w = tid + 256 * (lr * LPR + u)
        float ld_[LPR][K]; int li_[LPR][K];
        const unsigned long long *lq = p.lists + ((long long)b * 16 + jq) * G * K;
        auto load_lists = [&](int lr) {
            unsigned long long x[LPR][K];
#pragma unroll
            for (int u = 0; u < LPR; u++) {
                const int w = tid + 256 * (lr * LPR + u);
#pragma unroll
                for (int k = 0; k < K; k++) {
                    x[u][k] = 0x7fffffff7f800000ull;      // {+inf, no index}
                    if (w < G) x[u][k] = __hip_atomic_load(lq + (long long)w * K + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
#pragma unroll
            for (int u = 0; u < LPR; u++) {
#pragma unroll
                for (int k = 0; k < K; k++) { ld_[u][k] = __uint_as_float((unsigned)x[u][k]); li_[u][k] = (int)(unsigned)(x[u][k] >> 32); }
            }
        };
        // 1. the K-th smallest approximate distance: per-thread sorted top-K (static indices only), wave extraction, 4-way merge
        float td[K];
#pragma unroll
        for (int k = 0; k < K; k++) td[k] = INFINITY;
#pragma unroll
        for (int lr = 0; lr < NLR; lr++) {
            if (NLR > 1 && lr * LPR * 256 >= G) break;
            load_lists(lr);
#ifdef RVC_KNN_STAMPS
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            KNN_STAMP(12);
#endif
#pragma unroll
            for (int u = 0; u < LPR; u++) {
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const float d = ld_[u][k];
                    if (d < td[K - 1]) {
#pragma unroll
                        for (int q = K - 1; q >= 1; q--) {
                            const bool left = d < td[q - 1], here = !left && d < td[q];
                            td[q] = left ? td[q - 1] : (here ? d : td[q]);
                        }
                        if (d < td[0]) td[0] = d;
                    }
                }
            }
        }
        {
            // the wave's K smallest, with multiplicity: the minimum of the lanes' heads, the lowest lane holding it moves on
            int pos = 0;
            for (int k = 0; k < K; k++) {
                const float d0 = knn_pick(td, pos, INFINITY);
                const float md = wave_min_dpp(d0);
                const unsigned long long holders = __ballot(d0 == md && md < INFINITY);
                if (holders && lane == __ffsll((long long)holders) - 1) pos++;
                if (lane == 0) wd[wave][k] = md;
            }
        }
        KNN_STAMP(13);
        __syncthreads();
        // (every thread merges the four waves' lists itself: 4 K broadcast reads instead of a one-thread merge between two barriers)
        float aK;
        {
            float mK[K];
#pragma unroll
            for (int k = 0; k < K; k++) mK[k] = INFINITY;
#pragma unroll
            for (int w = 0; w < 4; w++) {
#pragma unroll
                for (int k4 = 0; k4 < K; k4 += 4) {
                    const f32x4 wv = *reinterpret_cast<const f32x4 *>(&wd[w][k4]);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const float d = wv[k];
                        if (d < mK[K - 1]) {
#pragma unroll
                            for (int q = K - 1; q >= 1; q--) {
                                const bool left = d < mK[q - 1], here = !left && d < mK[q];
                                mK[q] = left ? mK[q - 1] : (here ? d : mK[q]);
                            }
                            if (d < mK[0]) mK[0] = d;
                        }
                    }
                }
            }
            aK = mK[K - 1];
        }
        KNN_STAMP(5);
        // 2. candidates within the error margin of the approximate K-th distance (bound and margin as in knn_select_blend_kernel)
        const float s_xn = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
        const float margin = 2e-3f * (fabsf(aK + s_xn) + s_xn + 1e-3f);
        const float thr = aK + margin;
#pragma unroll
        for (int lr = 0; lr < NLR; lr++) {
            if (NLR > 1 && lr * LPR * 256 >= G) break;
            if constexpr (NLR > 1) load_lists(lr);
#pragma unroll
            for (int u = 0; u < LPR; u++) {
                const int w = tid + 256 * (lr * LPR + u);
                if (w < G) {
                    if (ld_[u][K - 1] <= thr) atomicOr(&s_flag[w >> 5], 1u << (w & 31));     // may hide a (K + 1)-th candidate: expanded below
                    else {
#pragma unroll
                        for (int k = 0; k < K - 1; k++) if (ld_[u][k] <= thr) cand[atomicAdd(&s_cnt, 1)] = li_[u][k];
                    }
                }
            }
        }
        __syncthreads();
        // 3. exact distances in the reference's order (ascending-d sequential fmaf).  The rows are fetched with coalesced 16-byte loads
        //    and staged in LDS as DIFFERENCES x - y (every thread subtracts what it fetched), so that the one thread per row that walks
        //    the chain issues a single dependent fmaf per dimension; thread r < KNN_FUSED_ROWS keeps a sorted top-K of what it has seen
        float bd[K]; int bi[K];
#pragma unroll
        for (int k = 0; k < K; k++) { bd[k] = INFINITY; bi[k] = 0x7fffffff; }
        auto round = [&](auto row_of, int nrows) {
            __syncthreads();
            for (int i = tid; i < nrows * nv; i += 256) {
                const int r = i / nv, c4 = i - r * nv;
                const f32x4 y = *reinterpret_cast<const f32x4 *>(p.index + (long long)row_of(r) * p.dim + c4 * 4);
                *reinterpret_cast<f32x4 *>(s_rows + r * QS + c4 * 4) = *reinterpret_cast<const f32x4 *>(s_x + c4 * 4) - y;
            }
            __syncthreads();
            KNN_STAMP(11);
            if (tid < nrows) {
                const float *v = s_rows + tid * QS;
                float acc = 0.f;
#ifdef RVC_KNN_STAMPS
                const long long cyc0 = clock64();
#endif
                // two register sets of 32 differences each: one is consumed while the other is on its way from LDS.  Dimensions that are a
                // multiple of 64 (768, 256) take the loop without per-group guards (the guards compile to a select and five scalar
                // instructions per four dimensions, in the middle of the dependent chain)
                f32x4 ra[8], rb[8];
                if ((p.dim & 63) == 0) {
#pragma unroll
                    for (int u = 0; u < 8; u++) ra[u] = *reinterpret_cast<const f32x4 *>(v + 4 * u);
                    for (int d = 0; d < p.dim; d += 64) {
#pragma unroll
                        for (int u = 0; u < 8; u++) rb[u] = *reinterpret_cast<const f32x4 *>(v + d + 32 + 4 * u);
#pragma unroll
                        for (int u = 0; u < 8; u++) {
#pragma unroll
                            for (int i = 0; i < 4; i++) acc = fmaf(ra[u][i], ra[u][i], acc);
                        }
                        if (d + 64 < p.dim) {
#pragma unroll
                            for (int u = 0; u < 8; u++) ra[u] = *reinterpret_cast<const f32x4 *>(v + d + 64 + 4 * u);
                        }
#pragma unroll
                        for (int u = 0; u < 8; u++) {
#pragma unroll
                            for (int i = 0; i < 4; i++) acc = fmaf(rb[u][i], rb[u][i], acc);
                        }
                    }
                } else {
                    auto fetch = [&](f32x4 (&r)[8], int d) {
#pragma unroll
                        for (int u = 0; u < 8; u++) r[u] = *reinterpret_cast<const f32x4 *>(v + (d + 4 * u < p.dim ? d + 4 * u : 0));
                    };
                    auto chain = [&](const f32x4 (&r)[8], int d) {
#pragma unroll
                        for (int u = 0; u < 8; u++) {
                            if (d + 4 * u < p.dim) {
#pragma unroll
                                for (int i = 0; i < 4; i++) acc = fmaf(r[u][i], r[u][i], acc);
                            }
                        }
                    };
                    fetch(ra, 0);
                    for (int d = 0; d < p.dim; d += 64) {
                        fetch(rb, d + 32);
                        chain(ra, d);
                        fetch(ra, d + 64);
                        chain(rb, d + 32);
                    }
                }
#ifdef RVC_KNN_STAMPS
                if (tid == 0 && blockIdx.y == 0) p.stamps[blockIdx.x * 16 + 1] = clock64() - cyc0 + (acc == 1.2345f ? 1 : 0);
#endif
                float cd = acc; int ci = row_of(tid);
                // sorted insert by (distance, index); a NaN distance never enters
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const bool sw = cd < bd[k] || (cd == bd[k] && ci < bi[k]);
                    const float t0 = sw ? bd[k] : cd; const int t1 = sw ? bi[k] : ci;
                    bd[k] = sw ? cd : bd[k]; bi[k] = sw ? ci : bi[k];
                    cd = t0; ci = t1;
                }
            }
        };
        const int ncand = s_cnt;
        KNN_STAMP(10);
        for (int base = 0; base < ncand; base += KNN_FUSED_ROWS) {
            const int nr = ncand - base < KNN_FUSED_ROWS ? ncand - base : KNN_FUSED_ROWS;
            round([&](int r) { return cand[base + r]; }, nr);
        }
        for (int fw = 0; fw < (G + 31) / 32; fw++) {
            unsigned m = s_flag[fw];
            while (m) {
                const int w = fw * 32 + __builtin_ctz(m); m &= m - 1;
                // every vector the flagged workgroup scanned: tiles w, w + G, ...
                for (long long t0 = (long long)w * 16; t0 < p.n; t0 += (long long)G * 16) {
                    const int nt = p.n - t0 < 16 ? (int)(p.n - t0) : 16;
                    for (int base = 0; base < nt; base += KNN_FUSED_ROWS) {
                        const int nr = nt - base < KNN_FUSED_ROWS ? nt - base : KNN_FUSED_ROWS;
                        round([&](int r) { return (int)t0 + base + r; }, nr);
                    }
                }
            }
        }
        KNN_STAMP(6);
        // the final K: wave 0 holds every list (threads < KNN_FUSED_ROWS); K rounds of a minimum by (distance, index) over those lanes
        if (wave == 0) {
            int pos = 0;
            for (int k = 0; k < K; k++) {
                float md = knn_pick(bd, pos, INFINITY);
                int mi = knn_pick(bi, pos, 0x7fffffff);
                int ml = lane;
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    const float od = __shfl_xor(md, o, 64); const int oi = __shfl_xor(mi, o, 64), ol = __shfl_xor(ml, o, 64);
                    if (oi != 0x7fffffff && (mi == 0x7fffffff || od < md || (od == md && oi < mi))) { md = od; mi = oi; ml = ol; }
                }
                if (ml == lane && mi != 0x7fffffff) pos++;
                if (lane == 0) { sd[k] = mi == 0x7fffffff ? INFINITY : md; si[k] = mi; }
            }
        }
        __syncthreads();
        KNN_STAMP(8);
        // 4. blend: w = (1/d)^2 normalised, feat = rate * sum w_i y_i + (1 - rate) * feat; computed once per
        //    query, written to every sliced frame that duplicates it (a contiguous range of r: frames (skip_head + r) / 2, clamped to T - 1)
        float wn[K];
        knn_blend_weights(sd, wn);
        const int raw = j + p.first_raw;
        int r_lo = 2 * raw - p.skip_head, r_hi = raw >= p.T - 1 ? p.R : 2 * raw + 2 - p.skip_head;
        r_lo = r_lo < 0 ? 0 : r_lo; r_hi = r_hi > p.R ? p.R : r_hi;
        float *ph = p.phone + (long long)b * p.ph_bs;
        for (int c = tid; c < p.dim; c += 256) {
            const float val = knn_blend_channel(p.index, p.dim, c, si, wn, p.rate, s_x[c]);
            for (int r = r_lo; r < r_hi; r++) ph[(long long)c * p.ph_cs + r] = val;
        }
        KNN_STAMP(9);
        if (tid < K)
            for (int r = r_lo; r < r_hi; r++) {
                p.out_idx[((long long)b * p.R + r) * K + tid] = si[tid] == 0x7fffffff ? -1 : si[tid];   // -1: no hit (non-finite query)
                p.out_dist[((long long)b * p.R + r) * K + tid] = sd[tid];
            }
    }
    __syncthreads();
    KNN_STAMP(7);
    // the last selector to leave re-arms the counters for the next launch (never after a time-out: a late workgroup may still take a ticket)
    if (tid == 0 && !s_dead) {
        const unsigned d = __hip_atomic_fetch_add(p.ticket + b * 2 + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((int)d == S - 1) {
            __hip_atomic_store(p.ticket + b * 2 + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p.ticket + b * 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
// the entry points: K = 4 under the kernel's own name (profiles and rvc_profile_last_knn know it), K = 8 beside it; the plan's k picks one (retrieval.hip)
static __global__ __launch_bounds__(256) void knn_scan_select_kernel(KnnFusedP p) { knn_scan_select_body<KNN_K>(p); }
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void knn_scan_select_k8_kernel(KnnFusedP p) { knn_scan_select_body<KNN_KMAX>(p); }

// |y_i|^2 for every index vector (load time); nhn = -|y_i|^2 / 2 is the per-column "residual" of the many-stream distance GEMM
static __global__ void knn_norms_kernel(const float *index, int n, int dim, float *ynorm, float *nhn)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = index + (long long)i * dim;
    float s = 0.f;
    for (int d = 0; d < dim; d++) s = fmaf(r[d], r[d], s);
    ynorm[i] = s;
    nhn[i] = -0.5f * s;
}

// Load-time repack of the index on the device (the matrix arrives in HBM by upload or by the RCCL broadcast and never goes back to
// the host): [n][dim] -> MFMA-fragment order [tile of 16 vectors][chunk of 16 dims][lane][4] for knn_scan_select_kernel (vectors past n zero).
// One thread per float4 of the output; reads are 16-byte pieces of 16 neighbouring rows.
static __global__ __launch_bounds__(256) void knn_pack_index_kernel(const float *index, long long n, int dim, float *indexF, long long total4)
{
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total4) return;
    const int nc = dim / 16;
    const int l = (int)(o & 63);
    const long long tc = o >> 6, tl = tc / nc;
    const int c = (int)(tc - tl * nc);
    const long long v = tl * 16 + (l & 15);
    f32x4 val = {0.f, 0.f, 0.f, 0.f};
    if (v < n) val = *reinterpret_cast<const f32x4 *>(index + v * dim + c * 16 + (l >> 4) * 4);
    *reinterpret_cast<f32x4 *>(indexF + o * 4) = val;
}
// [n][dim] -> [dim][n] through a 32 x 33 LDS tile (only plans that need the transposed copy build it: the many-stream distance GEMM
// and the forced exhaustive scan)
static __global__ __launch_bounds__(256) void knn_transpose_kernel(const float *index, long long n, int dim, float *indexT)
{
    __shared__ float tile[32][33];
    const long long v0 = (long long)blockIdx.x * 32; const int d0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) { const long long v = v0 + r; const int d = d0 + tx; tile[r][tx] = (v < n && d < dim) ? index[v * dim + d] : 0.f; }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) { const int d = d0 + r; const long long v = v0 + tx; if (d < dim && v < n) indexT[(long long)d * n + v] = tile[tx][r]; }
}

// Many streams: the queries of all streams as the WEIGHT operand of one implicit GEMM against the transposed index (approx[q][i] =
// |y_i|^2 - 2 x_q . y_i for every stream's queries in ONE pass over the index instead of one pass per 16 queries): [Q][dim] ->
// MFMA-fragment order [tile of 16 queries][chunk of 16 dims][lane][4], rows past Q zero.  grid = (Qpad / 16, dim / 16), 64 threads.
static __global__ __launch_bounds__(64) void knn_pack_queries_kernel(const float *q, int Q, int dim, float *qf)
{
    const int t = blockIdx.x, c = blockIdx.y, l = threadIdx.x, v = t * 16 + (l & 15);
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (v < Q) x = *reinterpret_cast<const f32x4 *>(q + (long long)v * dim + c * 16 + (l >> 4) * 4);
    *reinterpret_cast<f32x4 *>(qf + (((long long)t * gridDim.y + c) * 64 + l) * 4) = x;
}

// Stage B (knn_select_blend_kernel): one workgroup per (unique query, stream).
//  1. exact top-K of the APPROXIMATE distances -> K-th smallest a_K (K = 4 or 8: the plan's k);
//  2. candidate set = { i : approx_i <= a_K + margin }: since |approx - true| <= err < margin/2, every vector of the true top-K
//     (true distance <= true K-th distance <= a_K + err) is in the set;
//  3. exact sequential-fmaf distances (the reference definition) for the candidates, final order by (distance, index);
//  4. w = (1/d)^2 blend of the duplicated frames (as before).
// More than KNN_CAND candidates (degenerate data, e.g. thousands of duplicate vectors): overflow[b] is raised and the
// exhaustive exact scan (knn_scan_kernel + knn_merge_blend_kernel) recomputes this stream.
#define KNN_CAND 512
struct KnnSelP {
    const float *approx; long long approx_bs; int n, dim, nq;
    const float *index; const float *q; long long q_bs;
    int skip_head, T, R, first_raw; float rate;
    float *phone; int ph_cs; long long ph_bs;
    int *out_idx; float *out_dist; int *overflow;
};
template <int K> __device__ __forceinline__ void knn_select_blend_body(const KnnSelP &p)
{
    __shared__ float wd[16][K]; __shared__ int wi[16][K];
    __shared__ float sd[K]; __shared__ int si[K];
    __shared__ int cand_i[KNN_CAND]; __shared__ float cand_d[KNN_CAND];
    __shared__ int cnt; __shared__ float s_xn;
    extern __shared__ __attribute__((aligned(16))) float s_rows[];     // [32][dim + 4] candidate rows + the query
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *a = p.approx + (long long)b * p.approx_bs + (long long)j * p.n;
    const float *qv = p.q + (long long)b * p.q_bs + (long long)j * p.dim;
    if (tid == 0) cnt = 0;
    // |x|^2 (only to scale the error margin)
    float xn = 0.f;
    for (int d = tid; d < p.dim; d += 1024) xn += qv[d] * qv[d];
    xn = wave_sum(xn);
    if (lane == 0) wd[wave][0] = xn;
    __syncthreads();
    if (tid == 0) { float t = 0.f; for (int w = 0; w < 16; w++) t += wd[w][0]; s_xn = t; }
    __syncthreads();
    // 1. per-thread sorted top-K of the approximate distances
    float ld[K]; int li_[K];
#pragma unroll
    for (int k = 0; k < K; k++) { ld[k] = INFINITY; li_[k] = 0x7fffffff; }
    // sorted insert with static indices only (a `while (q > 0 && d < ld[q - 1])` walk indexes the arrays dynamically, which puts them
    // in scratch memory): slot q takes its left neighbour if d belongs further left, d itself if it belongs here
    auto keep = [&](float d, int i) {
        if (d < ld[K - 1]) {
#pragma unroll
            for (int q = K - 1; q >= 1; q--) {
                const bool left = d < ld[q - 1], here = !left && d < ld[q];
                ld[q] = left ? ld[q - 1] : (here ? d : ld[q]);
                li_[q] = left ? li_[q - 1] : (here ? i : li_[q]);
            }
            if (d < ld[0]) { ld[0] = d; li_[0] = i; }
        }
    };
    // the scan of the n approximate distances: 16-byte loads, four of them in flight per thread (one load per iteration and a
    // data-dependent branch behind it made this pass ~100 dependent round trips: 80 us for 100 k vectors, more than the scan that
    // produced the distances).  Only the VALUE of the 4th smallest is used below, so the visiting order does not matter.
    const int n4 = ((p.n & 3) == 0 && (reinterpret_cast<size_t>(a) & 15) == 0) ? p.n >> 2 : 0;
    for (int i4 = tid; i4 < n4; i4 += 4 * 1024) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int g = i4 + u * 1024; v[u] = *reinterpret_cast<const f32x4 *>(a + 4 * (g < n4 ? g : i4)); }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int g = i4 + u * 1024;
            if (g < n4) {
#pragma unroll
                for (int e = 0; e < 4; e++) keep(v[u][e], 4 * g + e);
            }
        }
    }
    for (int i = 4 * n4 + tid; i < p.n; i += 1024) keep(a[i], i);
    int pos = 0;
    for (int k = 0; k < K; k++) {
        float md = knn_pick(ld, pos, INFINITY); int mi = knn_pick(li_, pos, 0x7fffffff);
        const float d0 = md; const int i0 = mi;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            float od = __shfl_xor(md, o, 64); int oi = __shfl_xor(mi, o, 64);
            if (od < md || (od == md && oi < mi)) { md = od; mi = oi; }
        }
        if (d0 == md && i0 == mi && mi != 0x7fffffff) pos++;
        if (lane == 0) { wd[wave][k] = md; wi[wave][k] = mi; }
    }
    __syncthreads();
    if (tid == 0) {
        int ps[16];
        for (int w = 0; w < 16; w++) ps[w] = 0;
        float last = INFINITY;
        for (int k = 0; k < K; k++) {
            float md = INFINITY; int mi = 0x7fffffff, mw = 0;
#pragma unroll
            for (int w = 0; w < 16; w++) if (ps[w] < K) {
                float od = wd[w][ps[w]]; int oi = wi[w][ps[w]];
                if (od < md || (od == md && oi < mi)) { md = od; mi = oi; mw = w; }
            }
#pragma unroll
            for (int w = 0; w < 16; w++) ps[w] += w == mw ? 1 : 0;
            last = md;
        }
        sd[0] = last;      // approximate K-th smallest
    }
    __syncthreads();
    // 2. candidates within the error margin of the approximate K-th distance.  fp32 error of approx is bounded by
    //    ~dim*2^-24*(|y|^2 + 2|x||y|) <= 1e-4*(|x|^2 + |y|^2) for dim <= 1024; the margin is 20x that.
    const float aK = sd[0];
    const float margin = 2e-3f * (fabsf(aK + s_xn) + s_xn + 1e-3f);
    const float thr = aK + margin;
    __syncthreads();
    // The candidates are among the per-thread top-K lists unless some thread holds MORE than K values within the margin (its list is
    // then truncated: its K-th entry is still <= thr).  Common case: collect from the lists, no second pass over the n distances.
    if (ld[K - 1] <= thr) atomicOr(&cnt, 0x40000000);       // (a truncated list sends the stream through the full pass below)
    __syncthreads();
    const bool truncated = (cnt & 0x40000000) != 0;
    __syncthreads();
    if (tid == 0) cnt = 0;
    __syncthreads();
    if (!truncated) {
#pragma unroll
        for (int k = 0; k < K; k++)
            if (ld[k] <= thr) { int c = atomicAdd(&cnt, 1); if (c < KNN_CAND) cand_i[c] = li_[k]; }
    } else {
    for (int i4 = tid; i4 < n4; i4 += 4 * 1024) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int g = i4 + u * 1024; v[u] = *reinterpret_cast<const f32x4 *>(a + 4 * (g < n4 ? g : i4)); }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int g = i4 + u * 1024;
            if (g < n4) {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (v[u][e] <= thr) { int c = atomicAdd(&cnt, 1); if (c < KNN_CAND) cand_i[c] = 4 * g + e; }
            }
        }
    }
    for (int i = 4 * n4 + tid; i < p.n; i += 1024) {
        if (a[i] <= thr) { int c = atomicAdd(&cnt, 1); if (c < KNN_CAND) cand_i[c] = i; }
    }
    }
    __syncthreads();
    const int ncand = cnt;
    if (ncand > KNN_CAND) { if (tid == 0) p.overflow[b] = 1; return; }
    // 3. exact distances in the reference's order (ascending-d sequential fmaf), one candidate per thread; the rows are first
    //    staged in LDS with coalesced 16-byte loads (32 candidates per round) so the dependent chain never waits on HBM
    {
        const int RS = p.dim + 4, nv = p.dim >> 2;
        float *s_qv = s_rows + 32 * RS;
        for (int i = tid; i < nv; i += 1024) *reinterpret_cast<f32x4 *>(s_qv + i * 4) = *reinterpret_cast<const f32x4 *>(qv + i * 4);
        for (int base = 0; base < ncand; base += 32) {
            __syncthreads();
            for (int i = tid; i < 32 * nv; i += 1024) {
                const int r = i / nv, c4 = i - r * nv;
                if (base + r < ncand)
                    *reinterpret_cast<f32x4 *>(s_rows + r * RS + c4 * 4) = *reinterpret_cast<const f32x4 *>(p.index + (long long)cand_i[base + r] * p.dim + c4 * 4);
            }
            __syncthreads();
            if (tid < 32 && base + tid < ncand) {
                const float *v = s_rows + tid * RS;
                cand_d[base + tid] = knn_dist_exact(s_qv, v, p.dim);
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < K; k++) {
            float md = INFINITY; int mi = 0x7fffffff, mc = -1;
            for (int c = 0; c < ncand; c++) {
                const float od = cand_d[c]; const int oi = cand_i[c];
                if (oi >= 0 && (od < md || (od == md && oi < mi))) { md = od; mi = oi; mc = c; }
            }
            sd[k] = md; si[k] = mi;
            if (mc >= 0) cand_i[mc] = -1;
        }
    }
    __syncthreads();
    // 4. blend: w = (1/d)^2 normalised, feat = rate * sum w_i y_i + (1 - rate) * feat
    float w[K];
    knn_blend_weights(sd, w);
    for (int r = 0; r < p.R; r++) {
        int s = (p.skip_head + r) / 2; s = s < p.T - 1 ? s : p.T - 1;
        if (s - p.first_raw != j) continue;
        if (tid < K) {
            p.out_idx[((long long)b * p.R + r) * K + tid] = si[tid] == 0x7fffffff ? -1 : si[tid];   // -1: no hit (non-finite query)
            p.out_dist[((long long)b * p.R + r) * K + tid] = sd[tid];
        }
        for (int c = tid; c < p.dim; c += 1024)
            p.phone[(long long)b * p.ph_bs + (long long)c * p.ph_cs + r] = knn_blend_channel(p.index, p.dim, c, si, w, p.rate, qv[c]);
    }
}
// the entry points: K = 4 under the kernel's own name (profiles and rvc_profile_last_knn know it), K = 8 beside it; the plan's k picks one (retrieval.hip)
static __global__ __launch_bounds__(1024) void knn_select_blend_kernel(KnnSelP p) { knn_select_blend_body<KNN_K>(p); }
static __global__ __launch_bounds__(1024) void knn_select_blend_k8_kernel(KnnSelP p) { knn_select_blend_body<KNN_KMAX>(p); }

// unique query rows for retrieval: q[j][c] = cv[c][first_raw + j]
static __global__ void knn_queries_kernel(const float *cv, int cv_cs, long long cv_bs, int C, int first_raw, int nq, float *q)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= nq * C) return;
    int j = i / C, c = i - j * C;
    q[(long long)b * nq * C + i] = cv[(long long)b * cv_bs + (long long)c * cv_cs + first_raw + j];
}

}  // namespace rvc
