// plan_ops.hip.h -- the kernels plan.hip launches besides the implicit-GEMM family (igemm*.hip.h): the second stage of a split-K launch, LayerNorm,
// attention (plain and relative-position), the GRU recurrence and the timeline stamp.  Included by plan.hip only.
#pragma once
#include "igemm_common.hip.h"
#include "state.hip.h"
#include "reduce.hip.h"

namespace rvc {

// second stage of a split-K launch: fixed-order (deterministic) sum of the partials + epilogue
static __global__ __launch_bounds__(256) void splitk_epilogue_kernel(IgemmP p)
{
    const int total = p.M * p.N;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int z = blockIdx.y;
    const int phase = z % p.nphase, b = z / p.nphase;
    const PhaseD ph = p.ph[phase];
    const float *pp = p.part + (long long)(b * p.nphase + phase) * p.ksplit * total + i;
    float acc = 0.f;
    for (int ks = 0; ks < p.ksplit; ks++) acc += pp[(long long)ks * total];
    const int m = i / p.N, n = i - m * p.N;
    epilogue_store(p, ph, b, m, n, acc);
}

// ------------------------------------------------------------------------------------
// normalisation kernels
// ------------------------------------------------------------------------------------
// LayerNorm over channels of x[B][C][ld] for each time step (eps 1e-5), optional in-place.
// block = 4 time steps x 64 channel lanes (so T = 111 already spreads over 28 workgroups); each thread keeps
// its C/64 values in registers: one global read pass, two-pass mean/variance as in the reference definition.
template <int NV>
__global__ __launch_bounds__(256) void layernorm_ct_kernel(const float *x, float *y, const float *g, const float *bta,
                                                           int C, int T, int x_cs, long long x_bs, int y_cs, long long y_bs)
{
    __shared__ float red[4][4];
    const int tx = threadIdx.x & 3, ty = threadIdx.x >> 2;      // ty = 0..63
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * 4 + tx, b = blockIdx.y;
    const bool ok = t < T;
    const float *xp = x + (long long)b * x_bs + (ok ? t : 0);
    float v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        const int c = ty + i * 64;
        v[i] = (ok && c < C) ? xp[(long long)c * x_cs] : 0.f;
        s += v[i];
    }
    float gv[NV], bv[NV];       // loaded now, consumed after the two reductions
#pragma unroll
    for (int i = 0; i < NV; i++) {
        const int c = ty + i * 64;
        gv[i] = c < C ? g[c] : 0.f; bv[i] = c < C ? bta[c] : 0.f;
    }
    // reduce over the 16 lanes of this wave that share tx (lane bits 2..5), then over the 4 waves through LDS
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
    if (lane < 4) red[wave][lane] = s;
    __syncthreads();
    const float mean = (red[0][tx] + red[1][tx] + red[2][tx] + red[3][tx]) / (float)C;
    __syncthreads();
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        const int c = ty + i * 64;
        const float d = (c < C) ? v[i] - mean : 0.f;
        q += d * d;
    }
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) q += __shfl_xor(q, o, 64);
    if (lane < 4) red[wave][lane] = q;
    __syncthreads();
    const float var = (red[0][tx] + red[1][tx] + red[2][tx] + red[3][tx]) / (float)C;
    const float inv = 1.0f / sqrtf(var + 1e-5f);
    if (ok) {
        float *yp = y + (long long)b * y_bs + t;
#pragma unroll
        for (int i = 0; i < NV; i++) {
            const int c = ty + i * 64;
            if (c < C) yp[(long long)c * y_cs] = (v[i] - mean) * inv * gv[i] + bv[i];
        }
    }
}

// Throughput-mode LayerNorm (many streams): a workgroup owns 32 time steps x ALL channels of one stream.  Rows are read and written as
// full 128-byte lines (the 4-step kernel above touches 16-byte slivers of lines that other workgroups -- on other XCDs -- fetch again:
// 156 MB of HBM/MALL reads per launch for 22 MB of data at 64 streams); the tile sits in LDS ([C][33]) for the two-pass statistics.
static __global__ __launch_bounds__(256) void layernorm_tile_kernel(const float *x, float *y, const float *g, const float *bta,
                                                             int C, int T, int x_cs, long long x_bs, int y_cs, long long y_bs)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];      // [C][33]
    __shared__ float red[8][32], s_mean[32], s_inv[32];
    const int t0 = blockIdx.x * 32, b = blockIdx.y, tid = threadIdx.x, tx = tid & 31, part = tid >> 5;
    const float *xb = x + (long long)b * x_bs + t0;
    const bool ok = t0 + tx < T;
    for (int c0 = part; c0 < C; c0 += 8 * 4) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int c = c0 + 8 * u; v[u] = (ok && c < C) ? xb[(long long)c * x_cs + tx] : 0.f; }
#pragma unroll
        for (int u = 0; u < 4; u++) { const int c = c0 + 8 * u; if (c < C) tile[c * 33 + tx] = v[u]; }
    }
    __syncthreads();
    float s = 0.f;
    for (int c = part; c < C; c += 8) s += tile[c * 33 + tx];
    red[part][tx] = s;
    __syncthreads();
    if (part == 0) { float m = 0.f; for (int q = 0; q < 8; q++) m += red[q][tx]; s_mean[tx] = m / (float)C; }
    __syncthreads();
    const float mean = s_mean[tx];
    float qv = 0.f;
    for (int c = part; c < C; c += 8) { const float d = tile[c * 33 + tx] - mean; qv += d * d; }
    red[part][tx] = qv;
    __syncthreads();
    if (part == 0) { float m = 0.f; for (int q = 0; q < 8; q++) m += red[q][tx]; s_inv[tx] = 1.0f / sqrtf(m / (float)C + 1e-5f); }
    __syncthreads();
    if (!ok) return;
    const float inv = s_inv[tx];
    float *yb = y + (long long)b * y_bs + t0;
    for (int c = part; c < C; c += 8) yb[(long long)c * y_cs + tx] = (tile[c * 33 + tx] - mean) * inv * g[c] + bta[c];
}

// Many streams: LayerNorm over channels on 16-column strips, registers only.  A workgroup owns 16 consecutive time steps of one stream
// (one 64-byte segment of every channel row): thread (rg = tid / 4, quad = tid % 4) loads the float4 of rows rg, rg + 64, ... up front
// (NR independent 16-byte loads in flight per thread, no LDS staging), the per-column sums over the 64 row groups go through one
// small LDS exchange, mean and variance are taken from the values still in registers (two-pass, as the reference definition), and
// the strip is written back as float4 (the ragged last quad of a row element-wise, so a halo behind it stays zero).
// The round-1 tile kernel staged [C][32] in 100 KB of LDS: one workgroup per CU, 54 us for 22 MB in + 22 MB out at 64 streams.
template <int NR>
__global__ __launch_bounds__(256) void layernorm_strip_kernel(const float *x, float *y, const float *g, const float *bta,
                                                              int C, int T, int x_cs, long long x_bs, int y_cs, long long y_bs)
{
    __shared__ float red[64][17];
    __shared__ float s_stat[2][16];
    const int t0 = blockIdx.y * 16, b = blockIdx.x, tid = threadIdx.x, quad = tid & 3, rg = tid >> 2;      // (grid: x = stream, y = strip)
    const float *xb = x + (long long)b * x_bs + t0 + quad * 4;
    f32x4 v[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const int c = rg + r * 64;
        v[r] = c < C ? *reinterpret_cast<const f32x4 *>(xb + (long long)c * x_cs) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    f32x4 sm = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < NR; r++) sm += v[r];
#pragma unroll
    for (int j = 0; j < 4; j++) red[rg][quad * 4 + j] = sm[j];
    __syncthreads();
    if (tid < 16) { float m = 0.f; for (int q = 0; q < 64; q++) m += red[q][tid]; s_stat[0][tid] = m / (float)C; }
    __syncthreads();
    f32x4 mean;
#pragma unroll
    for (int j = 0; j < 4; j++) mean[j] = s_stat[0][quad * 4 + j];
    f32x4 qv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < NR; r++) { if (rg + r * 64 < C) { const f32x4 d = v[r] - mean; qv += d * d; } }
#pragma unroll
    for (int j = 0; j < 4; j++) red[rg][quad * 4 + j] = qv[j];
    __syncthreads();
    if (tid < 16) { float m = 0.f; for (int q = 0; q < 64; q++) m += red[q][tid]; s_stat[1][tid] = 1.0f / sqrtf(m / (float)C + 1e-5f); }
    __syncthreads();
    f32x4 inv;
#pragma unroll
    for (int j = 0; j < 4; j++) inv[j] = s_stat[1][quad * 4 + j];
    float *yb = y + (long long)b * y_bs + t0 + quad * 4;
    const int tq = t0 + quad * 4;
    if (tq >= T) return;
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const int c = rg + r * 64;
        if (c >= C) break;
        const float gg = g[c], bb = bta[c];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = (v[r][j] - mean[j]) * inv[j] * gg + bb;
        float *dst = yb + (long long)c * y_cs;
        if (tq + 4 <= T) *reinterpret_cast<f32x4 *>(dst) = o;
        else { for (int j = 0; j < 4 && tq + j < T; j++) dst[j] = o[j]; }
    }
}

// ------------------------------------------------------------------------------------
// attention (fp32 VALU; T <= 256, head_dim <= 128).  K and V of one head live in LDS.
// qkv: [B][3E][ld] (q rows 0..E, k rows E..2E, v rows 2E..3E), out: [B][E][ld]
// Optional relative-position terms (synth TextEncoder): rel_k/rel_v [2*window+1][hd]
// ------------------------------------------------------------------------------------
struct AttnP {
    const float *qkv; float *out;
    int E, T, heads, cs; long long bs;
    int o_cs; long long o_bs;
    float scale;
    const float *rel_k, *rel_v; int window;
    int qloop;      // attention_mfma_kernel: one workgroup per (head, stream) walks all query tiles, keeping its K / V fragments in registers
};

// One workgroup = one head x 16 query rows; each wave owns 4 query rows and keeps 4 accumulators
// live so that every K / V LDS read feeds 4 FMAs.  grid = (heads * ceil(T/16), B)
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

static __global__ __launch_bounds__(256) void attention_kernel(AttnP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int hd = p.E / p.heads, T = p.T, Tp = T | 1;
    const int qtiles = (T + 15) / 16;
    const int h = blockIdx.x / qtiles, qt = blockIdx.x - h * qtiles, b = blockIdx.y;
    float *KVs = smem;                                  // [hd][Tp]: K during the score pass, then V (one buffer: long windows fit)
    float *Ps = smem + ((hd * Tp + 3) & ~3);            // [4 waves][Tp][4]
    float *Qs = Ps + 16 * Tp;                           // [4 waves][hd][4]
    const float *base = p.qkv + (long long)b * p.bs;
    for (int d = threadIdx.x >> 6; d < hd; d += 4)
        for (int t = threadIdx.x & 63; t < T; t += 64) KVs[d * Tp + t] = base[(long long)(p.E + h * hd + d) * p.cs + t];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *P = Ps + wave * 4 * Tp, *Q = Qs + wave * 4 * hd;
    const int t1 = qt * 16 + wave * 4;
    for (int d = lane; d < hd; d += 64) {
        f32x4 qv;
#pragma unroll
        for (int r = 0; r < 4; r++) qv[r] = (t1 + r < T) ? base[(long long)(h * hd + d) * p.cs + t1 + r] * p.scale : 0.f;
        *reinterpret_cast<f32x4 *>(Q + d * 4) = qv;
    }
    __syncthreads();
    const bool active = t1 < T;                          // idle waves of the last tile still take part in the barriers below
    const int W = p.window;
    float inv[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int t2 = lane; t2 < T; t2 += 64) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            for (int d = 0; d < hd; d++) {
                const float kv = KVs[d * Tp + t2];
                const f32x4 qv = *reinterpret_cast<const f32x4 *>(Q + d * 4);
                a[0] += qv[0] * kv; a[1] += qv[1] * kv; a[2] += qv[2] * kv; a[3] += qv[3] * kv;
            }
            if (p.rel_k) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int rr = t2 - (t1 + r);
                    if (rr >= -W && rr <= W) {
                        float ra = 0.f;
                        const float *rk = p.rel_k + (rr + W) * hd;
                        for (int d = 0; d < hd; d++) ra += Q[d * 4 + r] * rk[d];
                        a[r] += ra;
                    }
                }
            }
            *reinterpret_cast<f32x4 *>(P + t2 * 4) = a;
#pragma unroll
            for (int r = 0; r < 4; r++) mx[r] = fmaxf(mx[r], a[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) mx[r] = wave_max(mx[r]);
        float sum[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t2 = lane; t2 < T; t2 += 64) {
            f32x4 e = *reinterpret_cast<const f32x4 *>(P + t2 * 4);
#pragma unroll
            for (int r = 0; r < 4; r++) { e[r] = expf(e[r] - mx[r]); sum[r] += e[r]; }
            *reinterpret_cast<f32x4 *>(P + t2 * 4) = e;
        }
#pragma unroll
        for (int r = 0; r < 4; r++) inv[r] = 1.0f / wave_sum(sum[r]);
        if (p.rel_v) {
            // relative-value path uses normalised probabilities (same order as the reference definition)
            for (int t2 = lane; t2 < T; t2 += 64) {
                f32x4 e = *reinterpret_cast<const f32x4 *>(P + t2 * 4);
#pragma unroll
                for (int r = 0; r < 4; r++) e[r] *= inv[r];
                *reinterpret_cast<f32x4 *>(P + t2 * 4) = e;
            }
        }
    }
    __syncthreads();                                     // every wave is done with K
    for (int d = threadIdx.x >> 6; d < hd; d += 4)
        for (int t = threadIdx.x & 63; t < T; t += 64) KVs[d * Tp + t] = base[(long long)(2 * p.E + h * hd + d) * p.cs + t];
    __syncthreads();
    if (!active) return;
    for (int d = lane; d < hd; d += 64) {
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        const float *vr = KVs + d * Tp;
        for (int t2 = 0; t2 < T; t2++) {
            const float vv = vr[t2];
            const f32x4 pr = *reinterpret_cast<const f32x4 *>(P + t2 * 4);
            o[0] += pr[0] * vv; o[1] += pr[1] * vv; o[2] += pr[2] * vv; o[3] += pr[3] * vv;
        }
        if (p.rel_v) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int tq = t1 + r;
                int lo = tq - W < 0 ? 0 : tq - W, hi = tq + W >= T ? T - 1 : tq + W;
                float acc = o[r];
                for (int t2 = lo; t2 <= hi; t2++) acc += P[t2 * 4 + r] * p.rel_v[(t2 - tq + W) * hd + d];
                o[r] = acc;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; r++) o[r] *= inv[r];
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (t1 + r < T) p.out[(long long)b * p.o_bs + (long long)(h * hd + d) * p.o_cs + t1 + r] = o[r];
    }
}

// Matrix-core attention for ContentVec (no relative terms, T <= 64*KF).  One workgroup = one head x 16 query rows.
// Latency-shaped for B = 1: every global operand (the Q tile, this wave's K fragments, this wave's V fragments) is loaded into
// registers up front in fully unrolled code, so the kernel pays ~one memory round trip instead of one per loop iteration.
// S = (Q*scale) K^T: A = Q tile, B = K (lanes along t, coalesced), the 4 waves split the key fragments.  Softmax over the
// D fragments (16-lane shuffles + a 4-wave LDS exchange).  O = P V: P goes through LDS into the A layout, V stays in registers
// in the B layout (lane (kq, li) holds V[d = dt*16 + li][t = 4c + kq]); the 4 waves split head_dim (HD/16 <= 4 fragments... one per wave
// for HD = 64; HD = 128 would need two passes and is handled by the VALU kernel).
template <int HD, int KF>
__global__ __launch_bounds__(256) void attention_mfma_kernel(AttnP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NC = KF * 16;                // t-chunks of 4 covered by the V registers
    const int T = p.T;
    const int qtiles = (T + 15) / 16, kfr = (T + 15) / 16;
    // many streams (qloop): the K and V fragments of a head do not depend on the query tile, so one workgroup per (head, stream) loads them
    // once and walks the query tiles (7 at T = 111): the K / V re-reads -- 5376 workgroups x 57 KB per layer at 64 streams -- drop 7-fold
    const int h = p.qloop ? (int)blockIdx.x : (int)blockIdx.x / qtiles, qt_first = p.qloop ? 0 : (int)blockIdx.x - h * qtiles, b = blockIdx.y;
    const int qt_last = p.qloop ? qtiles : qt_first + 1;
    const int Tq = KF * 64 + 1;
    float *Ps = smem;                         // [16][Tq]
    float *red = Ps + 16 * Tq;                // [4 waves][16 rows] x 2
    const float *base = p.qkv + (long long)b * p.bs;
    const float *qb = base + (long long)(h * HD) * p.cs, *kb = base + (long long)(p.E + h * HD) * p.cs, *vb = base + (long long)(2 * p.E + h * HD) * p.cs;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
    float qa[HD / 4], kv[HD / 4][KF], vv[NC];
    {
#pragma unroll
        for (int f = 0; f < KF; f++) {
            int t2 = (wave + f * 4) * 16 + li; t2 = t2 < T ? t2 : T - 1;
#pragma unroll
            for (int c = 0; c < HD / 4; c++) kv[c][f] = kb[(long long)(c * 4 + kq) * p.cs + t2];
        }
        const float *vr = vb + (long long)(wave * 16 + li) * p.cs + kq;
#pragma unroll
        for (int c = 0; c < NC; c++) vv[c] = (wave * 16 < HD && c * 4 + kq < T) ? vr[c * 4] : 0.f;
    }
    {
        const int tq = qt_first * 16 + li < T ? qt_first * 16 + li : T - 1;
#pragma unroll
        for (int c = 0; c < HD / 4; c++) qa[c] = qb[(long long)(c * 4 + kq) * p.cs + tq];
    }
    for (int qt = qt_first; qt < qt_last; qt++) {
    const int t1 = qt * 16;
    if (qt != qt_first) __syncthreads();         // the previous tile's probabilities / statistics have been consumed
    f32x4 sacc[KF];
#pragma unroll
    for (int f = 0; f < KF; f++) sacc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < HD / 4; c++) {
        const float a = qa[c] * p.scale;
#pragma unroll
        for (int f = 0; f < KF; f++) sacc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, kv[c][f], sacc[f], 0, 0, 0);
    }
    // (round 6) the NEXT query tile's rows are requested as soon as this tile's products have consumed the registers: the walk over the query tiles of a
    // (head, stream) paid one memory round trip per tile in front of its first MFMA (7 per workgroup at T = 111)
    if (qt + 1 < qt_last) {
        const int tq = t1 + 16 + li < T ? t1 + 16 + li : T - 1;
#pragma unroll
        for (int c = 0; c < HD / 4; c++) qa[c] = qb[(long long)(c * 4 + kq) * p.cs + tq];
    }
    // row statistics: this lane holds rows kq*4 + r, column li of each of its key fragments
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int f = 0; f < KF; f++) {
        const int kf = wave + f * 4;
        const bool ok = kf < kfr && kf * 16 + li < T;
#pragma unroll
        for (int r = 0; r < 4; r++) { if (!ok) sacc[f][r] = -INFINITY; mx[r] = fmaxf(mx[r], sacc[f][r]); }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], o, 64));
        if (li == 0) red[wave * 16 + kq * 4 + r] = mx[r];
    }
    __syncthreads();
    float sum[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = kq * 4 + r;
        mx[r] = fmaxf(fmaxf(red[row], red[16 + row]), fmaxf(red[32 + row], red[48 + row]));
        sum[r] = 0.f;
    }
#pragma unroll
    for (int f = 0; f < KF; f++) {
        const int kf = wave + f * 4;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float e = expf(sacc[f][r] - mx[r]);      // exp(-inf) = 0 for the masked columns
            sum[r] += e;
            Ps[(kq * 4 + r) * Tq + kf * 16 + li] = e;       // every column of [0, 64*KF) is written (zeros beyond T)
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) sum[r] += __shfl_xor(sum[r], o, 64);
        if (li == 0) red[64 + wave * 16 + kq * 4 + r] = sum[r];
    }
    __syncthreads();
    // O = P V, this wave's head_dim fragment dt = wave
    if (wave * 16 < HD) {
        f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
        const float *pr = Ps + li * Tq + kq;
#pragma unroll
        for (int c = 0; c < NC; c += 2) {
            o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[c * 4], vv[c], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[c * 4 + 4], vv[c + 1], o1, 0, 0, 0);
        }
        // D: row = kq*4 + r (query), col = li (d)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = kq * 4 + r, tq = t1 + row;
            const float inv = 1.0f / (red[64 + row] + red[64 + 16 + row] + red[64 + 32 + row] + red[64 + 48 + row]);
            if (tq < T) p.out[(long long)b * p.o_bs + (long long)(h * HD + wave * 16 + li) * p.o_cs + tq] = (o0[r] + o1[r]) * inv;
        }
    }
    }
}

// Small-T attention with relative-position terms (synthesizer TextEncoder: T = return_length <= 64, 2 heads x 96).
// grid = (heads * ceil(T/4), streams); a workgroup owns 4 query rows of one head (one per wave), lanes run along the key axis.
// K, V, both relative tables and the 4 Q rows are staged "all loads into registers, then all LDS stores" in unrolled batches
// (the kernel is a latency chain at B = 1); the dot products keep the sequential d / j order of the definition.
static __global__ __launch_bounds__(256) void relpos_attention_small_kernel(AttnP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NT = 256;
    const int hd = p.E / p.heads, T = p.T, Tp = T | 1, W = p.window, NR = 2 * W + 1;
    const int qtiles = (T + 3) / 4;
    const int h = blockIdx.x / qtiles, qt = blockIdx.x - h * qtiles, b = blockIdx.y;
    float *Ks = smem, *Vs = Ks + hd * Tp;                          // [hd][Tp] each, contiguous: K, V
    float *Rk = Vs + hd * Tp, *Rv = Rk + NR * hd;                  // [NR][hd] each, contiguous
    float *Qs = Rv + NR * hd;                                      // [4][hd]
    float *S = Qs + 4 * hd;                                        // [4][64]
    const float *base = p.qkv + (long long)b * p.bs;
    // staging without integer divisions (the first version spent most of its 19 us on them: three per staged element): K / V rows
    // are walked as (d, t) with t padded to a power of two, the relative-position tables are one contiguous copy, Q one row per pass
    // All global loads are issued before the first LDS write (one memory round trip for the whole staging instead of one per loop
    // iteration: the kernel was bound by exactly that serialisation).
    const int tsh = T <= 32 ? 5 : 6, tmask = (1 << tsh) - 1;
    constexpr int KV_IT = 16, RT_IT = 12;
    const int kv_n = hd << tsh, rt_n = NR * hd;
    float kk[KV_IT], vv[KV_IT], rk[RT_IT], rv[RT_IT], qq[4];
#pragma unroll
    for (int u = 0; u < KV_IT; u++) {
        const int idx = threadIdx.x + u * NT, d = idx >> tsh, t = idx & tmask;
        const bool ok = idx < kv_n && t < T;
        kk[u] = ok ? base[(long long)(p.E + h * hd + d) * p.cs + t] : 0.f;
        vv[u] = ok ? base[(long long)(2 * p.E + h * hd + d) * p.cs + t] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < RT_IT; u++) {
        const int j = threadIdx.x + u * NT;
        rk[u] = j < rt_n ? p.rel_k[j] : 0.f;
        rv[u] = j < rt_n ? p.rel_v[j] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int tq = qt * 4 + r;
        qq[r] = (threadIdx.x < hd && tq < T) ? base[(long long)(h * hd + threadIdx.x) * p.cs + tq] * p.scale : 0.f;
    }
#pragma unroll
    for (int u = 0; u < KV_IT; u++) {
        const int idx = threadIdx.x + u * NT, d = idx >> tsh, t = idx & tmask;
        if (idx < kv_n && t < T) { Ks[d * Tp + t] = kk[u]; Vs[d * Tp + t] = vv[u]; }
    }
#pragma unroll
    for (int u = 0; u < RT_IT; u++) {
        const int j = threadIdx.x + u * NT;
        if (j < rt_n) { Rk[j] = rk[u]; Rv[j] = rv[u]; }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) if (threadIdx.x < hd) Qs[r * hd + threadIdx.x] = qq[r];
    // sizes beyond the unrolled staging (not reached by any official configuration: 2 heads x 96, window 10, T <= 64)
    for (int idx = threadIdx.x + KV_IT * NT; idx < kv_n; idx += NT) {
        const int d = idx >> tsh, t = idx & tmask;
        if (t < T) { Ks[d * Tp + t] = base[(long long)(p.E + h * hd + d) * p.cs + t]; Vs[d * Tp + t] = base[(long long)(2 * p.E + h * hd + d) * p.cs + t]; }
    }
    for (int j = threadIdx.x + RT_IT * NT; j < rt_n; j += NT) { Rk[j] = p.rel_k[j]; Rv[j] = p.rel_v[j]; }
    for (int d = threadIdx.x + NT; d < hd; d += NT)
        for (int r = 0; r < 4; r++) { const int tq = qt * 4 + r; Qs[r * hd + d] = tq < T ? base[(long long)(h * hd + d) * p.cs + tq] * p.scale : 0.f; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = qt * 4 + wave;
    if (i >= T) return;
    const float *q = Qs + wave * hd;
    float *Sr = S + wave * 64;
    float sc = -INFINITY;
    if (lane < T) {
        const int j = lane;
        float a = 0.f;
#pragma unroll 8
        for (int d = 0; d < hd; d++) a += q[d] * Ks[d * Tp + j];
        const int r = j - i;
        if (r >= -W && r <= W) {
            float ra = 0.f;
            const float *rk = Rk + (r + W) * hd;
#pragma unroll 8
            for (int d = 0; d < hd; d++) ra += q[d] * rk[d];
            a += ra;
        }
        sc = a;
    }
    const float mx = wave_max(sc);
    const float ex = lane < T ? expf(sc - mx) : 0.f;
    const float inv = 1.0f / wave_sum(ex);
    if (lane < T) Sr[lane] = ex * inv;
    wave_lds_sync();
    const int lo = i - W < 0 ? 0 : i - W, hi = i + W >= T ? T - 1 : i + W;
    for (int d = lane; d < hd; d += 64) {
        float a = 0.f;
#pragma unroll 8
        for (int j = 0; j < T; j++) a += Sr[j] * Vs[d * Tp + j];
#pragma unroll 8
        for (int j = lo; j <= hi; j++) a += Sr[j] * Rv[(j - i + W) * hd + d];
        p.out[(long long)b * p.o_bs + (long long)(h * hd + d) * p.o_cs + i] = a;
    }
}

// The same attention on the matrix cores (one stream: the VALU kernel above is a latency chain of ~200 dependent LDS-read + FMA steps per lane,
// 12.4 us per layer).  grid = (heads * ceil(T / 16), streams): a workgroup owns 16 query columns of one head.  Every product is a 16x16x4 fp32
// MFMA (A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15], D[row = (lane >> 4) * 4 + r][col = lane & 15]):
//   scores[i][j] = sum_d q[d][i] k[d][j]            P[i][r] = sum_d q[d][i] rel_k[r][d]        scores[i][j] += P[i][j - i + W] inside the window
//   out[c][i]    = sum_j v[c][j] S[i][j] + sum_r rel_v[r][c] Ssk[i][r]      with Ssk[i][r] = S[i][i + r - W] (zero outside [0, T))
// Padded k (j >= T, r >= NR) multiplies a ZEROED S / Ssk entry by a finite staged value; padded rows / columns of D are not stored.
static __global__ __launch_bounds__(256) void relpos_attention_mfma_kernel(AttnP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NT = 256;
    const int kc = p.E / p.heads, T = p.T, TP = T | 1, Wd = p.window, NR = 2 * Wd + 1, NRP = (NR + 3) & ~3;
    const int JF = (T + 15) >> 4, SW = JF * 16, RF = (NR + 15) >> 4, PW = RF * 16;
    const int h = blockIdx.x / JF, qb = blockIdx.x - h * JF, b = blockIdx.y;
    const int col0 = qb * 16, nq = T - col0 < 16 ? T - col0 : 16;
    float *q = smem, *kk = q + kc * 16, *vv = kk + kc * TP, *rk = vv + kc * TP, *rv = rk + PW * kc;
    float *Sx = rv + NRP * kc, *P = Sx + 16 * SW, *Ssk = P + 16 * PW;
    const float *base = p.qkv + (long long)b * p.bs;
    // staging: every global load is issued before the first LDS write (one memory round trip)
    const int tsh = T <= 32 ? 5 : 6, tmask = (1 << tsh) - 1;
    constexpr int KV_IT = 16, RT_IT = 12, Q_IT = 6;
    const int kv_n = kc << tsh, rk_n = PW * kc, rv_n = NRP * kc, rt_n = NR * kc, q_n = kc * 16;
    float kr[KV_IT], vr[KV_IT], rkr[RT_IT], rvr[RT_IT], qr[Q_IT];
#pragma unroll
    for (int u = 0; u < Q_IT; u++) {
        const int idx = threadIdx.x + u * NT, d = idx >> 4, c = idx & 15;
        qr[u] = (idx < q_n && c < nq) ? base[(long long)(h * kc + d) * p.cs + col0 + c] * p.scale : 0.f;
    }
#pragma unroll
    for (int u = 0; u < KV_IT; u++) {
        const int idx = threadIdx.x + u * NT, d = idx >> tsh, t = idx & tmask;
        const bool ok = idx < kv_n && t < T;
        kr[u] = ok ? base[(long long)(p.E + h * kc + d) * p.cs + t] : 0.f;
        vr[u] = ok ? base[(long long)(2 * p.E + h * kc + d) * p.cs + t] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < RT_IT; u++) {
        const int j = threadIdx.x + u * NT;
        rkr[u] = j < rt_n ? p.rel_k[j] : 0.f;
        rvr[u] = j < rt_n ? p.rel_v[j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < Q_IT; u++) { const int idx = threadIdx.x + u * NT; if (idx < q_n) q[idx] = qr[u]; }
#pragma unroll
    for (int u = 0; u < KV_IT; u++) {
        const int idx = threadIdx.x + u * NT, d = idx >> tsh, t = idx & tmask;
        if (idx < kv_n && t < TP) { kk[d * TP + t] = kr[u]; vv[d * TP + t] = vr[u]; }       // (column T of the odd padding: zero)
    }
#pragma unroll
    for (int u = 0; u < RT_IT; u++) {
        const int j = threadIdx.x + u * NT;
        if (j < rk_n) rk[j] = rkr[u];
        if (j < rv_n) rv[j] = rvr[u];
    }
    // sizes beyond the unrolled staging (no official configuration: 2 heads x 96, window 10, T <= 32)
    for (int idx = threadIdx.x + Q_IT * NT; idx < q_n; idx += NT) { const int d = idx >> 4, c = idx & 15; q[idx] = c < nq ? base[(long long)(h * kc + d) * p.cs + col0 + c] * p.scale : 0.f; }
    for (int idx = threadIdx.x + KV_IT * NT; idx < kv_n; idx += NT) {
        const int d = idx >> tsh, t = idx & tmask;
        if (t < TP) { kk[d * TP + t] = t < T ? base[(long long)(p.E + h * kc + d) * p.cs + t] : 0.f; vv[d * TP + t] = t < T ? base[(long long)(2 * p.E + h * kc + d) * p.cs + t] : 0.f; }
    }
    for (int j = threadIdx.x + RT_IT * NT; j < rk_n; j += NT) rk[j] = j < rt_n ? p.rel_k[j] : 0.f;
    for (int j = threadIdx.x + RT_IT * NT; j < rv_n; j += NT) rv[j] = j < rt_n ? p.rel_v[j] : 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
    // scores and P: items (16-column block of keys), then (16-row block of relative positions), one per wave and pass
    for (int it = wave; it < JF + RF; it += 4) {
        const bool is_p = it >= JF;
        const int f = is_p ? it - JF : it;
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
        const float *qa = q + kq * 16 + li;
        const float *bb = is_p ? rk + (f * 16 + li) * kc + kq : kk + kq * TP + f * 16 + li;
        const int bst = is_p ? 4 : 4 * TP;
        for (int ks = 0; ks + 1 < kc / 4; ks += 2) {
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[ks * 64], bb[ks * bst], a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[(ks + 1) * 64], bb[(ks + 1) * bst], a1, 0, 0, 0);
        }
        if ((kc / 4) & 1) a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[(kc / 4 - 1) * 64], bb[(kc / 4 - 1) * bst], a0, 0, 0, 0);
        a0 += a1;
        float *dst = is_p ? P + f * 16 : Sx + f * 16;
        const int dw = is_p ? PW : SW;
#pragma unroll
        for (int r = 0; r < 4; r++) dst[(kq * 4 + r) * dw + li] = a0[r];
    }
    __syncthreads();
    // softmax with the relative-position term: 16 lanes per query row, keys strided over the lanes
    {
        const int i = threadIdx.x >> 4, gi = col0 + i;
        float *Sr = Sx + i * SW, *Kr = Ssk + i * PW;
        const float *Pr = P + i * PW;
        float mx = -INFINITY;
        if (gi < T) {
            for (int j = li; j < T; j += 16) {
                float a = Sr[j];
                const int r = j - gi;
                if (r >= -Wd && r <= Wd) a += Pr[r + Wd];
                Sr[j] = a; mx = fmaxf(mx, a);
            }
        }
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 16));
        float sum = 0.f;
        if (gi < T) for (int j = li; j < T; j += 16) { const float ex = expf(Sr[j] - mx); Sr[j] = ex; sum += ex; }
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 16);
        const float inv = 1.0f / sum;
        for (int j = li; j < SW; j += 16) Sr[j] = (gi < T && j < T) ? Sr[j] * inv : 0.f;
        // (the 16 lanes of a row run in lockstep inside one wave: Sr is complete before it is read back skewed)
        for (int r = li; r < PW; r += 16) { const int j = gi + r - Wd; Kr[r] = (gi < T && r < NR && j >= 0 && j < T) ? Sr[j] : 0.f; }
    }
    __syncthreads();
    // attention output of the own columns: items = 16-channel blocks of the head
    for (int cf = wave; cf < kc / 16; cf += 4) {
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
        const float *va = vv + (cf * 16 + li) * TP + kq, *sb = Sx + li * SW + kq;
        for (int ks = 0; ks < (T + 3) / 4; ks++) a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(va[ks * 4], sb[ks * 4], a0, 0, 0, 0);
        const float *ra = rv + kq * kc + cf * 16 + li, *kb = Ssk + li * PW + kq;
        for (int ks = 0; ks < NRP / 4; ks++) a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[ks * 4 * kc], kb[ks * 4], a1, 0, 0, 0);
        a0 += a1;
        // D: row = channel cf * 16 + kq * 4 + r, col = query li
        if (col0 + li < T) {
#pragma unroll
            for (int r = 0; r < 4; r++) p.out[(long long)b * p.o_bs + (long long)(h * kc + cf * 16 + kq * 4 + r) * p.o_cs + col0 + li] = a0[r];
        }
    }
}

// ------------------------------------------------------------------------------------
// RMVPE head: bidirectional GRU recurrence (input projections come from the implicit GEMM)
// gi: [B][2*3H][ld] (forward gates rows 0..3H, backward rows 3H..6H; biases b_ih included)
// whhT: [2][H][3H] (transposed so lanes read consecutive rows), bhh: [2][3H]
// out: [B][2H][ld] (forward h rows 0..H, backward rows H..2H)
// ------------------------------------------------------------------------------------
static __global__ __launch_bounds__(1024) void gru_kernel(const float *gi, int gi_cs, long long gi_bs, const float *whhT, const float *bhh,
                                                   float *out, int o_cs, long long o_bs, int H, int Tm)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *hs = smem;          // [H]
    float *gh = smem + H;      // [3H]
    const int dir = blockIdx.x, b = blockIdx.y, r = threadIdx.x;
    const float *gib = gi + (long long)b * gi_bs + (long long)dir * 3 * H * gi_cs;
    const float *wt = whhT + (long long)dir * H * 3 * H;
    const float *bh = bhh + dir * 3 * H;
    float *ob = out + (long long)b * o_bs + (long long)dir * H * o_cs;
    if (r < H) hs[r] = 0.f;
    __syncthreads();
    for (int step = 0; step < Tm; step++) {
        const int t = dir == 0 ? step : Tm - 1 - step;
        if (r < 3 * H) {
            float a = bh[r];
            for (int j = 0; j < H; j++) a += wt[(long long)j * 3 * H + r] * hs[j];
            gh[r] = a;
        }
        __syncthreads();
        if (r < H) {
            float ir = gib[(long long)r * gi_cs + t], iz = gib[(long long)(H + r) * gi_cs + t], in_ = gib[(long long)(2 * H + r) * gi_cs + t];
            float rg = 1.0f / (1.0f + expf(-(ir + gh[r])));
            float zg = 1.0f / (1.0f + expf(-(iz + gh[H + r])));
            float ng = tanhf(in_ + rg * gh[2 * H + r]);
            float hn = (1.f - zg) * ng + zg * hs[r];
            hs[r] = hn;
            ob[(long long)r * o_cs + t] = hn;
        }
        __syncthreads();
    }
}

// Multi-CU recurrence for few streams (B <= 8): 8 workgroups per direction, each owning 32 hidden units = 96 gate rows
// whose 96 KB slice of W_hh stays in LDS for all steps.  After every step the 8 slices exchange their 32 new h values through
// 8-byte {epoch, value} granules (cdna_hip_programming.md guideline 16, form R2: the data is the flag; relaxed agent-scope
// stores / loads, no fences, placement independent).  Two granule slots alternate by step parity; the granule buffer is zeroed
// by a memset node before every launch of a captured graph, and once per plan for eager launches (GruMultiP::epoch).  Every spin is bounded: on timeout the stream's status word is raised instead of hanging.
struct GruMultiP {
    const float *gi; int gi_cs; long long gi_bs;
    const float *whh;          // [2][3H][H] row-major
    const float *bhh;          // [2][3H]
    float *out; int o_cs; long long o_bs;
    unsigned long long *gran;  // [B][2 dirs][2 slots][H]
    int *status;               // per stream, stride status_stride ints
    int status_stride;
    int Tm;
    unsigned epoch;            // tags of this launch are epoch + 1 ... epoch + Tm (round 6: the host advances it by Tm per launch, so stale granules of earlier
                               // chunks never match and the buffer needs no memset in front of every launch -- a 5 us fill kernel on the f0 chain)
};
// Round 3: the 96 x 256 slice of W_hh lives in REGISTERS (thread (row r, quarter q) keeps its 64 weights for all steps: the matvec
// reads only h from LDS, 16 broadcast b128 reads per thread, instead of streaming 96 KB of weights through LDS every step), the
// slice's input gates gi[Tm][96] are copied to LDS once (they were three global loads per step on the critical path), and a step
// has two workgroup barriers instead of three.  384 threads; 98 -> ~45 us for 2 x 32 steps.
static __global__ __launch_bounds__(384) void gru_multi_kernel(GruMultiP p)
{
    constexpr int H = 256, G = 8, U = H / G, ROWS = 3 * U, NT = 384;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *hs = smem;                   // [H]
    float *gh = hs + H;                 // [ROWS]
    float *gis = gh + ROWS;             // [Tm][ROWS]: input gates of this slice (b_ih included), row = gate * U + unit
    const int g = blockIdx.x, dir = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int r = tid >> 2, q = tid & 3;                 // row of the slice, quarter of the hidden vector
    const int gate = r / U, u = r - gate * U;
    const float *wsrc = p.whh + (long long)dir * 3 * H * H + (long long)(gate * H + g * U + u) * H + q * 64;
    f32x4 w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = *reinterpret_cast<const f32x4 *>(wsrc + i * 4);
    const float bias = p.bhh[dir * 3 * H + gate * H + g * U + u];
    const float *gib = p.gi + (long long)b * p.gi_bs + (long long)dir * 3 * H * p.gi_cs;
    // (round 6: in batches of eight requests -- one memory round trip per batch instead of one per element of the strided copy loop)
    for (int i0 = tid; i0 < p.Tm * ROWS; i0 += 8 * NT) {
        float v8[8]; int d8[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int i = i0 + k * NT;
            const bool ok = i < p.Tm * ROWS;
            const int ii = ok ? i : 0;
            const int rr = ii / p.Tm, t = ii - rr * p.Tm, gg = rr / U, uu = rr - gg * U;      // coalesced along time
            v8[k] = gib[(long long)(gg * H + g * U + uu) * p.gi_cs + t];
            d8[k] = ok ? t * ROWS + rr : -1;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) if (d8[k] >= 0) gis[d8[k]] = v8[k];
    }
    if (tid < H) hs[tid] = 0.f;
    float *ob = p.out + (long long)b * p.o_bs + (long long)dir * H * p.o_cs;
    unsigned long long *gr = p.gran + ((long long)(b * 2 + dir) * 2) * H;
    __syncthreads();
    bool dead = false;
    for (int step = 0; step < p.Tm; step++) {
        const int t = dir == 0 ? step : p.Tm - 1 - step;
        if (step > 0) {
            // gather h_{step-1}: granule `tid` of slot (step-1)&1 must carry tag == step
            if (tid < H) {
                const unsigned long long *src = gr + ((step - 1) & 1) * H + tid;
                unsigned long long x = 0;
                unsigned spins = 0;
                while (!dead) {
                    x = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((unsigned)(x >> 32) == p.epoch + (unsigned)step) break;
                    if (++spins > (1u << 22)) { dead = true; atomicOr(&p.status[b * p.status_stride], (int)ST_HANDOFF); }
                    __builtin_amdgcn_s_sleep(1);
                }
                hs[tid] = __uint_as_float((unsigned)x);
            }
            __syncthreads();
        }
        // row r, columns q * 64 ..: the four quarters of a row sit in adjacent lanes
        {
            const float *hq = hs + q * 64;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const f32x4 hv = *reinterpret_cast<const f32x4 *>(hq + i * 4);
                a0 = fmaf(w[i][0], hv[0], a0); a1 = fmaf(w[i][1], hv[1], a1); a2 = fmaf(w[i][2], hv[2], a2); a3 = fmaf(w[i][3], hv[3], a3);
            }
            float a = (a0 + a1) + (a2 + a3);
            a += __shfl_xor(a, 1, 64);
            a += __shfl_xor(a, 2, 64);
            if (q == 0) gh[r] = a + bias;
        }
        __syncthreads();
        if (tid < U) {
            const int unit = g * U + tid;
            const float *gi = gis + t * ROWS;
            const float ir = gi[tid], iz = gi[U + tid], in_ = gi[2 * U + tid];
            const float rg = 1.0f / (1.0f + expf(-(ir + gh[tid])));
            const float zg = 1.0f / (1.0f + expf(-(iz + gh[U + tid])));
            const float ng = tanhf(in_ + rg * gh[2 * U + tid]);
            const float hn = (1.f - zg) * ng + zg * hs[unit];
            ob[(long long)unit * p.o_cs + t] = hn;
            __hip_atomic_store(gr + (step & 1) * H + unit, ((unsigned long long)(p.epoch + (unsigned)(step + 1)) << 32) | (unsigned long long)__float_as_uint(hn),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // (no barrier here: hs[unit] of the own slice is rewritten only after this thread's granule has been polled back, gh only
        // after the next step's first barrier)
    }
}

// timeline probe (RVC_STAMPS=1): device wall clock (constant 100 MHz) at a point of a stream's kernel chain
static __global__ void stamp_kernel(unsigned long long *slot) { *slot = wall_clock64(); }

}  // namespace rvc
