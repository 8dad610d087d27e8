// resample_whole.hip.h -- one-shot sample-rate conversion of a whole signal, included by engine.hip.  Not the streaming rubato mirror
// (resample.hip.h): a windowed-sinc polyphase converter with the formant stage's filter (formant_table.h: Hann-windowed sinc, width 6, rolloff 0.99).
// Definition (resample_geometry.h): o / n = rate_in / rate_out reduced, w = ceil(6 o / (0.99 min(o, n))), K = 2 w + o, N_out = ceil(N_in n / o),
//   y[i n + j] = sum_{k = 0 .. K-1} h[j][k] x[i o + k - w],   x = 0 outside [0, N_in)
// Each output is ONE fp32 fma chain over ascending k through the compact row of its phase (taps [kb[j], kb[j] + Kt); what the compact row leaves out are
// exact zeros): the result does not depend on the launch shape, nor on which of the two kernels below ran.  o == n is a copy.
#pragma once
#include "resample_geometry.h"

namespace rvc {

constexpr int RSW_THREADS = 256;
constexpr size_t RSW_LDS_FLOATS = 12288;      // 48 KB: what the staged kernel may take (three workgroups per CU)

// How a tile of `tile` consecutive outputs is staged: rows = table rows held (all n, or one per output when the tile is shorter than the phase cycle), Ks = the
// LDS stride of a row (odd: consecutive lanes read consecutive rows at one tap), span = input samples held, from x[(m0 / n) o - w]:
//   the tile's outputs lie in blocks i_lo = m0 / n .. i_hi <= i_lo + 1 + (tile - 2) / n, and output (i, j) reads x[i o - w + kb[j] + t], t < Kt, kb[j] <= K - 1
struct RswTile { int tile, rows, Ks, span; size_t floats() const { return (size_t)rows * Ks + span; } };
static inline RswTile rsw_tile(int o, int n, int K, int Kt, int per_thread)
{
    RswTile t;
    t.tile = RSW_THREADS * per_thread;
    t.rows = std::min(n, t.tile);
    t.Ks = Kt | 1;
    t.span = ((t.tile - 1) / n + 1) * o + K + Kt;
    return t;
}

// one workgroup = `tile` consecutive outputs from m0 = blockIdx.x * tile; thread t owns outputs m0 + t + 256 q.  LDS: hs [rows][Ks], then xs [span]
static __global__ __launch_bounds__(RSW_THREADS) void resample_whole_lds_kernel(const float *x, long long n_in, const float *tab, const int *kb, int o, int n, int w, int Kt,
                                                                                 int tile, int rows, int Ks, int span, float *y, long long n_out)
{
    extern __shared__ float rsw_lds[];
    float *hs = rsw_lds, *xs = rsw_lds + (size_t)rows * Ks;
    const long long m0 = (long long)blockIdx.x * tile;
    const long long i_lo = m0 / n;
    const int j0 = (int)(m0 - i_lo * n);
    const bool all_rows = rows == n;      // else: rows == tile < n, local row r holds phase (j0 + r) % n
    for (int q = threadIdx.x; q < rows * Kt; q += RSW_THREADS) {
        const int r = q / Kt, t = q - r * Kt;
        const int j = all_rows ? r : (j0 + r) % n;
        hs[r * Ks + t] = tab[(size_t)j * Kt + t];
    }
    const long long x0 = i_lo * o - w;
    for (int q = threadIdx.x; q < span; q += RSW_THREADS) {
        const long long src = x0 + q;
        xs[q] = (src >= 0 && src < n_in) ? x[src] : 0.f;
    }
    __syncthreads();
    for (int r = threadIdx.x; r < tile; r += RSW_THREADS) {
        const long long m = m0 + r;
        if (m >= n_out) break;
        const long long i = m / n;
        const int j = (int)(m - i * n);
        const float *h = hs + (all_rows ? j : r) * Ks;
        const float *xp = xs + (int)(i - i_lo) * o + kb[j];      // < span: see rsw_tile
        float acc = 0.f;
        for (int t = 0; t < Kt; t++) acc = fmaf(h[t], xp[t], acc);
        y[m] = acc;
    }
}

// the same chain from global memory, one thread per output: ratios whose tile does not fit the LDS budget (a long filter, or many input samples per output)
static __global__ __launch_bounds__(RSW_THREADS) void resample_whole_direct_kernel(const float *x, long long n_in, const float *tab, const int *kb, int o, int n, int w, int Kt,
                                                                                    float *y, long long n_out)
{
    const long long m = (long long)blockIdx.x * RSW_THREADS + threadIdx.x;
    if (m >= n_out) return;
    const long long i = m / n;
    const int j = (int)(m - i * n);
    const float *h = tab + (size_t)j * Kt;
    const long long s0 = i * o - w + kb[j];
    float acc = 0.f;
    for (int t = 0; t < Kt; t++) {
        const long long src = s0 + t;
        acc = fmaf(h[t], (src >= 0 && src < n_in) ? x[src] : 0.f, acc);
    }
    y[m] = acc;
}

// d_y [g.n_out] = d_x [n_in] converted, queued on the engine's stream.  The table of a ratio is built once per engine (formant_table_dev: the formant stage's cache)
static void launch_resample_whole(rvc_engine *e, const float *d_x, size_t n_in, const ResampleGeometry &g, float *d_y)
{
    hipStream_t st = e->stream;
    if (g.o == g.n) { HIPCHK(hipMemcpyAsync(d_y, d_x, n_in * sizeof(float), hipMemcpyDeviceToDevice, st)); return; }
    const FormantTable &t = formant_table_dev(e, (int)g.o, (int)g.n);
    for (int per_thread = 4; per_thread >= 1; per_thread >>= 1) {
        const RswTile tl = rsw_tile(t.o, t.n, (int)g.K, t.Kt, per_thread);
        if (tl.floats() > RSW_LDS_FLOATS) continue;
        const size_t wgs = (g.n_out + tl.tile - 1) / tl.tile;
        if (wgs > 0x7fffffffu) throw ShapeError("resample: signal too long");
        hipLaunchKernelGGL(resample_whole_lds_kernel, dim3((unsigned)wgs), dim3(RSW_THREADS), tl.floats() * sizeof(float), st, d_x, (long long)n_in, (const float *)t.tab,
                           (const int *)t.kb, t.o, t.n, t.w, t.Kt, tl.tile, tl.rows, tl.Ks, tl.span, d_y, (long long)g.n_out);
        return;
    }
    const size_t wgs = (g.n_out + RSW_THREADS - 1) / RSW_THREADS;
    if (wgs > 0x7fffffffu) throw ShapeError("resample: signal too long");
    hipLaunchKernelGGL(resample_whole_direct_kernel, dim3((unsigned)wgs), dim3(RSW_THREADS), 0, st, d_x, (long long)n_in, (const float *)t.tab, (const int *)t.kb, t.o, t.n, t.w,
                       t.Kt, d_y, (long long)g.n_out);
}

// arguments of rvc_resample / rvc_resample_device in the order the header documents; fills the geometry and *n_out
static rvc_status resample_check(rvc_engine *e, const void *in, size_t n_in, size_t rate_in, size_t rate_out, const void *out, size_t cap, size_t *n_out, ResampleGeometry *g)
{
    if (const char *why = resample_geometry(rate_in, rate_out, n_in, g)) throw ShapeError(why);
    if (n_out) *n_out = g->n_out;
    if (cap < g->n_out) { e->err = "resample: output buffer too small"; return RVC_SHAPE; }
    if (!in || !out) throw ShapeError("resample: null buffer");
    return RVC_OK;
}

}  // namespace rvc

extern "C" {

// host only, pure: out = {o, n, w, N_out}
rvc_status rvc_resample_geometry(size_t rate_in, size_t rate_out, size_t n_in, size_t out[4])
{
    if (!out) return RVC_SHAPE;
    ResampleGeometry g;
    if (resample_geometry(rate_in, rate_out, n_in, &g)) return RVC_SHAPE;
    out[0] = g.o; out[1] = g.n; out[2] = g.w; out[3] = g.n_out;
    return RVC_OK;
}

rvc_status rvc_resample_device(rvc_engine *e, const void *d_in, size_t n_in, size_t rate_in, size_t rate_out, void *d_out, size_t cap, size_t *n_out)
{
    return guarded(e, [&]() {
        ResampleGeometry g;
        const rvc_status rc = resample_check(e, d_in, n_in, rate_in, rate_out, d_out, cap, n_out, &g);
        if (rc != RVC_OK) return rc;
        launch_resample_whole(e, (const float *)d_in, n_in, g, (float *)d_out);
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipGetLastError());
        return RVC_OK;
    });
}

rvc_status rvc_resample(rvc_engine *e, const float *in, size_t n_in, size_t rate_in, size_t rate_out, float *out, size_t cap, size_t *n_out)
{
    return guarded(e, [&]() {
        ResampleGeometry g;
        const rvc_status rc = resample_check(e, in, n_in, rate_in, rate_out, out, cap, n_out, &g);
        if (rc != RVC_OK) return rc;
        DevBuf<float> d_x, d_y;
        d_x.alloc(n_in); d_y.alloc(g.n_out);
        HIPCHK(hipMemcpyAsync(d_x.get(), in, n_in * sizeof(float), hipMemcpyHostToDevice, e->stream));
        launch_resample_whole(e, d_x.get(), n_in, g, d_y.get());
        HIPCHK(hipMemcpyAsync(out, d_y.get(), g.n_out * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipGetLastError());
        return RVC_OK;
    });
}

}  // extern "C"
