// change_rms.hip.h -- the whole-file volume envelope (upstream's rms_mix_rate / change_rms, restated there -- unpinned against upstream),
// included by engine.hip.  Not rvc_envelop_mixing, the plugin's streaming form (align-corners interpolation, a floor of 1e-3, frames of 4 zc).
// For signal s in {1 = source at rate sr_1, 2 = converted at rate sr_2} (resample_geometry.h: change_rms_geometry):
//   L_s = 2 (sr_s / 2), hop_s = sr_s / 2, F_s = 1 + N_s / hop_s;  r_s[f] = sqrt(mean(xpad[f hop_s .. f hop_s + L_s)^2)), xpad = the signal zero-padded by L_s / 2
//   R_s[i], i < N_2: r_s brought to N_2 points by linear interpolation with half-pixel centres (F.interpolate(mode = "linear", align_corners = False)):
//       u = max((i + 0.5) F_s / N_2 - 0.5, 0), i0 = floor(u), i1 = min(i0 + 1, F_s - 1), R_s[i] = r_s[i0] (1 - (u - i0)) + r_s[i1] (u - i0)
//   out[i] = y[i] R_1[i]^(1 - rate) max(R_2[i], 1e-6)^(rate - 1)
// The RMS tracks are post_rms_kernel's (chunk.hip.h: fp64 from the fp32 samples); the product is evaluated in fp64 and rounded once at the store.
// rate = 1 launches nothing.
#pragma once
#include "resample_geometry.h"

namespace rvc {

__device__ __forceinline__ double lerp_half_pixel_at(const double *r, int F, long long size, long long i)
{
    double u = ((double)i + 0.5) * (double)F / (double)size - 0.5;
    u = u < 0.0 ? 0.0 : u;
    int i0 = (int)floor(u);
    i0 = i0 > F - 1 ? F - 1 : i0;
    const int i1 = i0 + 1 > F - 1 ? F - 1 : i0 + 1;
    const double fr = u - (double)i0;
    return r[i0] * (1.0 - fr) + r[i1] * fr;
}

static __global__ __launch_bounds__(256) void change_rms_apply_kernel(float *y, long long n, const double *r1, int F1, const double *r2, int F2, double rate)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double a = lerp_half_pixel_at(r1, F1, n, i);
    const double b = fmax(lerp_half_pixel_at(r2, F2, n, i), 1e-6);
    y[i] = (float)((double)y[i] * pow(a, 1.0 - rate) * pow(b, rate - 1.0));
}

// arguments of rvc_change_rms in the order the header documents
static void change_rms_check(size_t n_src, size_t rate_src, size_t n_y, size_t rate_y, double rate, RmsGeometry *g1, RmsGeometry *g2)
{
    if (!change_rms_rate_ok(rate)) throw ShapeError("change_rms: the mix rate is outside [0, 1]");
    if (const char *why = change_rms_geometry(n_src, rate_src, g1)) throw ShapeError(why);
    if (const char *why = change_rms_geometry(n_y, rate_y, g2)) throw ShapeError(why);
}

// d_y [n_y] rewritten in place from the envelope of d_src [n_src], queued on the engine's stream; `tracks` (r_1 then r_2) must outlive the launches
static void launch_change_rms(rvc_engine *e, const float *d_src, size_t n_src, const RmsGeometry &g1, float *d_y, size_t n_y, const RmsGeometry &g2, double rate,
                              DevBuf<double> &tracks)
{
    if (rate == 1.0) return;
    hipStream_t st = e->stream;
    tracks.alloc(g1.F + g2.F);
    double *r1 = tracks.get(), *r2 = r1 + g1.F;
    launch_post_rms(st, 1, d_src, (int)n_src, (int)g1.L, (int)g1.hop, (int)g1.F, r1, 0, 0);
    launch_post_rms(st, 1, d_y, (int)n_y, (int)g2.L, (int)g2.hop, (int)g2.F, r2, 0, 0);
    hipLaunchKernelGGL(change_rms_apply_kernel, dim3((unsigned)((n_y + 255) / 256)), dim3(256), 0, st, d_y, (long long)n_y, (const double *)r1, (int)g1.F, (const double *)r2,
                       (int)g2.F, rate);
}

}  // namespace rvc

extern "C" {

// y [n_y] at rate_y is rewritten in place; src [n_src] at rate_src is the signal whose envelope it takes on
rvc_status rvc_change_rms(rvc_engine *e, const float *src, size_t n_src, size_t rate_src, float *y, size_t n_y, size_t rate_y, double rate)
{
    return guarded(e, [&]() {
        RmsGeometry g1, g2;
        change_rms_check(n_src, rate_src, n_y, rate_y, rate, &g1, &g2);
        if (!src || !y) throw ShapeError("change_rms: null buffer");
        if (rate == 1.0) return RVC_OK;
        DevBuf<float> d_src, d_y; DevBuf<double> tracks;
        d_src.alloc(n_src); d_y.alloc(n_y);
        HIPCHK(hipMemcpyAsync(d_src.get(), src, n_src * sizeof(float), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(d_y.get(), y, n_y * sizeof(float), hipMemcpyHostToDevice, e->stream));
        launch_change_rms(e, d_src.get(), n_src, g1, d_y.get(), n_y, g2, rate, tracks);
        HIPCHK(hipMemcpyAsync(y, d_y.get(), n_y * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipGetLastError());
        return RVC_OK;
    });
}

}  // extern "C"
