// highpass.hip.h -- the file converter's 48 Hz high-pass: upstream filters every file it converts with a 5th-order Butterworth
// high-pass at 48 Hz run forwards and backwards; here the same job is a zero-phase FIR, 2 M + 1 taps with M = 1024, evaluated directly.  Included by
// engine.hip only.  Definition (fp64, then ONE rounding to fp32; highpass_taps below):
//   lp[j] = 2 fc sinc(2 fc (j - M)) (0.42 - 0.5 cos(2 pi j / 2M) + 0.08 cos(4 pi j / 2M)),  fc = 48 / 16000,  scaled to sum 1;   h = delta[j - M] - lp
//   y[i]  = sum_{j = 0 .. 2M} h[j] x[i + M - j],   x = 0 outside [0, n)
// No recursion, no state, output length n.  Each output is one fp32 fma chain over j = 0, 1, ..., 2M: the result does not depend on the launch shape.
#pragma once
#include "convert_geometry.h"

namespace rvc {

constexpr int HP_THREADS = 256, HP_PER_THREAD = 4, HP_TILE = HP_THREADS * HP_PER_THREAD;      // outputs per workgroup
constexpr int HP_TAPS = 2 * HP_M + 1;
constexpr size_t HP_LDS_BYTES = (size_t)(HP_TILE + 2 * HP_M + HP_TAPS) * sizeof(float);       // 20 KB: the tile's samples with both skirts, and the taps

// one workgroup = HP_TILE consecutive outputs; thread t owns outputs i0 + t + 256 k: consecutive lanes read consecutive LDS words, the tap is a broadcast
static __global__ __launch_bounds__(HP_THREADS) void highpass_fir_kernel(const float *x, long long n, const float *h, float *y)
{
    __shared__ float xs[HP_TILE + 2 * HP_M];
    __shared__ float hs[HP_TAPS];
    const long long i0 = (long long)blockIdx.x * HP_TILE;
    const int t = threadIdx.x;
    for (int q = t; q < HP_TILE + 2 * HP_M; q += HP_THREADS) {
        const long long src = i0 - HP_M + q;
        xs[q] = (src >= 0 && src < n) ? x[src] : 0.f;
    }
    for (int q = t; q < HP_TAPS; q += HP_THREADS) hs[q] = h[q];
    __syncthreads();
    float acc[HP_PER_THREAD];
#pragma unroll
    for (int k = 0; k < HP_PER_THREAD; k++) acc[k] = 0.f;
    // x[i + M - j] = xs[(i - i0) + 2 M - j]
    for (int j = 0; j < HP_TAPS; j++) {
        const float hj = hs[j];
#pragma unroll
        for (int k = 0; k < HP_PER_THREAD; k++) acc[k] = fmaf(hj, xs[t + HP_THREADS * k + 2 * HP_M - j], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < HP_PER_THREAD; k++) {
        const long long i = i0 + t + HP_THREADS * k;
        if (i < n) y[i] = acc[k];
    }
}

}  // namespace rvc
