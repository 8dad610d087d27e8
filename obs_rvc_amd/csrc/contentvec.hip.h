// contentvec.hip.h -- ContentVec's first layer (Conv1d + GroupNorm + GELU in one kernel, and the stand-alone GroupNorm + GELU).  Included by
// model_cv.hip only.
#pragma once
#include "igemm_common.hip.h"
#include "reduce.hip.h"

namespace rvc {

// ContentVec's first layer in one kernel: Conv1d(1 -> C, k taps, stride st, no bias) + GroupNorm(C groups = per channel over time) +
// GELU.  One workgroup per (channel, stream): the k weights live in registers, every thread computes its outputs from the raw 16 kHz
// ring (k fused multiply-adds each, in tap order -- the same f32 chain the matrix core runs) and KEEPS them in registers, the mean /
// variance go through two block reductions (two-pass, as the reference definition), and the normalised, activated row is written
// once.  HBM traffic = one write of the [C][T] row per stream instead of write + read + read + write (at 64 streams: 0.94 GB instead
// of 3.8 GB), and no implicit-GEMM launch with K = 16 for a 10-tap filter.
template <int NT>
__global__ __launch_bounds__(256) void conv0_gn_gelu_kernel(const float *audio, long long audio_bs, const float *w, int ktaps, int stride,
                                                            const float *g, const float *bta, float *y, int T, int y_cs, long long y_bs)
{
    __shared__ float red[16];
    const int c = blockIdx.x, b = blockIdx.y;
    const float *xin = audio + (long long)b * audio_bs;
    float wk[16];
#pragma unroll
    for (int k = 0; k < 16; k++) wk[k] = k < ktaps ? w[c * ktaps + k] : 0.f;
    float v[NT];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NT; i++) {
        const int t = threadIdx.x + i * 256;
        float a = 0.f;
        if (t < T) {
            const float *xp = xin + (long long)t * stride;
#pragma unroll
            for (int k = 0; k < 16; k++) if (k < ktaps) a = fmaf(wk[k], xp[k], a);
            s += a;
        }
        v[i] = a;
    }
    const float mean = block_sum(s, red) / (float)T;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NT; i++) { if ((int)threadIdx.x + i * 256 < T) { const float d = v[i] - mean; q += d * d; } }
    const float var = block_sum(q, red) / (float)T;
    const float inv = 1.0f / sqrtf(var + 1e-5f), gg = g[c], bb = bta[c];
    float *r = y + (long long)b * y_bs + (long long)c * y_cs;
#pragma unroll
    for (int i = 0; i < NT; i++) {
        const int t = threadIdx.x + i * 256;
        if (t < T) r[t] = apply_act((v[i] - mean) * inv * gg + bb, ACT_GELU, 0.f);
    }
}


// The same for `cpw` consecutive channels per workgroup (many streams): a thread's NT x KT input samples are loaded ONCE into
// registers (the stride-5 gathers are what the one-channel form spends its time on: 280 strided loads per thread and channel, 87 %
// of the wave cycles waiting) and reused for every channel; the k weights of a channel are wave-uniform.  1024 threads per workgroup
// keep the register copy at NT = ceil(T / 1024) samples per thread.  Same f32 chain per output as the one-channel kernel; the
// statistics are summed in a different grouping (1024 partial sums instead of 256), as every block-size choice does.
template <int NT, int KT>
__global__ __launch_bounds__(1024) void conv0_gn_gelu_multi_kernel(const float *audio, long long audio_bs, const float *w, int stride, const float *g,
                                                                   const float *bta, float *y, int T, int y_cs, long long y_bs, int cpw)
{
    __shared__ float red[16];
    const int b = blockIdx.y;
    const float *xin = audio + (long long)b * audio_bs;
    float xr[NT][KT];
#pragma unroll
    for (int i = 0; i < NT; i++) {
        const int t = threadIdx.x + i * 1024;
        const float *xp = xin + (long long)(t < T ? t : 0) * stride;
#pragma unroll
        for (int k = 0; k < KT; k++) xr[i][k] = xp[k];
    }
    for (int cc = 0; cc < cpw; cc++) {
        const int c = blockIdx.x * cpw + cc;
        float wk[KT];
#pragma unroll
        for (int k = 0; k < KT; k++) wk[k] = w[c * KT + k];
        float v[NT];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NT; i++) {
            float a = 0.f;
            if ((int)threadIdx.x + i * 1024 < T) {
#pragma unroll
                for (int k = 0; k < KT; k++) a = fmaf(wk[k], xr[i][k], a);
                s += a;
            }
            v[i] = a;
        }
        const float mean = block_sum(s, red) / (float)T;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NT; i++) { if ((int)threadIdx.x + i * 1024 < T) { const float d = v[i] - mean; q += d * d; } }
        const float var = block_sum(q, red) / (float)T;
        const float inv = 1.0f / sqrtf(var + 1e-5f), gg = g[c], bb = bta[c];
        float *r = y + (long long)b * y_bs + (long long)c * y_cs;
#pragma unroll
        for (int i = 0; i < NT; i++) {
            const int t = threadIdx.x + i * 1024;
            if (t < T) r[t] = apply_act((v[i] - mean) * inv * gg + bb, ACT_GELU, 0.f);
        }
    }
}

// GroupNorm with one group per channel (= per-channel normalisation over time) + GELU, in place.
static __global__ __launch_bounds__(256) void groupnorm_gelu_kernel(float *x, const float *g, const float *bta, int T, int cs, long long bs)
{
    __shared__ float red[16];
    const int c = blockIdx.x, b = blockIdx.y;
    float *r = x + (long long)b * bs + (long long)c * cs;
    float s = 0.f;
    for (int t = threadIdx.x; t < T; t += 256) s += r[t];
    const float mean = block_sum(s, red) / (float)T;
    float v = 0.f;
    for (int t = threadIdx.x; t < T; t += 256) { float d = r[t] - mean; v += d * d; }
    const float var = block_sum(v, red) / (float)T;
    const float inv = 1.0f / sqrtf(var + 1e-5f), gg = g[c], bb = bta[c];
    for (int t = threadIdx.x; t < T; t += 256) r[t] = apply_act((r[t] - mean) * inv * gg + bb, ACT_GELU, 0.f);
}

}  // namespace rvc
