// synth.hip.h -- the synthesizer's kernels besides its convolutions: pitch embedding, prior sampling, channel flip, the ResBlock mean, the NSF harmonic
// source and the two kernels of the formant stage (geometry and filter tables: formant.hip.h).  Included by model_synth.hip only.
#pragma once
#include "state.hip.h"
#include "reduce.hip.h"

namespace rvc {

// TextEncoder front: x = lrelu((lin + emb_pitch[pitch]) * sqrt(H), 0.1), in place on lin [B][H][ld]
static __global__ void embed_pitch_kernel(float *x, int cs, long long bs, const float *emb, const int *pitch, int H, int R, float sq)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= H * R) return;
    int c = i / R, t = i - c * R;
    float *xp = x + (long long)b * bs + (long long)c * cs + t;
    float a = *xp + emb[(long long)pitch[(long long)b * R + t] * H + c];
    a *= sq;
    *xp = a > 0.f ? a : a * 0.1f;
}

// ... of a model without pitch guidance (ModelSY::has_f0 false): x = lrelu(lin * sqrt(H), 0.1)
static __global__ void embed_nopitch_kernel(float *x, int cs, long long bs, int H, int R, float sq)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= H * R) return;
    int c = i / R, t = i - c * R;
    float *xp = x + (long long)b * bs + (long long)c * cs + t;
    float a = *xp * sq;
    *xp = a > 0.f ? a : a * 0.1f;
}

// Philox4x32-10, the same counter layout as oracle/rvc_oracle.c (ora_philox_normal)
// (philox4x32_10 / u01 / philox_normal4: state.hip.h)

// z_p = m + exp(logs) * eps * 0.66666 ; stats [B][2I][ld] -> z [B][I][ld]; eps index = c*T + t
static __global__ void prior_sample_kernel(const float *stats, int s_cs, long long s_bs, float *z, int z_cs, long long z_bs, int I, int T,
                                    const StreamState *st, const CallParams *cp)
{
    int blk = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    int total = I * T;
    if (blk * 4 >= total) return;
    float n4[4];
    philox_normal4(cp->seed, st[b].stream_id, st[b].chunk, 0u, (uint32_t)blk, n4);
    for (int j = 0; j < 4; j++) {
        int i = blk * 4 + j;
        if (i >= total) break;
        int c = i / T, t = i - c * T;
        float m = stats[(long long)b * s_bs + (long long)c * s_cs + t], lg = stats[(long long)b * s_bs + (long long)(I + c) * s_cs + t];
        z[(long long)b * z_bs + (long long)c * z_cs + t] = m + expf(lg) * n4[j] * 0.66666f;
    }
}

// channel flip (Flip flow): y[c] = x[C-1-c]
static __global__ void flip_channels_kernel(const float *x, int x_cs, long long x_bs, float *y, int y_cs, long long y_bs, int C, int T)
{
    // (source and destination have their own strides: with composed WaveNets the latent is a row range of a wider tensor -- a shared stride put every
    //  stream but the first in the wrong place: found in round 5 by the first multi-stream test of an odd flow count)
    int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= C * T) return;
    int c = i / T, t = i - c * T;
    y[(long long)b * y_bs + (long long)c * y_cs + t] = x[(long long)b * x_bs + (long long)(C - 1 - c) * x_cs + t];
}

// average of up to three ResBlock outputs: y = ((a + b) + c) * inv
static __global__ void mean3_kernel(const float *a, const float *b2, const float *c, int i_cs, long long i_bs, float *y, int y_cs, long long y_bs, int C, int T, float inv)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= C * T) return;
    int ch = i / T, t = i - ch * T;
    const long long o = (long long)b * i_bs + (long long)ch * i_cs + t;
    float v = a[o];
    if (b2) v += b2[o];
    if (c) v += c[o];
    y[(long long)b * y_bs + (long long)ch * y_cs + t] = v * inv;
}

// ------------------------------------------------------------------------------------
// NSF harmonic source (SineGen, harmonic_num = 0, + Linear(1,1) + tanh).  One workgroup of
// 1024 threads per stream; the sample-rate phase cumsum is a block prefix scan.
// ------------------------------------------------------------------------------------
struct SrcP {
    const float *pitchf;   // [B][T]
    float *src;            // [B][1][ld] interior pointer
    long long src_bs;
    int T, upp; float sr;
    float lin_w, lin_b;
    const StreamState *st; const CallParams *cp;
    int f0_num, f0_den;    // formant shift: the source reads f0 x f0_num / f0_den in fp32 (R2 / R, formant.hip.h); equal: f0 as it is
};

static __global__ __launch_bounds__(1024) void nsf_source_kernel(SrcP p)
{
    __shared__ float rad[512], cum[512];
    __shared__ float part[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = p.T, upp = p.upp;
    const long long N = (long long)T * upp;
    const float *f0 = p.pitchf + (long long)b * T;
    if (tid == 0) {
        float c = 0.f;
        const bool scale = p.f0_num != p.f0_den;
        for (int t = 0; t < T; t++) {
            const float f = scale ? (f0[t] * (float)p.f0_num) / (float)p.f0_den : f0[t];
            float r = fmodf(f / p.sr, 1.0f); rad[t] = r; c += r; cum[t] = c * (float)upp;
        }
    }
    __syncthreads();
    // each thread owns a contiguous segment whose length is a multiple of 4 (one Philox block = 4 samples)
    long long seg = ((N + 1023) / 1024 + 3) / 4 * 4;
    long long i0 = (long long)tid * seg, i1 = i0 + seg < N ? i0 + seg : N;
    auto interp = [&](long long i) -> float {
        float pos = (N > 1) ? (float)i * (float)(T - 1) / (float)(N - 1) : 0.f;
        int j0 = (int)floorf(pos); if (j0 > T - 1) j0 = T - 1; int j1 = j0 + 1 < T ? j0 + 1 : T - 1;
        float w = pos - (float)j0;
        float v = cum[j0] * (1.0f - w) + cum[j1] * w;
        return fmodf(v, 1.0f);
    };
    float local = 0.f;
    if (i0 < N) {
        float prev = i0 > 0 ? interp(i0 - 1) : 0.f;
        for (long long i = i0; i < i1; i++) {
            float cur = interp(i);
            float shift = (i > 0 && (cur - prev) < 0.f) ? -1.0f : 0.f;
            local += rad[(int)(i / upp)] + shift;
            prev = cur;
        }
    }
    part[tid] = local;
    __syncthreads();
    // inclusive scan over the 1024 partial sums (Hillis-Steele)
    for (int o = 1; o < 1024; o <<= 1) {
        float v = tid >= o ? part[tid - o] : 0.f;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    if (i0 < N) {
        float phase = tid > 0 ? part[tid - 1] : 0.f;
        float prev = i0 > 0 ? interp(i0 - 1) : 0.f;
        float *out = p.src + (long long)b * p.src_bs;
        const uint32_t seed = p.cp->seed, sid = p.st[b].stream_id, chunk = p.st[b].chunk;
        float nz[4];
        for (long long i = i0; i < i1; i++) {
            if (((i - i0) & 3) == 0) philox_normal4(seed, sid, chunk, 1u, (uint32_t)(i >> 2), nz);
            float cur = interp(i);
            float shift = (i > 0 && (cur - prev) < 0.f) ? -1.0f : 0.f;
            int t = (int)(i / upp);
            phase += rad[t] + shift;
            prev = cur;
            float sine = sinf(phase * 6.28318530717958647692f) * 0.1f;
            float uv = f0[t] > 0.f ? 1.f : 0.f;
            float namp = uv * 0.003f + (1.f - uv) * 0.1f / 3.f;
            float sw = sine * uv + namp * nz[(i - i0) & 3];
            out[i] = tanhf(p.lin_w * sw + p.lin_b);
        }
    }
}

// y[b][c][0:Nout] = linear interpolation of x[b][c][0:Nin] (torch.nn.functional.interpolate, mode "linear", align_corners=False)
static __global__ __launch_bounds__(256) void time_lerp_kernel(const float *x, int xld, long long xbs, float *y, int yld, long long ybs, int C, int Nin, int Nout)
{
    const int b = blockIdx.y;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)C * Nout) return;
    const int c = (int)(idx / Nout), i = (int)(idx - (long long)c * Nout);
    const float s = (float)Nin / (float)Nout;
    const float xs = fmaxf(__fmul_rn(s, (float)i + 0.5f) - 0.5f, 0.f);
    const int i0 = min((int)xs, Nin - 1), i1 = i0 + (i0 < Nin - 1 ? 1 : 0);
    const float l = fminf(fmaxf(xs - (float)i0, 0.f), 1.f);
    const float *row = x + (long long)b * xbs + (long long)c * xld;
    y[(long long)b * ybs + (long long)c * yld + i] = __fmul_rn(1.f - l, row[i0]) + __fmul_rn(l, row[i1]);
}

// Back to the model rate, per stream from its descriptor (StreamState::ctl.f, so that the streams of one plan may differ and a captured
// graph stays valid when the shift changes): y[q n + j] = sum_t ht[j][t] x[q o + kb[j] + t - w], x = y2[0 : nx] and zero outside;
// an identity stream (upp_res = upp) copies y2[0 : N].  One thread per output sample.
static __global__ __launch_bounds__(256) void formant_resample_kernel(const float *x, long long xbs, float *y, long long ybs, int N, const StreamState *st)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const StreamState &s = st[b];
    const float *row = x + (long long)b * xbs;
    float *out = y + (long long)b * ybs;
    if (s.ctl.f.ident) { out[i] = row[i]; return; }
    const int n = s.ctl.f.n, q = i / n, j = i - q * n, Kt = s.ctl.f.kt, nx = s.ctl.f.nx;
    const float *h = s.ctl.f.tab + (long long)j * Kt;
    const int base = q * s.ctl.f.o + s.ctl.f.kb[j] - s.ctl.f.w;
    float acc = 0.f;
    for (int t = 0; t < Kt; t++) {
        const int k = base + t;
        const float v = (k >= 0 && k < nx) ? row[k] : 0.f;
        acc = fmaf(h[t], v, acc);
    }
    out[i] = acc;
}

}  // namespace rvc
