// fcpe.hip.h -- the kernels around FCPE's convolutions (torchfcpe's CFNaiveMelPE with conv_only; DESIGN.md section 23 has the definition): the padded copy of
// the log-mel, GroupNorm(4) + LeakyReLU, LayerNorm over channels (out of place: the layer's input is its residual), GLU + 31-tap depthwise convolution + SiLU,
// and the decoder (sigmoid, arg-max, the nine-bin average, the threshold and the 50 Hz floor).  The k = 3 / 1x1 convolutions and the classifier are
// implicit-GEMM launches of the planner; the mel front end is RMVPE's kernel on FCPE's tables (model_fcpe.hip, the one unit that includes this header).
#pragma once
#include <hip/hip_runtime.h>
#include "reduce.hip.h"

namespace rvc {

constexpr int FCPE_BINS = 360, FCPE_MELS = 128;
constexpr int FCPE_DW_K = 31, FCPE_DW_PAD = 15;        // the depthwise filter and its zero padding
constexpr int FCPE_DW_CH = 16, FCPE_DW_TT = 64;        // fcpe_glu_dw_silu_kernel: channels and frames per workgroup (four waves, four channels each, a lane per frame)
constexpr int FCPE_DW_ROW = FCPE_DW_TT + 2 * FCPE_DW_PAD;      // 94 floats per staged row: 16 rows = 6016 bytes of LDS
constexpr float FCPE_EPS = 1e-5f;

// mel [B][128][Tm] (the front end's contiguous rows) -> the first convolution's operand [B][128][ld] with its zero halo
static __global__ __launch_bounds__(256) void fcpe_mel_pad_kernel(const float *mel, int Tm, long long total, float *out, int o_ld, long long o_bs)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int t = (int)(idx % Tm), m = (int)((idx / Tm) % FCPE_MELS);
    const long long b = idx / ((long long)Tm * FCPE_MELS);
    out[b * o_bs + (long long)m * o_ld + t] = mel[idx];
}

struct FcpeGnP {
    const float *x; int x_ld; long long x_bs;      // [B][H][x_ld]
    float *y; int y_ld; long long y_bs;            // [B][H][y_ld] (the next convolution's operand: its halo is not written)
    const float *g, *b;                            // [H]
    int Cg, T;                                     // channels per group (H / 4), frames
    float slope;
};

// One workgroup = one group of one stream: mean, then the variance about it (two passes over the Cg x T values, both block sums of reduce.hip.h), then
// (x - mean) * rstd * g[c] + b[c] -> LeakyReLU.  Consecutive lanes are consecutive frames.
static __global__ __launch_bounds__(256) void fcpe_gn_lrelu_kernel(FcpeGnP p)
{
    __shared__ float red[16];
    const int grp = blockIdx.x, b = blockIdx.y, n = p.Cg * p.T;
    const float *x = p.x + (long long)b * p.x_bs + (long long)grp * p.Cg * p.x_ld;
    float *y = p.y + (long long)b * p.y_bs + (long long)grp * p.Cg * p.y_ld;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { const int c = i / p.T, t = i - c * p.T; s += x[(long long)c * p.x_ld + t]; }
    const float mean = block_sum(s, red) / (float)n;
    float ss = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { const int c = i / p.T, t = i - c * p.T; const float d = x[(long long)c * p.x_ld + t] - mean; ss += d * d; }
    const float rstd = 1.0f / sqrtf(block_sum(ss, red) / (float)n + FCPE_EPS);
    for (int i = threadIdx.x; i < n; i += 256) {
        const int c = i / p.T, t = i - c * p.T, ch = grp * p.Cg + c;
        const float v = (x[(long long)c * p.x_ld + t] - mean) * rstd * p.g[ch] + p.b[ch];
        y[(long long)c * p.y_ld + t] = v >= 0.f ? v : v * p.slope;
    }
}

struct FcpeLnP {
    const float *x; int x_ld; long long x_bs;      // [B][C][x_ld]
    float *y; int y_ld; long long y_bs;
    const float *g, *b;                            // [C]
    int C, T;
};

// LayerNorm over the channels of every frame, out of place.  One workgroup = 16 frames of one stream: thread (column = tid & 15, part = tid >> 4) takes the
// channels part, part + 16, ...; the 16 partial sums of a column meet in LDS.  Mean first, then the variance about it.
static __global__ __launch_bounds__(256) void fcpe_layernorm_kernel(FcpeLnP p)
{
    __shared__ float red[16][17];
    const int col = threadIdx.x & 15, part = threadIdx.x >> 4, t = blockIdx.x * 16 + col, b = blockIdx.y;
    const bool live = t < p.T;
    const float *x = p.x + (long long)b * p.x_bs + t;
    float s = 0.f;
    if (live) for (int c = part; c < p.C; c += 16) s += x[(long long)c * p.x_ld];
    red[part][col] = s;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) tot += red[i][col];
    const float mean = tot / (float)p.C;
    __syncthreads();
    float ss = 0.f;
    if (live) for (int c = part; c < p.C; c += 16) { const float d = x[(long long)c * p.x_ld] - mean; ss += d * d; }
    red[part][col] = ss;
    __syncthreads();
    tot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) tot += red[i][col];
    const float rstd = 1.0f / sqrtf(tot / (float)p.C + FCPE_EPS);
    if (!live) return;
    float *y = p.y + (long long)b * p.y_bs + t;
    for (int c = part; c < p.C; c += 16) y[(long long)c * p.y_ld] = (x[(long long)c * p.x_ld] - mean) * rstd * p.g[c] + p.b[c];
}

struct FcpeDwP {
    const float *z; int z_ld; long long z_bs;      // [B][2 I][z_ld]: the pointwise H -> 2 I output, value rows then gate rows
    float *y; int y_ld; long long y_bs;            // [B][I][y_ld]
    const float *w, *bias;                         // [I][31], [I]
    int I, T;
};

// Grid (I / 16, ceil(T / 64), B), 256 threads.  A workgroup stages GLU(z) = z[c] * sigmoid(z[I + c]) of its 16 channels over the frames
// [t0 - 15, t0 + 64 + 15) into LDS, zeros outside [0, T) -- a stream's own ends, never a neighbour's frames; a time tile re-reads its halo from z -- then wave w
// runs the 31 taps + bias + SiLU of channels 4 w .. 4 w + 3 out of LDS, a lane per frame (consecutive lanes read consecutive dwords: no bank conflict).
// y[c][t] = silu(bias[c] + sum_k w[c][k] glu[c][t + k - 15])
static __global__ __launch_bounds__(256) void fcpe_glu_dw_silu_kernel(FcpeDwP p)
{
    __shared__ float row[FCPE_DW_CH][FCPE_DW_ROW];
    const int c0 = blockIdx.x * FCPE_DW_CH, t0 = blockIdx.y * FCPE_DW_TT, b = blockIdx.z;
    const float *z = p.z + (long long)b * p.z_bs;
    for (int e = threadIdx.x; e < FCPE_DW_CH * FCPE_DW_ROW; e += 256) {
        const int cc = e / FCPE_DW_ROW, i = e - cc * FCPE_DW_ROW, q = t0 - FCPE_DW_PAD + i, c = c0 + cc;
        float v = 0.f;
        if (q >= 0 && q < p.T && c < p.I) {
            const float a = z[(long long)c * p.z_ld + q], g = z[(long long)(p.I + c) * p.z_ld + q];
            v = a * (1.0f / (1.0f + expf(-g)));
        }
        row[cc][i] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t = t0 + lane;
    if (t >= p.T) return;
#pragma unroll
    for (int j = 0; j < FCPE_DW_CH / 4; j++) {
        const int cc = wave * (FCPE_DW_CH / 4) + j, c = c0 + cc;
        if (c >= p.I) break;
        const float *w = p.w + (long long)c * FCPE_DW_K;
        float acc = p.bias[c];
#pragma unroll
        for (int k = 0; k < FCPE_DW_K; k++) acc += w[k] * row[cc][lane + k];
        p.y[(long long)b * p.y_bs + (long long)c * p.y_ld + t] = acc * (1.0f / (1.0f + expf(-acc)));
    }
}

struct FcpeDecP {
    const float *logit; int l_ld; long long l_bs;      // classifier output [B][360][l_ld], or null:
    const float *prob_in;                              // ... the caller's posteriors [B][Tm][360] (rvc_debug_fcpe_decode), taken as they are
    float *prob;                                       // [B][Tm][360] written when logit is set
    const float *f0tab;                                // [360] Hz of a bin's centre, rounded once from double
    float cent_step;                                   // cents between neighbouring bins
    double threshold;                                  // f0 = 0 where p[t][k*] <= threshold, compared in double: the decision the float64 definition makes on the same float
    int Tm;
    float *f0; int *bins;                              // [B][Tm]; bins may be null
};

// Grid (ceil(Tm / 4), B), 256 threads: a wave per frame, one barrier.  The frame's 360 posteriors go through LDS, so the value written is the value decided on; arg-max
// by a wave reduction on (-value, index), ties to the lower bin; lanes 0..8 take the nine clamped indices (a clamped index counts as often as it occurs).
// cents = c[k*] + sum p (c - c[k*]) / sum p -- the definition's average with the centre taken out, so float32 rounds offsets of at most 80 cents and not
// sums near 9000 -- and f0 = f0tab[k*] * 2^(offset / 1200).
static __global__ __launch_bounds__(256) void fcpe_decode_kernel(FcpeDecP p)
{
    __shared__ float pl[4][FCPE_BINS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t = blockIdx.x * 4 + wave, b = blockIdx.y;
    const bool live = t < p.Tm;
    const long long fo = ((long long)b * p.Tm + t) * FCPE_BINS;
    float best = INFINITY; int bi = 0;
    if (live)
        for (int i = lane; i < FCPE_BINS; i += 64) {
            float v;
            if (p.logit) { v = 1.0f / (1.0f + expf(-p.logit[(long long)b * p.l_bs + (long long)i * p.l_ld + t])); p.prob[fo + i] = v; }
            else v = p.prob_in[fo + i];
            pl[wave][i] = v;
            if (-v < best) { best = -v; bi = i; }          // ascending i per lane: the lane's first maximum
        }
    __syncthreads();
    if (!live) return;
    wave_min_pair(best, bi);
    float ps = 0.f, ws = 0.f;
    if (lane < 9) {
        int k = bi - 4 + lane;
        k = k < 0 ? 0 : (k > FCPE_BINS - 1 ? FCPE_BINS - 1 : k);
        ws = pl[wave][k];
        ps = ws * ((float)(k - bi) * p.cent_step);
    }
    ps = wave_sum(ps); ws = wave_sum(ws);
    if (lane == 0) {
        float hz = p.f0tab[bi] * exp2f((ps / ws) * (1.0f / 1200.0f));
        if ((double)pl[wave][bi] <= p.threshold || !(hz >= 50.0f)) hz = 0.f;          // (a frame of zeros: 0 / 0, caught by either test)
        p.f0[(long long)b * p.Tm + t] = hz;
        if (p.bins) p.bins[(long long)b * p.Tm + t] = bi;
    }
}

}  // namespace rvc
