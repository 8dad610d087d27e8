// crepe.hip.h -- the kernels around CREPE's convolutions (Kim et al. 2018; DESIGN.md section 21 has the definition): frame normalisation, ReLU -> BatchNorm ->
// max-pool, the sigmoid behind the classifier, and the Viterbi / arg-max decoder with its two width-3 filters.  The convolutions and the classifier themselves
// are implicit-GEMM launches of the planner (model_crepe.hip, the one unit that includes this header).
#pragma once
#include <hip/hip_runtime.h>
#include "reduce.hip.h"

namespace rvc {

constexpr int CREPE_FRAME = 1024, CREPE_HOP = 160, CREPE_PAD = 512, CREPE_BINS = 360;
constexpr int CREPE_LO = 39, CREPE_HI = 308;          // floor(bin(50 Hz)), ceil(bin(1100 Hz)), bin(f) = (1200 log2(f / 10) - 1997.3794084376191) / 20: bins [LO, HI) are decoded
constexpr int CREPE_BAND = 11;                         // the transition max(12 - |i - j|, 0) is positive for |i - j| <= 11: 23 predecessors per state
constexpr float CREPE_VOICED = 0.1f;                   // f0 = 0 where the filtered periodicity is below this
constexpr int CREPE_DEC_THREADS = 384;                 // six waves: one state per thread, 24 idle
constexpr int CREPE_BP_LDS_FRAMES = 128;               // back-pointers of up to this many frames stay in LDS (45 KB); longer windows keep them in the plan arena

struct CrepeFrameP {
    const float *audio;     // [B][n] 16 kHz input (device)
    long long audio_bs;
    int n, frame, Tm;       // samples per stream; the last `frame` of them are analysed as Tm frames
    float *out;             // frame b * Tm + t at out + (b * Tm + t) * out_fs (the layer-1 operand: one channel, zero halo around it)
    long long out_fs;
};

// One workgroup = one frame of one stream: the 1024 samples centred on sample 160 t (zeros outside the window), minus their mean, over max(1e-10, std), std with
// the unbiased (N - 1) estimator.  Four samples per thread stay in registers between the two block sums.
static __global__ __launch_bounds__(256) void crepe_frame_kernel(CrepeFrameP p)
{
    __shared__ float red[16];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float *sig = p.audio + (long long)b * p.audio_bs + (p.n - p.frame);
    float v[4], s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int q = t * CREPE_HOP + tid + 256 * i - CREPE_PAD;
        v[i] = (q >= 0 && q < p.frame) ? sig[q] : 0.f;
        s += v[i];
    }
    const float mean = block_sum(s, red) * (1.0f / CREPE_FRAME);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) { v[i] -= mean; ss += v[i] * v[i]; }
    const float sd = fmaxf(1e-10f, sqrtf(block_sum(ss, red) / (float)(CREPE_FRAME - 1)));
    float *o = p.out + ((long long)b * p.Tm + t) * p.out_fs;
#pragma unroll
    for (int i = 0; i < 4; i++) o[tid + 256 * i] = v[i] / sd;
}

struct CrepePoolP {
    const float *y;         // conv + bias of one layer: [frames][C][y_ld]
    int y_ld; long long y_bs;
    int C, L;               // channels, POOLED length (the conv output has 2 L columns)
    long long total;        // frames * C * L
    const float *scale, *shift;      // BatchNorm in inference form, per channel
    float *out;
    // cls = 0: the next layer's padded buffer, out + frame * o_bs + c * o_ld + l (the halo around the L columns is never written and stays zero);
    // cls = 1: the classifier's operand [B][L * C][o_ld], row l * C + c (time major, channel minor), column = frame within the stream (Tm of them)
    int o_ld; long long o_bs; int cls, Tm;
};

// ReLU -> scale, shift -> max over pairs, in that order: a scale may be negative, so the affine step does not commute with the pool
static __global__ __launch_bounds__(256) void crepe_bn_pool_kernel(CrepePoolP p)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.total) return;
    const int l = (int)(idx % p.L), c = (int)((idx / p.L) % p.C);
    const long long f = idx / ((long long)p.L * p.C);
    const float *src = p.y + f * p.y_bs + (long long)c * p.y_ld + 2 * l;
    const float sc = p.scale[c], sh = p.shift[c];
    const float a = fmaxf(src[0], 0.f) * sc + sh, b = fmaxf(src[1], 0.f) * sc + sh;
    const float v = fmaxf(a, b);
    if (p.cls) {
        const long long s = f / p.Tm; const int t = (int)(f - s * p.Tm);
        p.out[s * p.o_bs + (long long)(l * p.C + c) * p.o_ld + t] = v;
    } else p.out[f * p.o_bs + (long long)c * p.o_ld + l] = v;
}

// classifier logits [B][360][ld] -> posteriors [B][Tm][360] (the decoder's layout: a frame's bins are contiguous)
static __global__ __launch_bounds__(256) void crepe_sigmoid_kernel(const float *logit, int ld, long long bs, int Tm, long long total, float *prob)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int i = (int)(idx % CREPE_BINS), t = (int)((idx / CREPE_BINS) % Tm);
    const long long b = idx / ((long long)CREPE_BINS * Tm);
    prob[idx] = 1.0f / (1.0f + expf(-logit[b * bs + (long long)i * ld + t]));
}

struct CrepeDecP {
    const float *prob;      // [B][Tm][360]
    int Tm, decoder;        // 0 = Viterbi, 1 = arg-max
    const float *f0tab;     // [360] Hz of a bin
    unsigned char *bp;      // [B][Tm][360] back-pointers for Tm > CREPE_BP_LDS_FRAMES, else unused
    float *f0;              // [B][Tm] filtered, thresholded
    int *bins; float *pd;   // [B][Tm] the path and its unfiltered periodicity p[t][bin[t]]; either may be null
};

// One workgroup = one stream.  Viterbi in the log domain over the bins [LO, HI) (the others are at -inf): the observation of state j at frame t is p[t][j] --
// the softmax of the definition takes a per-frame constant off every state, and so does the uniform prior, which no arg-max sees; the transition from i to j is
// log(12 - |i - j|) - log(row sum of i).  Thread j owns state j: the scores of frame t - 1, less their row's log sum, lie in LDS with 11 cells of -inf on
// either side, so the 23 predecessors are read without a bounds test (consecutive threads, consecutive dwords: no bank conflict); the two buffers alternate,
// one barrier per frame.  `>` over ascending i leaves ties with the lower bin.  A back-pointer is the byte d + 11.  Then thread 0 walks back, and the threads
// take a frame each for the periodicity, the median and mean of three (two at either end; the median of two is their mean) and the threshold.
static __global__ __launch_bounds__(CREPE_DEC_THREADS) void crepe_decode_kernel(CrepeDecP p)
{
    __shared__ float sc[2][CREPE_BINS + 2 * CREPE_BAND + 2];
    __shared__ unsigned char bpl[CREPE_BP_LDS_FRAMES * CREPE_BINS];
    __shared__ float pdl[1024], f0l[1024];
    __shared__ short binl[1024];
    __shared__ float lw[CREPE_BAND + 1], wmax[2][CREPE_DEC_THREADS / 64];
    const int j = threadIdx.x, b = blockIdx.x, Tm = p.Tm, lane = j & 63, wave = j >> 6;
    const float *prob = p.prob + (long long)b * Tm * CREPE_BINS;
    const bool state = j < CREPE_BINS, live = j >= CREPE_LO && j < CREPE_HI;
    if (p.decoder == 1) {
        // the same decoder without the transition term: every frame on its own, a wave per frame
        for (int t = wave; t < Tm; t += CREPE_DEC_THREADS / 64) {
            float best = INFINITY; int bi = CREPE_LO;
            for (int i = CREPE_LO + lane; i < CREPE_HI; i += 64) { const float v = -prob[(long long)t * CREPE_BINS + i]; if (v < best) { best = v; bi = i; } }
            wave_min_pair(best, bi);
            if (lane == 0) binl[t] = (short)bi;
        }
    } else {
        unsigned char *bp = Tm > CREPE_BP_LDS_FRAMES ? p.bp + (long long)b * Tm * CREPE_BINS : bpl;
        float lrs = 0.f;
        if (state) {
            int rs = 0;
            for (int d = -CREPE_BAND; d <= CREPE_BAND; d++) if (j + d >= 0 && j + d < CREPE_BINS) rs += CREPE_BAND + 1 - (d < 0 ? -d : d);
            lrs = logf((float)rs);
        }
        if (j <= CREPE_BAND) lw[j] = logf((float)(CREPE_BAND + 1 - j));
        for (int i = j; i < CREPE_BINS + 2 * CREPE_BAND + 2; i += CREPE_DEC_THREADS) { sc[0][i] = -INFINITY; sc[1][i] = -INFINITY; }
        __syncthreads();
        // scores are kept relative to the best score of the frame before (a constant per frame, which no arg-max sees): over 1024 frames the raw sums reach
        // thousands, where a float's spacing is 5e-4 and near-ties between paths are lost.  Every wave leaves its maximum in LDS in front of the frame's
        // barrier; the next frame's threads take the largest of the six
        float score = live ? prob[j] : -INFINITY;
        if (state) sc[0][CREPE_BAND + j] = score - lrs;
        { const float wm = wave_max(score); if (lane == 0) wmax[0][wave] = wm; }
        __syncthreads();
        int cur = 0;
        float obs_next = (state && Tm > 1) ? prob[CREPE_BINS + j] : 0.f;          // a frame's observation is loaded a frame ahead: in flight across the band loop and the barrier
        for (int t = 1; t < Tm; t++) {
            const float obs = obs_next;
            if (state && t + 1 < Tm) obs_next = prob[(long long)(t + 1) * CREPE_BINS + j];
            float m = wmax[cur][0];
#pragma unroll
            for (int w = 1; w < CREPE_DEC_THREADS / 64; w++) m = fmaxf(m, wmax[cur][w]);
            score = -INFINITY;
            if (state) {
                float best = -INFINITY; int bd = CREPE_BAND;
#pragma unroll
                for (int d = -CREPE_BAND; d <= CREPE_BAND; d++) {
                    const float v = sc[cur][CREPE_BAND + j + d] + lw[d < 0 ? -d : d];
                    if (v > best) { best = v; bd = d + CREPE_BAND; }
                }
                if (live) score = (best - m) + obs;
                sc[cur ^ 1][CREPE_BAND + j] = score - lrs;
                bp[(long long)t * CREPE_BINS + j] = (unsigned char)bd;
            }
            { const float wm = wave_max(score); if (lane == 0) wmax[cur ^ 1][wave] = wm; }
            cur ^= 1;
            __syncthreads();
        }
        // the best last state, ties to the lower bin: the raw scores through LDS, then wave 0
        if (state) sc[cur ^ 1][CREPE_BAND + j] = score;
        __syncthreads();
        if (wave == 0) {
            float best = INFINITY; int bi = CREPE_LO;
            for (int i = CREPE_LO + lane; i < CREPE_HI; i += 64) { const float v = -sc[cur ^ 1][CREPE_BAND + i]; if (v < best) { best = v; bi = i; } }
            wave_min_pair(best, bi);
            if (lane == 0) {
                binl[Tm - 1] = (short)bi;
                for (int t = Tm - 1; t > 0; t--) {
                    bi += (int)bp[(long long)t * CREPE_BINS + bi] - CREPE_BAND;
                    bi = bi < CREPE_LO ? CREPE_LO : (bi >= CREPE_HI ? CREPE_HI - 1 : bi);          // (a live state's predecessor is live: never taken)
                    binl[t - 1] = (short)bi;
                }
            }
        }
    }
    __syncthreads();
    for (int t = j; t < Tm; t += CREPE_DEC_THREADS) {
        const int bi = binl[t];
        pdl[t] = prob[(long long)t * CREPE_BINS + bi];
        f0l[t] = p.f0tab[bi];
    }
    __syncthreads();
    for (int t = j; t < Tm; t += CREPE_DEC_THREADS) {
        float pm, fm;
        if (Tm == 1) { pm = pdl[0]; fm = f0l[0]; }
        else if (t == 0 || t == Tm - 1) {
            const int u = t == 0 ? 1 : Tm - 2;
            pm = (pdl[t] + pdl[u]) * 0.5f; fm = (f0l[t] + f0l[u]) * 0.5f;
        } else {
            const float a = pdl[t - 1], c = pdl[t], d = pdl[t + 1];
            pm = fmaxf(fminf(a, c), fminf(fmaxf(a, c), d));
            fm = ((f0l[t - 1] + f0l[t]) + f0l[t + 1]) / 3.0f;
        }
        const long long o = (long long)b * Tm + t;
        p.f0[o] = pm < CREPE_VOICED ? 0.f : fm;
        if (p.bins) p.bins[o] = binl[t];
        if (p.pd) p.pd[o] = pdl[t];
    }
}

}  // namespace rvc
