// rmvpe.hip.h -- the f0 branch's kernels around the RMVPE network: the mel front end, AvgPool2d, the GRU input transpose and the pitch tail (salience
// decode, pitch controls, pitch cache).  Included by model_rmvpe.hip only (the fused ConvBlockRes kernel: rmblock.hip.h).
#pragma once
#include "state.hip.h"
#include "f0cond.hip.h"
#include "reduce.hip.h"

namespace rvc {

// ------------------------------------------------------------------------------------
// RMVPE front end: reflect pad + periodic Hann + 1024-pt FFT + magnitude + mel + log
// (reference: rvc/src/f0/rmvpe.rs:80-116, 159-205).  One workgroup per frame, everything
// LDS-resident; the mel reduction is a wavefront shuffle reduction.
// Output goes straight into the RMVPE input image [1][Tm(+halo)][128(+halo)] with the
// network's input BatchNorm affine applied; the raw log-mel is kept for taps.
// ------------------------------------------------------------------------------------
struct MelP {
    const float *audio;     // [B][n] 16 kHz input (device)
    long long audio_bs;
    int n;                  // samples per stream
    int frame;              // f0_extractor_frame: the last `frame` samples are analysed
    int Tm;
    const float *window;    // [1024]
    const float *twiddle;   // [512][2] cos,sin of -2*pi*j/1024
    const float *basis;     // [128][513]
    const int *band;        // [128][2] first / one-past-last non-zero bin of each mel filter
    float *mel;             // [B][128][Tm] raw log-mel (tap / parity)
    float *img;             // RMVPE input image interior pointer
    long long img_bs; int img_ld;
    float bn_scale, bn_shift;
};

// One workgroup = one frame.  rmvpe.rs:159-205 restated for the GPU: reflect pad + periodic Hann while loading, a 1024-point
// complex FFT as five radix-4 Stockham passes (every thread owns one 4-point butterfly per pass; ping-pong in LDS, five barriers
// instead of the ten of a radix-2 pass structure), magnitudes of the 513 kept bins, then the mel projection as WAVEFRONT-SHUFFLE
// reductions: a 16-lane group per filter strides over the filter's non-zero band and folds its partial sums with four xor-shuffles
// (four filters per wave at a time, 128 filters over the four waves), log, and the RMVPE input affine.
__device__ __forceinline__ void tw1024(const float *tw, int e, float &c, float &s)
{
    // W^e = exp(-2 pi i e / 1024) from the half table (e < 512); W^(e + 512) = -W^e
    const int h = e & 511;
    c = tw[2 * h]; s = tw[2 * h + 1];
    if (e & 512) { c = -c; s = -s; }
}
static __global__ __launch_bounds__(256) void mel_frontend_kernel(MelP p)
{
    __shared__ float bufr[2][1024], bufi[2][1024];
    __shared__ float mag[516];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float *sig = p.audio + (long long)b * p.audio_bs + (p.n - p.frame);
    const int L = p.frame;
    const int lane = tid & 63, wave = tid >> 6, sub = lane >> 4, l16 = lane & 15;
    // Round 6: EVERY table value this thread will need is requested here, next to the signal -- its twelve twiddles (they depend on tid only), the bands of its eight
    // mel filters and, behind those, the first four basis values per filter.  The tables are cold at every chunk (853 MB of weights pass between two uses) and
    // were read where they were needed: a memory round trip in front of each of four FFT passes and two per mel filter group -- most of the kernel's 20 us, which is
    // the head of the f0 branch, the critical path of the chunk's front.  Same arithmetic in the same order.
    float sg[4], wn[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int j = tid + r * 256;
        int q = t * 160 + j - 512;            // index into the unpadded signal
        if (q < 0) q = -q;                     // left reflect: padded[512-i-1] = sig[i+1]
        if (q >= L) q = 2 * L - 2 - q;         // right reflect: padded[L+512+i] = sig[L-i-2]
        sg[r] = sig[q]; wn[r] = p.window[j];
    }
    float twc[4][3], tws[4][3];                // passes Ns = 4, 16, 64, 256; r = 1..3
    {
        int pi = 0;
#pragma unroll
        for (int Ns = 4; Ns < 1024; Ns *= 4, pi++) {
            const int estep = (tid & (Ns - 1)) * (256 / Ns);
#pragma unroll
            for (int r = 1; r < 4; r++) tw1024(p.twiddle, estep * r, twc[pi][r - 1], tws[pi][r - 1]);
        }
    }
    int blo[8], bhi[8];
#pragma unroll
    for (int it = 0; it < 8; it++) { const int m = wave * 32 + it * 4 + sub; blo[it] = p.band[2 * m]; bhi[it] = p.band[2 * m + 1]; }
    float bpre[8][4];
#pragma unroll
    for (int it = 0; it < 8; it++) {
        const float *br = p.basis + (wave * 32 + it * 4 + sub) * 513;
#pragma unroll
        for (int j = 0; j < 4; j++) { const int k = blo[it] + l16 + 16 * j; bpre[it][j] = k < bhi[it] ? br[k] : 0.f; }
    }
    // frame t covers padded[t*160 .. t*160+1024), padded = reflect(sig, 512); natural order (the Stockham passes sort as they go)
#pragma unroll
    for (int r = 0; r < 4; r++) { const int j = tid + r * 256; bufr[0][j] = sg[r] * wn[r]; bufi[0][j] = 0.f; }
    __syncthreads();
    int cur = 0;
    int pass = -1;
#pragma unroll
    for (int Ns = 1; Ns < 1024; Ns *= 4, pass++) {
        const int k = tid & (Ns - 1);
        float vr[4], vi[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float xr = bufr[cur][tid + r * 256], xi = bufi[cur][tid + r * 256];
            if (r == 0 || Ns == 1) { vr[r] = xr; vi[r] = xi; }
            else { const float c = twc[Ns == 1 ? 0 : pass][r - 1], sn = tws[Ns == 1 ? 0 : pass][r - 1]; vr[r] = xr * c - xi * sn; vi[r] = xr * sn + xi * c; }
        }
        const float a0r = vr[0] + vr[2], a0i = vi[0] + vi[2], a1r = vr[0] - vr[2], a1i = vi[0] - vi[2];
        const float a2r = vr[1] + vr[3], a2i = vi[1] + vi[3];
        const float a3r = vi[1] - vi[3], a3i = -(vr[1] - vr[3]);     // (v1 - v3) * (-i)
        const int j0 = (tid / Ns) * Ns * 4 + k;
        float *orr = bufr[cur ^ 1], *oi = bufi[cur ^ 1];
        orr[j0] = a0r + a2r;          oi[j0] = a0i + a2i;
        orr[j0 + Ns] = a1r + a3r;     oi[j0 + Ns] = a1i + a3i;
        orr[j0 + 2 * Ns] = a0r - a2r; oi[j0 + 2 * Ns] = a0i - a2i;
        orr[j0 + 3 * Ns] = a1r - a3r; oi[j0 + 3 * Ns] = a1i - a3i;
        cur ^= 1;
        __syncthreads();
    }
    for (int k = tid; k < 513; k += 256) { const float xr = bufr[cur][k], xi = bufi[cur][k]; mag[k] = sqrtf(xr * xr + xi * xi); }
    __syncthreads();
    // mel projection: filter m = wave * 32 + it * 4 + (lane >> 4); its 16 lanes stride over the band [lo, hi), xor-shuffle fold
#pragma unroll
    for (int it = 0; it < 8; it++) {
        const int m = wave * 32 + it * 4 + sub;
        const int lo = blo[it], hi = bhi[it];
        const float *br = p.basis + m * 513;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; j++) { const int k = lo + l16 + 16 * j; if (k < hi) s += bpre[it][j] * mag[k]; }
        for (int k = lo + l16 + 64; k < hi; k += 16) s += br[k] * mag[k];          // (bands wider than 64 bins: none at 16 kHz / 1024 points)
        s += __shfl_xor(s, 8, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 1, 64);
        if (l16 == 0) {
            const float lm = logf(fmaxf(s, 1e-5f));
            p.mel[((long long)b * 128 + m) * p.Tm + t] = lm;
            p.img[(long long)b * p.img_bs + (long long)t * p.img_ld + m] = lm * p.bn_scale + p.bn_shift;
        }
    }
}

// AvgPool2d(2,2): x [B][C][H(+2)][ld] -> y [B][C][H/2(+2)][ld2]
static __global__ void avgpool2_kernel(const float *x, int x_ld, int x_cs, long long x_bs, float *y, int y_ld, int y_cs, long long y_bs, int C, int H2, int W2)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= C * H2 * W2) return;
    int c = i / (H2 * W2), r = i - c * H2 * W2, h = r / W2, w = r - h * W2;
    const float *s = x + (long long)b * x_bs + (long long)c * x_cs + (long long)(2 * h) * x_ld + 2 * w;
    y[(long long)b * y_bs + (long long)c * y_cs + (long long)h * y_ld + w] = (s[0] + s[1] + s[x_ld] + s[x_ld + 1]) * 0.25f;
}

// (3, Tm, n_mels) conv output image -> GRU input [B][3*n_mels][ld]: feat[c*n_mels + m][t] = img[c][t][m]
static __global__ void gru_input_kernel(const float *img, int i_ld, int i_cs, long long i_bs, float *feat, int f_cs, long long f_bs, int Tm, int n_mels)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= 3 * n_mels * Tm) return;
    int row = i / Tm, t = i - row * Tm, c = row / n_mels, m = row - c * n_mels;
    feat[(long long)b * f_bs + (long long)row * f_cs + t] = img[(long long)b * i_bs + (long long)c * i_cs + (long long)t * i_ld + m];
}

// RMVPE decode (rmvpe.rs:118-133, 243-248) + pitch shift (rvc.rs:121-122) + the stream's pitch controls (f0cond.hip.h) + pitch cache
// update and slice (rvc.rs:167-179) + get_f0_post (f0/mod.rs:7-12).  One workgroup per stream.
struct PitchP {
    const float *sal; int sal_cs; long long sal_bs;   // salience [B][360][ld] (channel-major)
    const float *f0_in;   // [B][Tm] f0 in Hz from another method (yin.hip.h): when set, the salience decode and its threshold are skipped and the tail below runs on it
    int Tm;
    StreamState *st; const CallParams *cp;
    float *f0;            // [B][Tm] (shifted f0, tap)
    float *pitchf;        // [B][R]
    int *pitch;           // [B][R]
    int shift, cache_start, read_start, R;
    float threshold;
    int update;           // 0: decode only (RvcInfer::pitch, rvc.rs:111-131), 1: also update + slice the cache (infer)
};

static __global__ __launch_bounds__(1024) void pitch_post_kernel(PitchP p)
{
    __shared__ float f0s[1024];
    __shared__ float cache[1024];
    __shared__ int idxs[1024];
    const int b = blockIdx.x, t = threadIdx.x;
    StreamState *st = p.st + b;
    const float up = st->ctl.uppower;        // per stream: every stream of a batch is its own caller with its own pitch shift (obs-rvc/src/lib.rs:701-707)
    // Row scan split over bin groups: thread (tt = t % TT, grp = t / TT) scans bins [grp*BPG, ...) of time step tt (loads
    // coalesced along time), then group 0 combines.  Same result as the sequential scan of the zero-padded row (368 wide,
    // "first strictly greater wins", padded[0] = 0): start = first index of the maximum if it is > 0, else 0.
    int TT = 1; while (TT < p.Tm) TT <<= 1;
    TT = TT < 1024 ? TT : 1024;
    const int NG = 1024 / TT, BPG = (360 + NG - 1) / NG, tt = t & (TT - 1), grp = t / TT;
    if (!p.f0_in) {
        float best = 0.f, mx = -INFINITY; int start = 0;
        if (tt < p.Tm) {
            const float *col = p.sal + (long long)b * p.sal_bs + tt;
            const int i0 = grp * BPG, i1 = (i0 + BPG < 360) ? i0 + BPG : 360;
#pragma unroll 4
            for (int i = i0; i < i1; i++) { const float v = col[(long long)i * p.sal_cs]; if (v > best) { best = v; start = i + 4; } mx = fmaxf(mx, v); }
        }
        f0s[t] = best; cache[t] = mx; idxs[t] = start;
    }
    __syncthreads();
    float hz_out = 0.f;
    if (grp == 0 && tt < p.Tm) {
        const float *col = p.sal + (long long)b * p.sal_bs + tt;
        int start = 0; float best = 0.f, mx = -INFINITY;
        for (int g = 0; g < (p.f0_in ? 0 : NG); g++) {
            const float v = f0s[g * TT + tt];
            if (v > best) { best = v; start = idxs[g * TT + tt]; }
            mx = fmaxf(mx, cache[g * TT + tt]);
        }
        float hz = 0.f;
        if (p.f0_in) hz = p.f0_in[(long long)b * p.Tm + tt];
        else if (start + 8 >= 360) { atomicOr(&st->status, (int)ST_PANIC); }
        else {
            float sv[9];
#pragma unroll
            for (int y = 0; y < 9; y++) sv[y] = col[(long long)(start + y) * p.sal_cs];
            float ps = 0.f, ws = 0.f;
#pragma unroll
            for (int y = 0; y < 9; y++) { const float cm = ((float)(start + y) - 4.f) * 20.f + 1997.3794084376191f; ps += sv[y] * cm; ws += sv[y]; }
            float cents = ps / ws;
            if (!(mx > p.threshold)) cents = 0.f;
            hz = 10.0f * powf(2.0f, cents / 1200.0f);
            if (hz == 10.0f) hz = 0.f;
        }
        hz *= up;
        hz_out = hz;
    }
    __syncthreads();
    // pitch controls (f0cond.hip.h): gate, median and scale snap on the multiplied rows, for either f0 method and for update = 0; a stream with every
    // control neutral (ctl.c.on == 0, uniform over the workgroup) passes with this one load
    const uint32_t con = st->ctl.c.on;
    if (con) {
        const float lo = st->ctl.c.lo, hi = st->ctl.c.hi, strength = st->ctl.c.strength;
        if (grp == 0 && tt < p.Tm) f0s[tt] = f0cond_gate(hz_out, con, lo, hi);
        __syncthreads();
        if (grp == 0 && tt < p.Tm) hz_out = f0cond_row(f0s, p.Tm, tt, con, strength);     // (kept in the register across the barrier: the neighbours still read f0s[])
        __syncthreads();
    }
    if (grp == 0 && tt < p.Tm) { f0s[tt] = hz_out; p.f0[(long long)b * p.Tm + tt] = hz_out; }
    if (!p.update) return;
    __syncthreads();
    cache[t] = st->cache_pitchf[t];
    __syncthreads();
    // copy_within(shift.., 0): cache[i] = cache[i+shift] for i < 1024-shift (tail keeps old values)
    float v = (t + p.shift < 1024) ? cache[t + p.shift] : cache[t];
    // cache[cache_start..] = pitchf[3..len-1]
    if (t >= p.cache_start) v = f0s[3 + (t - p.cache_start)];
    __syncthreads();
    cache[t] = v;
    st->cache_pitchf[t] = v;
    __syncthreads();
    if (t < p.R) {
        float f = cache[p.read_start + t];
        p.pitchf[(long long)b * p.R + t] = f;
        const float mel_min = logf(50.0f / 700.0f + 1.f) * 1127.f, mel_max = logf(500.0f / 700.0f + 1.f) * 1127.f;
        float x = logf(f / 700.0f + 1.f) * 1127.f;
        if (!(x <= 0.f)) x = (x - mel_min) * 254.f / (mel_max - mel_min) + 1.f;
        x = fminf(fmaxf(x, 1.f), 255.f);
        p.pitch[(long long)b * p.R + t] = (int)roundf(x);
    }
}

}  // namespace rvc
