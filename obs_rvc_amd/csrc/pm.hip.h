// pm.hip.h -- "pm", Praat's autocorrelation pitch tracker (Boersma 1993; upstream RVC's f0_method pm = to_pitch_ac) as the engine's second weight-free f0
// method: DESIGN.md section 26 has the definition.  Three kernels: the stream's peak, the candidates of every frame, one Viterbi path per stream.
#pragma once
#include <hip/hip_runtime.h>
#include "reduce.hip.h"

namespace rvc {

constexpr int PM_FRAME = 1024, PM_HOP = 160, PM_PAD = 512;          // YIN's frames (yin.hip.h), unchanged
constexpr int PM_W = 960, PM_OFF = 32;                              // the analysis window: three periods of the 50 Hz floor, centred in the frame
constexpr int PM_NLAG = 353, PM_ILO = 14, PM_IHI = 321, PM_D = 30;  // lags computed 0 .. 352, peak lags searched, sinc depth
constexpr int PM_MAXC = 14, PM_NC = PM_MAXC + 1;                    // voiced candidates per frame; with the unvoiced one in front
constexpr float PM_FLOOR = 50.f, PM_CEILING = 1100.f, PM_VT = 0.6f, PM_ST = 0.03f, PM_OC = 0.01f, PM_OJ = 0.35f, PM_VUV = 0.14f;
constexpr int PM_WAVES = 8, PM_THREADS = PM_WAVES * 64, PM_SEG = PM_W / PM_WAVES;          // one wave per 120 window positions
constexpr int PM_LPL = 7, PM_LANES = 51, PM_NL = PM_LPL * PM_LANES;                        // seven lags per lane, lanes 0 .. 50: lags 0 .. 356
constexpr int PM_AS = 1320;                                         // a[] and the zeros behind it (the highest index read is 956 + 350 + 9)
constexpr int PM_PEAKS = 160;                                       // (at most 154 local maxima among 308 lags)
constexpr int PM_CHUNK = 64;                                        // frames of candidates staged at a time by the path kernel
static_assert(PM_NL >= PM_NLAG && PM_SEG * PM_WAVES == PM_W && PM_SEG % 4 == 0 && PM_W - 4 + PM_LPL * (PM_LANES - 1) + PM_LPL + 2 < PM_AS, "pm_cand_kernel: lag layout");
static_assert(PM_IHI + PM_D < PM_NLAG && (PM_IHI - PM_ILO + 2) / 2 <= PM_PEAKS && 2 * PM_PEAKS <= PM_THREADS && PM_NLAG <= PM_THREADS, "pm_cand_kernel: peaks");

struct PmP {
    const float *audio;     // [B][n] 16 kHz input (device)
    long long audio_bs;
    int n;                  // samples per stream
    int frame;              // f0_extractor_frame: the last `frame` samples are analysed
    int Tm;
    const float *rw;        // [353] the window's normalised autocorrelation (pm_rw_table)
    float *gpk;             // [B][2] mean and peak |s - mean| of the stream's f0 window
    int *cn;                // [B][Tm] voiced candidates of the frame, 0 .. 14
    float *cf, *cs, *cd;    // [B][Tm][15] frequency, strength, local score; entry 0 is the unvoiced candidate, 1 .. n the voiced ones in ascending lag
    int *path;              // [B][Tm] the chosen candidate
    float *f0;              // [B][Tm] its frequency in Hz, 0 = unvoiced
};

// One workgroup = one stream: the mean of its f0 window and G = max |s - mean| (Praat takes the peak of the whole sound).
static __global__ __launch_bounds__(256) void pm_peak_kernel(PmP p)
{
    __shared__ float red[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *sig = p.audio + (long long)b * p.audio_bs + (p.n - p.frame);
    float s = 0.f;
    for (int j = tid; j < p.frame; j += 256) s += sig[j];
    const float mu = block_sum(s, red) / (float)p.frame;
    float g = 0.f;
    for (int j = tid; j < p.frame; j += 256) g = fmaxf(g, fabsf(sig[j] - mu));
    g = block_max(g, red);
    if (tid == 0) { p.gpk[2 * b] = mu; p.gpk[2 * b + 1] = g; }
}

// One workgroup = one frame of one stream.  The window w = frame[32 .. 992) goes to LDS, a[j] = (w[j] - mean) hanning[j] replaces it in place, zeros stand
// behind it.  ra(tau) = sum_j a[j] a[j + tau] for tau = 0 .. 356: lane l < 51 of EVERY wave owns the seven lags 7l .. 7l + 6 and wave w the window positions
// [120w, 120w + 120); the zeros make the bound j + tau < 960 of the sum.  For four positions j .. j+3 a lane needs a[j + 7l .. j + 7l + 9]: lanes are seven
// dwords apart, an odd stride, so a dword read is free of bank conflicts, and a[j .. j+3] is one address for the whole wave (a broadcast); six of the ten
// values stay in registers from the block before.  The eight partial sums per lag are folded pairwise, r = ra / (ra(0) rw) goes back to LDS.  Peaks: lag i
// is thread i's, a ballot per wave numbers them in lag order.  Two lanes per peak sum the 30 + 30 sinc taps; one lane per peak ranks it among the others
// and the best 14 are written in lag order.
static __global__ __launch_bounds__(PM_THREADS) void pm_cand_kernel(PmP p)
{
    __shared__ __attribute__((aligned(16))) float a[PM_AS];
    __shared__ float part[PM_WAVES][PM_NL];
    __shared__ float r[PM_NLAG];
    __shared__ float red[16];
    __shared__ int wcnt[PM_WAVES];
    __shared__ int pk_lag[PM_PEAKS];
    __shared__ float pk_off[PM_PEAKS], pk_f[PM_PEAKS], pk_s[PM_PEAKS], pk_score[PM_PEAKS];
    __shared__ unsigned char pk_keep[PM_PEAKS];
    __shared__ float s_ra0;
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *sig = p.audio + (long long)b * p.audio_bs + (p.n - p.frame);
    const int L = p.frame;
    // frame t covers padded[160 t .. 160 t + 1024), padded = reflect(sig, 512): the reflection is index arithmetic (yin_f0_kernel)
    for (int j = tid; j < PM_AS; j += PM_THREADS) {
        float v = 0.f;
        if (j < PM_W) {
            int q = t * PM_HOP + PM_OFF + j - PM_PAD;
            if (q < 0) q = -q;
            if (q >= L) q = 2 * L - 2 - q;
            v = sig[q];
        }
        a[j] = v;
    }
    __syncthreads();
    float ps = 0.f;
    for (int j = tid; j < PM_W; j += PM_THREADS) ps += a[j];
    const float mu = block_sum(ps, red) / (float)PM_W;
    float pm = 0.f;
    for (int j = 320 + tid; j < 640; j += PM_THREADS) pm = fmaxf(pm, fabsf(a[j] - mu));          // the central floor period
    pm = block_max(pm, red);
    const float G = p.gpk[2 * b + 1];
    const float inten = G > 0.f ? fminf(1.f, pm / G) : 0.f;
    for (int j = tid; j < PM_W; j += PM_THREADS) a[j] = (a[j] - mu) * (0.5f - 0.5f * cospif((float)(2 * j + 1) / (float)PM_W));
    __syncthreads();
    if (lane < PM_LANES) {
        const int j0 = wave * PM_SEG, o = PM_LPL * lane;
        float acc[PM_LPL];
        float y[PM_LPL + 3];
#pragma unroll
        for (int k = 0; k < PM_LPL; k++) acc[k] = 0.f;
#pragma unroll
        for (int k = 0; k < PM_LPL - 1; k++) y[k] = a[j0 + o + k];
#pragma unroll 2
        for (int j = j0; j < j0 + PM_SEG; j += 4) {
            const float4 xv = *reinterpret_cast<const float4 *>(&a[j]);
            const float x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
            for (int k = 0; k < 4; k++) y[PM_LPL - 1 + k] = a[j + o + PM_LPL - 1 + k];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int k = 0; k < PM_LPL; k++) acc[k] = fmaf(x4[i], y[i + k], acc[k]);
#pragma unroll
            for (int k = 0; k < PM_LPL - 1; k++) y[k] = y[4 + k];
        }
#pragma unroll
        for (int k = 0; k < PM_LPL; k++) part[wave][o + k] = acc[k];
    }
    __syncthreads();
    float ra = 0.f;
    if (tid < PM_NLAG) {
        ra = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) + ((part[4][tid] + part[5][tid]) + (part[6][tid] + part[7][tid]));
        if (tid == 0) s_ra0 = ra;
    }
    __syncthreads();
    const float ra0 = s_ra0;
    const bool live = G > 0.f && ra0 > 0.f;          // a silent stream or an all-zero frame has the unvoiced candidate only
    if (tid < PM_NLAG) r[tid] = live ? ra / (ra0 * p.rw[tid]) : 0.f;
    __syncthreads();
    // peaks: r[i] > VT / 2, above the left neighbour, not below the right one; the vertex of Praat's parabola; inside [floor, ceiling]
    bool pk = false;
    float off = 0.f, f = 0.f;
    if (live && tid >= PM_ILO && tid <= PM_IHI) {
        const float ra_ = r[tid - 1], rb = r[tid], rc = r[tid + 1];
        if (rb > 0.5f * PM_VT && rb > ra_ && rb >= rc) {
            off = 0.5f * (rc - ra_) / (2.f * rb - ra_ - rc);
            f = 16000.f / ((float)tid + off);
            pk = f >= PM_FLOOR && f <= PM_CEILING;
        }
    }
    const unsigned long long hit = __ballot(pk);
    if (lane == 0) wcnt[wave] = __popcll(hit);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < PM_WAVES; w++) { if (w < wave) base += wcnt[w]; total += wcnt[w]; }
    if (pk) {
        const int q = base + __popcll(hit & ((1ull << lane) - 1ull));
        pk_lag[q] = tid; pk_off[q] = off; pk_f[q] = f;
    }
    __syncthreads();
    // strength: Praat's raised-cosine windowed sinc interpolation of r at i + off, depth 30.  With m = floor(i + off) and phi the fraction,
    // sin(pi (tau - k)) = (-1)^(m - k) sin(pi phi); phi and 1 - phi come from off itself.  The even lane of a pair sums the taps m, m-1, ..., the odd lane m+1, ...
    {
        const int q = tid >> 1, side = tid & 1;
        float sum = 0.f;
        int i = 0;
        float o = 0.f;
        if (q < total) {
            i = pk_lag[q]; o = pk_off[q];
            if (o != 0.f) {
                const int m = o > 0.f ? i : i - 1;
                const float phi = o > 0.f ? o : 1.f + o, omphi = o > 0.f ? 1.f - o : -o;
                const float sp = sinpif(fminf(phi, omphi));
                const float d0 = side ? omphi : phi, den = d0 + (float)PM_D;
                const float pi = 3.14159265358979323846f;
                float sign = 1.f;
                for (int j = 0; j < PM_D; j++) {
                    const int k = side ? m + 1 + j : abs(m - j);
                    const float d = d0 + (float)j;
                    sum += r[k] * (sign * sp / (pi * d)) * (0.5f + 0.5f * cospif(d / den));
                    sign = -sign;
                }
            }
        }
        const float other = __shfl_xor(sum, 1, 64);
        if (q < total && side == 0) {
            float s = o != 0.f ? sum + other : r[i];
            if (s > 1.f) s = 1.f / s;
            pk_s[q] = s;
            pk_score[q] = s + PM_OC * log2f(pk_f[q] / PM_FLOOR);
        }
    }
    __syncthreads();
    // the 14 largest by score, ties to the smaller lag
    if (tid < total) {
        const float sc = pk_score[tid];
        int above = 0;
        for (int q = 0; q < total; q++) { const float v = pk_score[q]; above += (v > sc || (v == sc && q < tid)) ? 1 : 0; }
        pk_keep[tid] = above < PM_MAXC ? 1 : 0;
    }
    __syncthreads();
    const long long row = (long long)b * p.Tm + t;
    const int n = total < PM_MAXC ? total : PM_MAXC;
    if (tid < total && pk_keep[tid]) {
        int slot = 1;
        for (int q = 0; q < tid; q++) slot += pk_keep[q];
        if (slot <= PM_MAXC) {
            const float fq = pk_f[tid], s = pk_s[tid];
            p.cf[row * PM_NC + slot] = fq; p.cs[row * PM_NC + slot] = s; p.cd[row * PM_NC + slot] = s - PM_OC * log2f(PM_CEILING / fq);
        }
    }
    if (tid > n && tid < PM_NC) { p.cf[row * PM_NC + tid] = 0.f; p.cs[row * PM_NC + tid] = 0.f; p.cd[row * PM_NC + tid] = 0.f; }
    if (tid == 0) {
        p.cn[row] = n;
        p.cf[row * PM_NC] = 0.f; p.cs[row * PM_NC] = 0.f;
        p.cd[row * PM_NC] = PM_VT + fmaxf(0.f, 2.f - inten / (PM_ST / (1.f + PM_VT)));
    }
}

// One workgroup of one wave = one stream: the path through the candidates of its Tm frames that maximises the sum of the local scores minus the transition
// costs (0 between unvoiced frames, VUV across a voicing change, OJ |log2(f1 / f2)| between voiced ones).  Frames are serial; lane = 4 c + q holds candidate c
// of the current frame against the predecessors 4q .. 4q + 3, two shuffles finish the maximum (ties to the lowest index).  A step is
// (score[p] - cost(p, c)) maximised over p, plus delta[c]: the order of tests/pm_ref.py.  Candidates are staged 64 frames at a time, the back-pointers of the
// whole window stay in LDS (Tm <= 1024 frames x 16 bytes); lane 0 walks them back, column 15 takes the chosen index.
static __global__ __launch_bounds__(64) void pm_path_kernel(PmP p)
{
    __shared__ float sf[PM_CHUNK][16], sd[PM_CHUNK][16];
    __shared__ int sn[PM_CHUNK];
    __shared__ unsigned char bp[1024][16];
    __shared__ float sc[2][16], flast[16];
    const int b = blockIdx.x, lane = threadIdx.x, c = lane >> 2, q = lane & 3, Tm = p.Tm;
    const int *cn = p.cn + (long long)b * Tm;
    const float *cf = p.cf + (long long)b * Tm * PM_NC, *cd = p.cd + (long long)b * Tm * PM_NC;
    const float NEG = -__builtin_huge_valf();
    int nprev = 0, nlast = 0;
    for (int t0 = 0; t0 < Tm; t0 += PM_CHUNK) {
        const int nt = Tm - t0 < PM_CHUNK ? Tm - t0 : PM_CHUNK;
        __syncthreads();
        for (int k = lane; k < nt * 16; k += 64) {
            const int tt = k >> 4, cc = k & 15;
            sf[tt][cc] = cc < PM_NC ? cf[(long long)(t0 + tt) * PM_NC + cc] : 0.f;
            sd[tt][cc] = cc < PM_NC ? cd[(long long)(t0 + tt) * PM_NC + cc] : 0.f;
        }
        for (int k = lane; k < nt; k += 64) { const int v = cn[t0 + k]; sn[k] = v < 0 ? 0 : v > PM_MAXC ? PM_MAXC : v; }
        __syncthreads();
        for (int tt = 0; tt < nt; tt++) {
            const int t = t0 + tt, n = sn[tt];
            if (t == 0) {
                if (lane < 16) sc[0][lane] = lane <= n ? sd[0][lane] : NEG;
            } else {
                const int cur = t & 1, prv = cur ^ 1;
                const float *fp_row = tt ? sf[tt - 1] : flast;
                const float fc = sf[tt][c];
                float best = NEG;
                int arg = 4 * q;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int pp = 4 * q + k;
                    if (pp <= nprev) {
                        const float fp = fp_row[pp];
                        const float tr = (fp == 0.f && fc == 0.f) ? 0.f : (fp == 0.f || fc == 0.f) ? PM_VUV : PM_OJ * fabsf(log2f(fp / fc));
                        const float v = sc[prv][pp] - tr;
                        if (v > best) { best = v; arg = pp; }
                    }
                }
#pragma unroll
                for (int o = 1; o < 4; o <<= 1) {
                    const float ov = __shfl_xor(best, o, 64); const int oa = __shfl_xor(arg, o, 64);
                    if (ov > best || (ov == best && oa < arg)) { best = ov; arg = oa; }
                }
                if (q == 0) { sc[cur][c] = c <= n ? best + sd[tt][c] : NEG; bp[t][c] = (unsigned char)arg; }
            }
            nprev = n; nlast = n;
            __syncthreads();
        }
        if (lane < 16) flast[lane] = sf[nt - 1][lane];
    }
    __syncthreads();
    if (lane == 0) {
        const int cur = (Tm - 1) & 1;
        int idx = 0;
        float bv = sc[cur][0];
        for (int k = 1; k <= nlast; k++) if (sc[cur][k] > bv) { bv = sc[cur][k]; idx = k; }
        for (int t = Tm - 1; t > 0; t--) { const int prev = bp[t][idx]; bp[t][15] = (unsigned char)idx; idx = prev; }
        bp[0][15] = (unsigned char)idx;
    }
    __syncthreads();
    for (int t = lane; t < Tm; t += 64) {
        const int idx = bp[t][15];
        p.path[(long long)b * Tm + t] = idx;
        p.f0[(long long)b * Tm + t] = idx ? cf[(long long)t * PM_NC + idx] : 0.f;
    }
}

}  // namespace rvc
