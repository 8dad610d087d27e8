// yin.hip.h -- YIN pitch tracker (de Cheveigne & Kawahara 2002) as the engine's weight-free f0 method: DESIGN.md section 11 has the definition
#pragma once
#include <hip/hip_runtime.h>

namespace rvc {

constexpr int YIN_FRAME = 1024, YIN_HOP = 160, YIN_PAD = 512;       // the mel front end's frames (rmvpe.rs:47-67, 159-205)
constexpr int YIN_TAU_MIN = 14, YIN_TAU_MAX = 320, YIN_N = YIN_FRAME - YIN_TAU_MAX;      // lags searched [14, 320), integration window 704
constexpr float YIN_THRESHOLD = 0.15f;
constexpr int YIN_WAVES = 8, YIN_SEG = YIN_N / YIN_WAVES;           // one wave per 88 window positions
static_assert(YIN_TAU_MAX == 5 * 64 && YIN_SEG * YIN_WAVES == YIN_N && YIN_SEG % 4 == 0, "yin_f0_kernel: five lags per lane, whole blocks of four positions per wave");

struct YinP {
    const float *audio;     // [B][n] 16 kHz input (device)
    long long audio_bs;
    int n;                  // samples per stream
    int frame;              // f0_extractor_frame: the last `frame` samples are analysed
    int Tm;
    float *f0;              // [B][Tm] raw f0 in Hz, 0 = unvoiced
};

// One workgroup = one frame of one stream.  d(tau) = sum_{j < 704} (x[j] - x[j + tau])^2 in the direct difference form for tau = 1..320 (d(0) = 0):
// lane l of EVERY wave owns the five lags 5l+1 .. 5l+5 and wave w the window positions [88w, 88w + 88).  For four positions j..j+3 a lane needs
// x[j + 5l + 1 .. j + 5l + 8]: lanes are five dwords apart, an odd stride, so a dword read is free of bank conflicts, and x[j..j+3] is one address
// for the whole wave (a broadcast); four of the eight values stay in registers from the block before.  The eight partial sums per lag are
// folded pairwise by wave 0, whose lanes then hold five consecutive d: the running sum S(tau) is a serial sum of five and a wave-64 shuffle scan.
static __global__ __launch_bounds__(YIN_WAVES * 64) void yin_f0_kernel(YinP p)
{
    __shared__ __attribute__((aligned(16))) float xs[YIN_FRAME];            // (the highest index read is 703 + 320)
    __shared__ float part[YIN_WAVES][YIN_TAU_MAX];
    __shared__ float dp[YIN_TAU_MAX + 1];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *sig = p.audio + (long long)b * p.audio_bs + (p.n - p.frame);
    const int L = p.frame;
    // frame t covers padded[160 t .. 160 t + 1024), padded = reflect(sig, 512): the reflection is index arithmetic (mel_frontend_kernel)
    for (int j = tid; j < YIN_FRAME; j += YIN_WAVES * 64) {
        int q = t * YIN_HOP + j - YIN_PAD;
        if (q < 0) q = -q;
        if (q >= L) q = 2 * L - 2 - q;
        xs[j] = sig[q];
    }
    __syncthreads();
    {
        const int j0 = wave * YIN_SEG, o = 5 * lane + 1;
        float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        float y[8];
#pragma unroll
        for (int k = 0; k < 4; k++) y[k] = xs[j0 + o + k];
#pragma unroll 2
        for (int j = j0; j < j0 + YIN_SEG; j += 4) {
            const float4 xv = *reinterpret_cast<const float4 *>(&xs[j]);
            const float x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
            for (int k = 0; k < 4; k++) y[4 + k] = xs[j + o + 4 + k];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int k = 0; k < 5; k++) { const float df = x4[i] - y[i + k]; acc[k] = fmaf(df, df, acc[k]); }
#pragma unroll
            for (int k = 0; k < 4; k++) y[k] = y[4 + k];
        }
#pragma unroll
        for (int k = 0; k < 5; k++) part[wave][o - 1 + k] = acc[k];
    }
    __syncthreads();
    int tau = YIN_TAU_MAX;
    if (wave == 0) {
        // d'(tau) = d(tau) tau / S(tau), S(tau) = d(1) + ... + d(tau); S == 0 -> 1 (an all-zero frame is unvoiced); d'(0) = 1
        float d[5], s[5];
        float run = 0.f;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int i = 5 * lane + k;
            d[k] = ((part[0][i] + part[1][i]) + (part[2][i] + part[3][i])) + ((part[4][i] + part[5][i]) + (part[6][i] + part[7][i]));
            run += d[k]; s[k] = run;
        }
        float incl = run;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const float v = __shfl_up(incl, off, 64); if (lane >= off) incl += v; }
        float base = __shfl_up(incl, 1, 64);     // S of the lag in front of this lane's five
        if (lane == 0) base = 0.f;
        int first = YIN_TAU_MAX;
#pragma unroll
        for (int k = 4; k >= 0; k--) {
            const int tk = 5 * lane + 1 + k;
            const float S = base + s[k];
            const float v = S > 0.f ? d[k] * (float)tk / S : 1.f;
            dp[tk] = v;
            if (tk >= YIN_TAU_MIN && tk < YIN_TAU_MAX && v < YIN_THRESHOLD) first = tk;
        }
        if (lane == 0) dp[0] = 1.f;
        // the smallest lag under the threshold: the lowest lane that has one holds it
        const unsigned long long hit = __ballot(first < YIN_TAU_MAX);
        if (hit) tau = __shfl(first, __ffsll((long long)hit) - 1, 64);
    }
    __syncthreads();
    if (tid == 0) {
        // walk down to the local minimum, then the vertex of the parabola through its neighbours
        float hz = 0.f;
        if (tau < YIN_TAU_MAX) {
            while (tau + 1 < YIN_TAU_MAX && dp[tau + 1] < dp[tau]) tau++;
            const float a = dp[tau - 1], bb = dp[tau], c = dp[tau + 1];
            const float den = a - 2.f * bb + c;
            const float off = den > 0.f ? 0.5f * (a - c) / den : 0.f;
            hz = 16000.0f / ((float)tau + off);
        }
        p.f0[(long long)b * p.Tm + t] = hz;
    }
}

}  // namespace rvc
