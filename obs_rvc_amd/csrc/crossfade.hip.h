// crossfade.hip.h -- the two per-stream session stages that have no counterpart in the plugin (DESIGN.md "Phase-vocoder crossfade and input
// gate"), included by engine.hip behind chunk.hip.h:
//   * the phase-vocoder blend of the SOLA seam: analysis (windowed DFT of the saved tail and of the aligned new segment at n/2+1 bins, any n)
//     and synthesis (oscillator bank: every bin's phase glides from the old segment's to the new one's along the seam);
//   * the input gate: 10 ms blocks whose 40 ms RMS lies below a threshold are zeroed in front of the host-rate ring.
// Both run behind / in front of the existing launches on the engine's stream: the offset the seam starts at is read on the device.
#pragma once

namespace rvc {

constexpr int PV_MAX_N = 4096;      // 4 n floats of LDS in the analysis (64 KiB): every host rate up to 102.4 kHz (n = 4 zc)
constexpr int PV_AT = 128;          // analysis: bins (= threads) per workgroup
constexpr int PV_JT = 32, PV_KS = 8;   // synthesis: samples per workgroup x bin slices (256 threads)

// host tables of one seam length, evaluated in double and rounded once: [cos 2 pi m/n | sin 2 pi m/n] interleaved (2n), then win (n),
// fo^2 (n), fi^2 (n) with fi = sin^2(pi/2 j/(n-1)), fo = 1 - fi, win = sqrt(fo fi).  win[0] = win[n-1] = 0 exactly.
static inline void pv_tables(int n, std::vector<float> &t)
{
    t.assign((size_t)5 * n, 0.f);
    const double pi = 3.14159265358979323846;
    for (int m = 0; m < n; m++) {
        const double th = 2.0 * pi * (double)m / (double)n;
        t[2 * m] = (float)cos(th); t[2 * m + 1] = (float)sin(th);
        const double sn = sin(0.5 * pi * (double)m / (double)(n - 1));
        const double fi = m == n - 1 ? 1.0 : sn * sn, fo = 1.0 - fi;
        t[2 * n + m] = (float)sqrt(fo * fi); t[3 * n + m] = (float)(fo * fo); t[4 * n + m] = (float)(fi * fi);
    }
}
// the gate's threshold as the kernel takes it: -60 dB or lower is "off"
static inline float gate_threshold(double db) { return db > -60.0 ? (float)db : -INFINITY; }
static inline size_t pv_analysis_lds(int n) { return (size_t)4 * n * sizeof(float); }
static inline size_t pv_synth_lds(int n) { return ((size_t)2 * n + 3 * (size_t)(n / 2 + 1) + PV_KS * PV_JT) * sizeof(float); }

// mode of a stream: mode_v[stream], or mode_all for every stream when mode_v is NULL (the caller-side single-stream form)
__device__ __forceinline__ bool pv_stream(const int *mode_v, int mode_all, int b) { return (mode_v ? mode_v[b] : mode_all) == 1; }

// Analysis: Fa = DFT(a win), Fb = DFT(b win) at bins 0 .. n/2, one bin per thread, b = output[off ..] with the offset post_sola_kernel wrote.
// The phase k j mod n is carried in integers and the twiddle comes from the n-entry table in LDS: no angle is ever formed in fp32.
// spec [stream][3][K]: mag = |Fa| + |Fb| (doubled except DC and, n even, Nyquist), d = wrap(pb - pa) in [-pi, pi), pa.
static __global__ __launch_bounds__(PV_AT) void pv_analysis_kernel(const float *output, const float *a_g, const int *offset, const int *mode_v, int mode_all,
                                                            const float *tab, int n, float *spec, long long out_bs, long long a_bs)
{
    const int b = blockIdx.y;
    if (!pv_stream(mode_v, mode_all, b)) return;
    extern __shared__ __align__(16) float pv_lds[];
    float2 *cs = reinterpret_cast<float2 *>(pv_lds);
    float *aw = pv_lds + 2 * n, *bw = pv_lds + 3 * n;
    const int t = threadIdx.x, K = n / 2 + 1;
    const float *o = output + b * out_bs + offset[b], *a = a_g + b * a_bs;
    for (int j = t; j < n; j += PV_AT) {
        cs[j] = make_float2(tab[2 * j], tab[2 * j + 1]);
        const float w = tab[2 * n + j];
        aw[j] = a[j] * w; bw[j] = o[j] * w;
    }
    __syncthreads();
    const int k = blockIdx.x * PV_AT + t;
    if (k >= K) return;
    float ar = 0.f, ai = 0.f, br = 0.f, bi = 0.f;
    int idx = 0;
    for (int j = 0; j < n; j++) {
        const float2 w = cs[idx];
        const float x = aw[j], y = bw[j];
        ar = fmaf(x, w.x, ar); ai = fmaf(-x, w.y, ai);
        br = fmaf(y, w.x, br); bi = fmaf(-y, w.y, bi);
        idx += k; if (idx >= n) idx -= n;
    }
    float mag = sqrtf(ar * ar + ai * ai) + sqrtf(br * br + bi * bi);
    if (k != 0 && !(2 * k == n)) mag *= 2.f;
    const float pa = (ar == 0.f && ai == 0.f) ? 0.f : atan2f(ai, ar);
    const float pb = (br == 0.f && bi == 0.f) ? 0.f : atan2f(bi, br);
    float d = pb - pa;
    d -= 6.28318530717958647692f * floorf(d * 0.15915494309189533577f + 0.5f);
    spec += (long long)b * 3 * K;
    spec[k] = mag; spec[K + k] = d; spec[2 * K + k] = pa;
}

// Synthesis: out[j] = a[j] fo[j]^2 + b[j] fi[j]^2 + win[j]/n sum_k mag[k] cos((2 pi k + d[k]) j/n + pa[k]).  The argument is split into the
// table part 2 pi (k j mod n)/n and the small part d[k] j/n + pa[k] (|.| < 2 pi: accurate in fp32), combined by the angle-addition formula.
// A workgroup owns PV_JT samples of one stream; its 256 threads are PV_JT samples x PV_KS interleaved bin slices, summed in a fixed order.
// out goes where the linear blend goes: output[off + j], and with it into the frame (j < frame) or the saved tail (j >= frame), which
// post_sola_kernel filled from the unblended segment.
static __global__ __launch_bounds__(PV_JT * PV_KS) void pv_synth_kernel(float *output, const float *a_g, float *sola, float *frame_out, const int *offset,
                                                                 const int *mode_v, int mode_all, const float *tab, const float *spec, int n, int frame,
                                                                 long long out_bs, long long a_bs, long long sola_bs, long long frame_bs)
{
    const int b = blockIdx.y;
    if (!pv_stream(mode_v, mode_all, b)) return;
    extern __shared__ __align__(16) float pv_lds[];
    const int t = threadIdx.x, K = n / 2 + 1;
    float2 *cs = reinterpret_cast<float2 *>(pv_lds);
    float *mag = pv_lds + 2 * n, *dd = mag + K, *pa = dd + K, *red = pa + K;
    spec += (long long)b * 3 * K;
    for (int m = t; m < n; m += PV_JT * PV_KS) cs[m] = make_float2(tab[2 * m], tab[2 * m + 1]);
    for (int k = t; k < 3 * K; k += PV_JT * PV_KS) mag[k] = spec[k];
    __syncthreads();
    const int jl = t % PV_JT, sl = t / PV_JT, j = blockIdx.x * PV_JT + jl;
    float acc = 0.f;
    if (j < n) {
        const float jn = (float)j / (float)n;
        int idx = (sl * j) % n;
        const int step = (PV_KS * j) % n;
        for (int k = sl; k < K; k += PV_KS) {
            float sp, cp;
            sincosf(fmaf(dd[k], jn, pa[k]), &sp, &cp);
            const float2 w = cs[idx];
            acc = fmaf(mag[k], w.x * cp - w.y * sp, acc);
            idx += step; if (idx >= n) idx -= n;
        }
    }
    red[sl * PV_JT + jl] = acc;
    __syncthreads();
    if (sl == 0 && j < n) {
        float s = red[jl];
#pragma unroll
        for (int q = 1; q < PV_KS; q++) s += red[q * PV_JT + jl];
        float *o = output + b * out_bs + offset[b];
        const float v = a_g[b * a_bs + j] * tab[3 * n + j] + o[j] * tab[4 * n + j] + tab[2 * n + j] / (float)n * s;
        o[j] = v;
        if (j < frame) frame_out[b * frame_bs + j] = v; else sola[b * sola_bs + j - frame] = v;
    }
}

// Input gate.  x = concat(hist (3 zc, the ungated input before this chunk), chunk (f = a multiple of zc)); workgroup i < f/zc owns block i:
// rms over x[i zc .. i zc + 4 zc), db = 20 log10(max(rms, 1e-5)), the block's zc samples are zero in `out` when db < threshold and the chunk's
// otherwise.  A threshold <= -60 is "off": the stream is copied through without a sum.  Workgroup f/zc writes the next history (the last
// 3 zc samples of x) into the other half of the ping-pong pair.
static __global__ __launch_bounds__(256) void input_gate_kernel(const float *chunk, float *out, const float *hist_in, float *hist_out, const float *thr_v, float thr_all,
                                                         int zc, int f, long long chunk_bs, long long hist_bs)
{
    __shared__ float red[16];
    const int b = blockIdx.y, i = blockIdx.x, t = threadIdx.x, h = 3 * zc;
    chunk += b * chunk_bs; out += b * chunk_bs; hist_in += b * hist_bs; hist_out += b * hist_bs;
    if (i == f / zc) {
        for (int q = t; q < h; q += 256) { const int p = f + q; hist_out[q] = p < h ? hist_in[p] : chunk[p - h]; }
        return;
    }
    const float thr = thr_v ? thr_v[b] : thr_all;
    bool open = true;
    if (thr > -60.f) {
        float s = 0.f;
        for (int q = t; q < 4 * zc; q += 256) { const int p = i * zc + q; const float v = p < h ? hist_in[p] : chunk[p - h]; s = fmaf(v, v, s); }
        s = block_sum(s, red);
        const float db = 20.f * log10f(fmaxf(sqrtf(s / (float)(4 * zc)), 1e-5f));
        open = !(db < thr);
    }
    for (int q = t; q < zc; q += 256) out[i * zc + q] = open ? chunk[i * zc + q] : 0.f;
}

}  // namespace rvc
