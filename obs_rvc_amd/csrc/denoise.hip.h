// denoise.hip.h -- streaming spectral-gate noise reduction (DESIGN.md "Spectral-gate noise reduction"), included by engine.hip in front of
// session.hip.h.  The plugin has no such stage; this is the upstream real-time client's input / output noise reduction restated causally.
//
// Definition, per stream at sample rate sr (a multiple of 100).  H = zc = sr / 100 is the hop, N = 2 zc the frame (bins are 50 Hz wide),
// K = zc + 1 bins, w[j] = sin(pi (j + 0.5) / N) for analysis and synthesis (w[j]^2 + w[j + H]^2 = 1).  The input is a stream of hop blocks
// x_0, x_1, ... with x_{-1} = 0; frame m = concat(x_{m-1}, x_m).  State: S[k] = 0, g[k] = 0, the previous block and the previous frame's
// synthesis tail, all zero at creation and after reset.  For frame m and bin k:
//   1. X[k] = sum_j w[j] frame[j] exp(-2 pi i k j / N) (unnormalised), M = |X[k]|
//   2. slope = (M - S[k]) / max(S[k], 1e-8) with S read before its update S[k] = a S[k] + (1 - a) M, a = (float)exp(-10 / 200): a 200 ms noise floor
//   3. g0[k] = 1 / (1 + exp(-(slope - threshold) / 0.1))
//   4. g1[k] = sum_{d = -10 .. 10, 0 <= k + d < K} t[d] g0[k + d] / sum_{same d} t[d], t[d] = 11 - |d|: a +-500 Hz triangle, renormalised at the edges
//   5. g[k] = max(g1[k], b g[k]), b = (float)exp(-10 / 50): a 50 ms release hold
//   6. G = strength g[k] + (1 - strength), Y[k] = G X[k]
//   7. f = w . irfft_N(Y) (the real inverse with its 1 / N)
// Output block m = f_{m-1}[H:] + f_m[:H]: the gated x_{m-1}, i.e. the input delayed by zc samples (10 ms).  The constants 0.1, 200 ms, 50 ms,
// +-10 bins and 1e-8 are fixed.  strength in [0, 1] (0 = off: the stream is copied undelayed, bit for bit, its state untouched), threshold in [0, 16].
//
// Three launches per call on the engine's stream:
//   dn_analysis_kernel  grid (ceil(K / 128), frames, streams): direct DFT (N is no power of two: 882 at 44.1 kHz), one bin per thread.  The phase
//                       k j mod N is carried in integers and the twiddle is read from an N-entry (cos, sin) table in LDS (evaluated on the host in
//                       double, once per sr, like w).  exp(-2 pi i k (j + H) / N) = (-1)^k exp(-2 pi i k j / N): a bin sums H terms of
//                       w[j] a[j] +- w[j + H] b[j] (a = the frame's first block, b its second), not N.
//   dn_mask_kernel      grid (streams): steps 1 (|X|) to 6 for the call's frames in order, S, g and the K gains of step 4 in LDS; Y overwrites X;
//                       the call's last block becomes the next call's previous block.
//   dn_synth_kernel     grid (ceil(H / 32), frames + 1, streams), 256 threads = 32 samples x 8 interleaved bin slices summed through LDS in a
//                       fixed order.  Row m computes the first half of frame m and the second half of frame m - 1 (the same twiddle serves both:
//                       the second half's is (-1)^k times it) and adds them; row 0 takes the second half from the saved tail, row `frames` writes
//                       the next tail into the other half of a ping-pong pair.
// Every sum has a fixed order and no stream reads another's data: a stream's result depends neither on the batch nor on how the signal is cut into
// calls (the tail a call saves is the value the next call would have computed in place).  Floating-point contraction is off inside the kernels
// and every fused multiply-add is written out, so that the two places the same value is formed in give the same bits.
// LDS: analysis 12 N bytes, synthesis 8 N + 16 K + 2 KiB, mask 12 K; N <= DN_MAX_N = 3840 (sr <= 192 000) keeps each under 64 KiB (synthesis: 62 KiB).
#pragma once

namespace rvc {

constexpr int DN_MAX_N = 3840;            // frame length limit (62 KiB of LDS in the synthesis): every host rate up to 192 kHz
constexpr int DN_AT = 128;                // analysis: bins (= threads) per workgroup
constexpr int DN_JT = 32, DN_KS = 8;      // synthesis: samples per workgroup x bin slices (256 threads)
constexpr int DN_MT = 256;                // mask: threads of a stream's workgroup
constexpr int DN_MAX_FRAMES = 4096;       // hops per call
constexpr int DN_SMOOTH = 10;             // step 4: +-10 bins
constexpr float DN_SOFT = 0.1f, DN_EPS = 1e-8f;

// host tables of one frame length, evaluated in double and rounded once: [cos 2 pi m / N | sin 2 pi m / N] interleaved (2 N), then w (N)
static inline void dn_tables(int N, std::vector<float> &t)
{
    t.assign((size_t)3 * N, 0.f);
    const double pi = 3.14159265358979323846;
    for (int m = 0; m < N; m++) {
        const double th = 2.0 * pi * (double)m / (double)N;
        t[2 * m] = (float)cos(th); t[2 * m + 1] = (float)sin(th);
        t[2 * N + m] = (float)sin(pi * ((double)m + 0.5) / (double)N);
    }
}
static inline size_t dn_analysis_lds(int N) { return (size_t)3 * N * sizeof(float); }
static inline size_t dn_synth_lds(int N) { return ((size_t)2 * N + 4 * (size_t)(N / 2 + 1) + 2 * DN_KS * DN_JT) * sizeof(float); }
static inline size_t dn_mask_lds(int N) { return (size_t)3 * (N / 2 + 1) * sizeof(float); }

// par [stream] = (strength, threshold); spec [stream][frame][re | im][K]
static __global__ __launch_bounds__(DN_AT) void dn_analysis_kernel(const float *in, const float *prev, const float2 *par, const float *tab, int N, int F, float *spec,
                                                                    long long in_bs, long long spec_bs)
{
#pragma clang fp contract(off)
    const int b = blockIdx.z, m = blockIdx.y, t = threadIdx.x, H = N / 2, K = H + 1;
    if (par[b].x == 0.f) return;
    extern __shared__ __align__(16) float dn_lds[];
    float2 *cs = reinterpret_cast<float2 *>(dn_lds);
    float *ev = dn_lds + 2 * N, *od = ev + H;
    const float *x1 = in + b * in_bs + (long long)m * H;                                    // x_m
    const float *x0 = m == 0 ? prev + (long long)b * H : x1 - H;                            // x_{m-1}
    for (int j = t; j < N; j += DN_AT) cs[j] = make_float2(tab[2 * j], tab[2 * j + 1]);
    for (int j = t; j < H; j += DN_AT) {
        const float wa = tab[2 * N + j] * x0[j], wb = tab[2 * N + H + j] * x1[j];
        ev[j] = wa + wb; od[j] = wa - wb;
    }
    __syncthreads();
    const int k = blockIdx.x * DN_AT + t;
    if (k >= K) return;
    const float *v = (k & 1) ? od : ev;
    float re = 0.f, im = 0.f;
    int idx = 0;
    for (int j = 0; j < H; j++) {
        const float2 w = cs[idx];
        const float x = v[j];
        re = fmaf(x, w.x, re); im = fmaf(-x, w.y, im);
        idx += k; if (idx >= N) idx -= N;
    }
    spec += b * spec_bs + (long long)m * 2 * K;
    spec[k] = re; spec[K + k] = im;
}

// one workgroup per stream walks the call's frames in order; S / g [stream][K] are updated in place, prev [stream][H] takes the call's last block
static __global__ __launch_bounds__(DN_MT) void dn_mask_kernel(const float *in, float *prev, const float2 *par, int N, int F, float *spec, float *S_g, float *g_g,
                                                                float a, float rel, long long in_bs, long long spec_bs)
{
#pragma clang fp contract(off)
    const int b = blockIdx.x, t = threadIdx.x, H = N / 2, K = H + 1;
    const float strength = par[b].x, thr = par[b].y;
    if (strength == 0.f) return;
    extern __shared__ __align__(16) float dn_lds[];
    float *S = dn_lds, *g = S + K, *g0 = g + K;
    S_g += (long long)b * K; g_g += (long long)b * K; spec += b * spec_bs;
    for (int k = t; k < K; k += DN_MT) { S[k] = S_g[k]; g[k] = g_g[k]; }
    const float oma = 1.f - a, oms = 1.f - strength;
    for (int m = 0; m < F; m++) {
        float *X = spec + (long long)m * 2 * K;
        for (int k = t; k < K; k += DN_MT) {
            const float re = X[k], im = X[K + k];
            const float M = sqrtf(fmaf(re, re, im * im)), s = S[k];
            const float slope = (M - s) / fmaxf(s, DN_EPS);
            S[k] = fmaf(a, s, oma * M);
            g0[k] = 1.f / (1.f + expf(-(slope - thr) / DN_SOFT));
        }
        __syncthreads();
        for (int k = t; k < K; k += DN_MT) {
            float num = 0.f; int den = 0;
            for (int d = -DN_SMOOTH; d <= DN_SMOOTH; d++) {
                const int kk = k + d, tw = DN_SMOOTH + 1 - (d < 0 ? -d : d);
                if (kk >= 0 && kk < K) { num = fmaf((float)tw, g0[kk], num); den += tw; }
            }
            const float gn = fmaxf(num / (float)den, rel * g[k]);
            g[k] = gn;
            const float G = fmaf(strength, gn, oms);
            X[k] *= G; X[K + k] *= G;
        }
        __syncthreads();
    }
    for (int k = t; k < K; k += DN_MT) { S_g[k] = S[k]; g_g[k] = g[k]; }
    const float *last = in + b * in_bs + (long long)(F - 1) * H;
    prev += (long long)b * H;
    for (int j = t; j < H; j += DN_MT) prev[j] = last[j];
}

// w[j] / N * (Y[0] + sign Y[N/2] + 2 sum): one windowed sample of a frame's inverse transform from its inner-bin sum
static __device__ __forceinline__ float dn_sample(float w, float inv_n, float dc, float ny, float sum)
{
#pragma clang fp contract(off)
    return (w * inv_n) * ((dc + ny) + 2.f * sum);
}

static __global__ __launch_bounds__(DN_JT * DN_KS) void dn_synth_kernel(const float *in, float *out, const float2 *par, const float *tab, const float *spec, int N, int F,
                                                                         const float *tail_old, float *tail_new, long long in_bs, long long out_bs, long long spec_bs)
{
#pragma clang fp contract(off)
    const int b = blockIdx.z, m = blockIdx.y, t = threadIdx.x, H = N / 2, K = H + 1;
    const int jl = t % DN_JT, sl = t / DN_JT, j = blockIdx.x * DN_JT + jl;
    in += b * in_bs; out += b * out_bs; tail_old += (long long)b * H; tail_new += (long long)b * H;
    if (par[b].x == 0.f) {          // off: the stream passes undelayed and keeps its state
        if (sl == 0 && j < H) {
            if (m == F) tail_new[j] = tail_old[j];
            else if (in != out) out[(long long)m * H + j] = in[(long long)m * H + j];
        }
        return;
    }
    extern __shared__ __align__(16) float dn_lds[];
    float2 *cs = reinterpret_cast<float2 *>(dn_lds);
    float *Yc = dn_lds + 2 * N, *Yp = Yc + 2 * K, *red = Yp + 2 * K;       // frame m, frame m - 1: [re | im][K]
    const bool cur = m < F, prv = m > 0;
    spec += b * spec_bs;
    for (int q = t; q < N; q += DN_JT * DN_KS) cs[q] = make_float2(tab[2 * q], tab[2 * q + 1]);
    for (int q = t; q < 2 * K; q += DN_JT * DN_KS) {
        Yc[q] = cur ? spec[(long long)m * 2 * K + q] : 0.f;
        Yp[q] = prv ? spec[(long long)(m - 1) * 2 * K + q] : 0.f;
    }
    __syncthreads();
    float acc0 = 0.f, acc1 = 0.f;
    if (j < H) {
        int idx = ((1 + sl) * j) % N;
        const int step = (DN_KS * j) % N;
        for (int k = 1 + sl; k < K - 1; k += DN_KS) {        // inner bins; DC and Nyquist are added by dn_sample
            const float2 w = cs[idx];
            acc0 = fmaf(Yc[k], w.x, acc0); acc0 = fmaf(-Yc[K + k], w.y, acc0);
            const float sg = (k & 1) ? -1.f : 1.f;            // exp(2 pi i k (j + H) / N) = (-1)^k exp(2 pi i k j / N)
            acc1 = fmaf(sg * Yp[k], w.x, acc1); acc1 = fmaf(-(sg * Yp[K + k]), w.y, acc1);
            idx += step; if (idx >= N) idx -= N;
        }
    }
    red[sl * DN_JT + jl] = acc0; red[(DN_KS + sl) * DN_JT + jl] = acc1;
    __syncthreads();
    if (sl == 0 && j < H) {
        float s0 = red[jl], s1 = red[DN_KS * DN_JT + jl];
#pragma unroll
        for (int q = 1; q < DN_KS; q++) { s0 += red[q * DN_JT + jl]; s1 += red[(DN_KS + q) * DN_JT + jl]; }
        const float inv_n = 1.f / (float)N;
        // second half of frame m - 1 (sample H + j), or the tail the previous call saved
        const float f1 = prv ? dn_sample(tab[2 * N + H + j], inv_n, Yp[0], ((H + j) & 1) ? -Yp[K - 1] : Yp[K - 1], s1) : tail_old[j];
        if (!cur) { tail_new[j] = f1; return; }
        const float f0 = dn_sample(tab[2 * N + j], inv_n, Yc[0], (j & 1) ? -Yc[K - 1] : Yc[K - 1], s0);
        out[(long long)m * H + j] = f1 + f0;
    }
}

}  // namespace rvc

using namespace rvc;

struct rvc_denoiser {
    rvc_engine *e = nullptr;
    int sample_rate = 0, zc = 0, N = 0, K = 0, nb = 1, cap_frames = 0, n_on = 0, parity = 0;
    float a = 0.f, rel = 0.f;
    std::vector<float2> par; bool dirty = true;         // (strength, threshold) per stream
    float *d_tab = nullptr, *d_prev = nullptr, *d_S = nullptr, *d_g = nullptr, *d_tail[2] = {nullptr, nullptr}, *d_spec = nullptr, *d_x = nullptr, *d_y = nullptr;
    float2 *d_par = nullptr;
    size_t cap_host = 0;                                // samples per stream the host-path staging buffers d_x / d_y hold
};

static void denoiser_zero_state(rvc_denoiser *d)
{
    hipStream_t st = d->e->stream;
    const size_t nb = (size_t)d->nb;
    HIPCHK(hipMemsetAsync(d->d_prev, 0, nb * d->zc * 4, st)); HIPCHK(hipMemsetAsync(d->d_S, 0, nb * d->K * 4, st)); HIPCHK(hipMemsetAsync(d->d_g, 0, nb * d->K * 4, st));
    for (float *p : d->d_tail) HIPCHK(hipMemsetAsync(p, 0, nb * d->zc * 4, st));
}

// the spectrum scratch holds `frames` frames per stream (grown between calls; the session sizes it once)
static void denoiser_reserve(rvc_denoiser *d, int frames)
{
    if (frames <= d->cap_frames) return;
    HIPCHK(hipStreamSynchronize(d->e->stream));
    (void)hipFree(d->d_spec); d->d_spec = nullptr; d->cap_frames = 0;
    HIPCHK(hipMalloc(&d->d_spec, (size_t)d->nb * frames * 2 * d->K * 4));
    d->cap_frames = frames;
}

static void denoiser_check(double strength, double threshold)
{
    if (!(strength >= 0.0 && strength <= 1.0)) throw ShapeError("denoiser: strength must lie in [0, 1]");
    if (!(threshold >= 0.0 && threshold <= 16.0)) throw ShapeError("denoiser: threshold must lie in [0, 16]");
}

// a call takes 1 .. DN_MAX_FRAMES whole hops (the frames are a grid dimension)
static void denoiser_check_n(const rvc_denoiser *d, size_t n)
{
    if (n == 0 || n % (size_t)d->zc != 0) throw ShapeError("denoiser: n must be a positive multiple of sample_rate / 100");
    if (n / (size_t)d->zc > (size_t)DN_MAX_FRAMES) throw ShapeError("denoiser: a call takes at most 4096 hops (40.96 s)");
}

extern "C" void rvc_denoiser_destroy(rvc_denoiser *d);

static rvc_status denoiser_create_n(rvc_engine *e, size_t sample_rate, int nb, int frames, rvc_denoiser **out)
{
    if (out) *out = nullptr;
    return guarded(e, [&]() {
        if (!out || nb < 1) throw ShapeError("denoiser: bad arguments");
        if (sample_rate < 1000 || sample_rate % 100 != 0) throw ShapeError("denoiser: the sample rate must be a multiple of 100 (at least 1000)");
        if (sample_rate / 50 > (size_t)DN_MAX_N) throw ShapeError("denoiser: the frame of sample_rate / 50 samples exceeds 3840 (sample rates up to 192000)");
        std::unique_ptr<rvc_denoiser, void (*)(rvc_denoiser *)> dp(new rvc_denoiser(), rvc_denoiser_destroy);
        rvc_denoiser *d = dp.get();
        d->e = e; d->sample_rate = (int)sample_rate; d->zc = (int)sample_rate / 100; d->N = 2 * d->zc; d->K = d->zc + 1; d->nb = nb;
        d->a = (float)exp(-10.0 / 200.0); d->rel = (float)exp(-10.0 / 50.0);
        d->par.assign(nb, make_float2(0.f, 2.f));
        std::vector<float> tab; dn_tables(d->N, tab);
        HIPCHK(hipMalloc(&d->d_tab, tab.size() * 4)); HIPCHK(hipMemcpy(d->d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        const size_t NB = (size_t)nb;
        HIPCHK(hipMalloc(&d->d_prev, NB * d->zc * 4)); HIPCHK(hipMalloc(&d->d_S, NB * d->K * 4)); HIPCHK(hipMalloc(&d->d_g, NB * d->K * 4));
        for (float *&p : d->d_tail) HIPCHK(hipMalloc(&p, NB * d->zc * 4));
        HIPCHK(hipMalloc(&d->d_par, NB * sizeof(float2)));
        denoiser_zero_state(d);
        denoiser_reserve(d, std::max(frames, 1));
        HIPCHK(hipStreamSynchronize(e->stream));
        *out = dp.release();
        return RVC_OK;
    });
}

// queue one call (n = frames * zc samples of every stream) on the engine's stream; stream b at d_in + b * in_bs / d_out + b * out_bs
static void denoiser_launch(rvc_denoiser *d, const float *d_in, float *d_out, int n, long long in_bs, long long out_bs)
{
    hipStream_t st = d->e->stream;
    const int F = n / d->zc, N = d->N, H = d->zc, K = d->K, B = d->nb;
    if (d->dirty) {      // settings that changed since the last call (ordered behind the calls still queued; paid by the call after a setter only)
        HIPCHK(hipMemcpyAsync(d->d_par, d->par.data(), (size_t)B * sizeof(float2), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        d->dirty = false;
    }
    if (d->n_on == 0) {   // every stream off: a copy, no launch
        if (d_in != d_out) HIPCHK(hipMemcpy2DAsync(d_out, (size_t)out_bs * 4, d_in, (size_t)in_bs * 4, (size_t)n * 4, B, hipMemcpyDeviceToDevice, st));
        return;
    }
    denoiser_reserve(d, F);
    const long long spec_bs = (long long)d->cap_frames * 2 * K;
    hipLaunchKernelGGL(dn_analysis_kernel, dim3((K + DN_AT - 1) / DN_AT, F, B), dim3(DN_AT), dn_analysis_lds(N), st, d_in, d->d_prev, d->d_par, d->d_tab, N, F, d->d_spec, in_bs, spec_bs);
    hipLaunchKernelGGL(dn_mask_kernel, dim3(B), dim3(DN_MT), dn_mask_lds(N), st, d_in, d->d_prev, d->d_par, N, F, d->d_spec, d->d_S, d->d_g, d->a, d->rel, in_bs, spec_bs);
    hipLaunchKernelGGL(dn_synth_kernel, dim3((H + DN_JT - 1) / DN_JT, F + 1, B), dim3(DN_JT * DN_KS), dn_synth_lds(N), st, d_in, d_out, d->d_par, d->d_tab, d->d_spec, N, F,
                       d->d_tail[d->parity], d->d_tail[d->parity ^ 1], in_bs, out_bs, spec_bs);
    d->parity ^= 1;
}

// settings of streams [first, last); validated by the caller
static void denoiser_set_range(rvc_denoiser *d, int first, int last, double strength, double threshold)
{
    for (int b = first; b < last; b++) d->par[b] = make_float2((float)strength, (float)threshold);
    d->n_on = 0;
    for (int b = 0; b < d->nb; b++) d->n_on += d->par[b].x != 0.f;
    d->dirty = true;
}

extern "C" {

rvc_status rvc_denoiser_create(rvc_engine *e, size_t sample_rate, int n_streams, rvc_denoiser **out)
{
    if (out) *out = nullptr;
    if (e && (n_streams < 1 || n_streams > 4096)) { e->err = "denoiser: n_streams must lie in 1 .. 4096"; return RVC_SHAPE; }
    return denoiser_create_n(e, sample_rate, n_streams, 16, out);
}

void rvc_denoiser_destroy(rvc_denoiser *d)
{
    if (!d) return;
    (void)hipSetDevice(d->e->device);
    (void)hipStreamSynchronize(d->e->stream);
    for (float *p : {d->d_tab, d->d_prev, d->d_S, d->d_g, d->d_tail[0], d->d_tail[1], d->d_spec, d->d_x, d->d_y}) (void)hipFree(p);
    (void)hipFree(d->d_par);
    delete d;
}

// zero S, g, the previous block and the synthesis tail of every stream; the settings stay
void rvc_denoiser_reset(rvc_denoiser *d)
{
    if (!d) return;
    (void)guarded(d->e, [&]() {
        denoiser_zero_state(d);
        HIPCHK(hipStreamSynchronize(d->e->stream));
        return RVC_OK;
    });
}

rvc_status rvc_denoiser_set(rvc_denoiser *d, int stream, double strength, double threshold)
{
    if (!d) return RVC_BACKEND;
    return guarded(d->e, [&]() {
        if (stream < -1 || stream >= d->nb) throw ShapeError("denoiser: stream out of range");
        denoiser_check(strength, threshold);
        denoiser_set_range(d, stream < 0 ? 0 : stream, stream < 0 ? d->nb : stream + 1, strength, threshold);
        return RVC_OK;
    });
}

size_t rvc_denoiser_latency(rvc_denoiser *d) { return d ? (size_t)d->zc : 0; }

rvc_status rvc_denoiser_process(rvc_denoiser *d, const float *in, size_t n, float *out)
{
    if (!d) return RVC_BACKEND;
    return guarded(d->e, [&]() {
        denoiser_check_n(d, n);
        if (!in || !out) throw ShapeError("denoiser: null buffer");
        hipStream_t st = d->e->stream;
        if (n > d->cap_host) {
            HIPCHK(hipStreamSynchronize(st));
            (void)hipFree(d->d_x); (void)hipFree(d->d_y); d->d_x = d->d_y = nullptr; d->cap_host = 0;
            HIPCHK(hipMalloc(&d->d_x, (size_t)d->nb * n * 4)); HIPCHK(hipMalloc(&d->d_y, (size_t)d->nb * n * 4));
            d->cap_host = n;
        }
        HIPCHK(hipMemcpyAsync(d->d_x, in, (size_t)d->nb * n * 4, hipMemcpyHostToDevice, st));
        denoiser_launch(d, d->d_x, d->d_y, (int)n, (long long)n, (long long)n);
        HIPCHK(hipMemcpyAsync(out, d->d_y, (size_t)d->nb * n * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        return RVC_OK;
    });
}

rvc_status rvc_denoiser_process_device(rvc_denoiser *d, const void *d_in, void *d_out, size_t n, size_t in_stride, size_t out_stride, int sync)
{
    if (!d) return RVC_BACKEND;
    return guarded(d->e, [&]() {
        denoiser_check_n(d, n);
        if (!d_in || !d_out) throw ShapeError("denoiser: null device pointer");
        if (in_stride < n || out_stride < n) throw ShapeError("denoiser: a stream stride is shorter than n");
        denoiser_launch(d, static_cast<const float *>(d_in), static_cast<float *>(d_out), (int)n, (long long)in_stride, (long long)out_stride);
        if (sync) HIPCHK(hipStreamSynchronize(d->e->stream));
        HIPCHK(hipGetLastError());
        return RVC_OK;
    });
}

}  // extern "C"
