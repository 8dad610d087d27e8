// formant.hip.h -- formant shift (the plugin's resonance shift, obs-rvc/src/lib.rs:80,103,176,369-375,446-451): geometry, the
// windowed-sinc filter table, and the two kernels of the synthesizer's formant stage (DESIGN.md "Formant shift").
//   geometry   f = 2^(phi / 12), R2 = ceil(R f), upp_res = floor(f sr / 100)
//   stretch    the NSF source (R upp samples) and the latent z (R frames) are linearly interpolated to R2 upp / R2 (time_lerp_kernel)
//   decoder    runs on R2 frames
//   back       y2[0 : R upp_res] is resampled upp_res -> upp by a Hann-windowed sinc (width 6, rolloff 0.99; formant_resample_kernel)
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>
#include "state.hip.h"

namespace rvc {

constexpr double FORMANT_MAX = 5.0;      // the plugin's slider range (lib.rs:369-375)

// -> false for a semitone value outside [-5, 5] or NaN, or a geometry the stage cannot serve
static inline bool formant_geometry(size_t R, size_t sr, double semitones, size_t *R2, size_t *upp_res)
{
    if (!(semitones >= -FORMANT_MAX && semitones <= FORMANT_MAX)) return false;
    if (R < 1 || sr < 100 || sr % 100 != 0) return false;
    const double f = std::pow(2.0, semitones / 12.0);
    *R2 = (size_t)std::ceil((double)R * f);
    *upp_res = (size_t)std::floor(f * (double)sr / 100.0);
    return *upp_res >= 1;
}

static inline size_t formant_gcd(size_t a, size_t b) { while (b) { const size_t t = a % b; a = b; b = t; } return a; }

// The filter table of the resampler o -> n (both already divided by their gcd): h[j][k], j < n, k < K = 2w + o, computed in double and
// stored as fp32.  Meant to equal torchaudio.transforms.Resample(o, n) with its defaults -- unpinned against upstream.
static inline void formant_table(size_t o, size_t n, std::vector<float> &h, size_t *w_out, size_t *K_out)
{
    const double PI = 3.14159265358979323846;
    const double b = 0.99 * (double)(o < n ? o : n);
    const size_t w = (size_t)std::ceil(6.0 * (double)o / b), K = 2 * w + o;
    h.assign(n * K, 0.f);
    for (size_t j = 0; j < n; j++)
        for (size_t k = 0; k < K; k++) {
            double t = (((double)k - (double)w) / (double)o - (double)j / (double)n) * b;
            t = t < -6.0 ? -6.0 : (t > 6.0 ? 6.0 : t);
            const double a = PI * t, c = std::cos(a / 12.0);
            const double s = t == 0.0 ? 1.0 : std::sin(a) / a;
            h[j * K + k] = (float)(s * c * c * b / (double)o);
        }
    *w_out = w; *K_out = K;
}

// the formant fields of StreamState (f_tab .. f_ident) as the host writes them
struct FormantDesc {
    const float *tab; const int *kb; int o, n, w, kt, nx, ident;
    bool operator==(const FormantDesc &x) const { return tab == x.tab && kb == x.kb && o == x.o && n == x.n && w == x.w && kt == x.kt && nx == x.nx && ident == x.ident; }
};
// Device form of a table: row j keeps only its span of nonzero fp32 taps, [kb[j], kb[j] + Kt).  The taps left out are exact zeros, so
// the sum is the same sum over the full row.
struct FormantTable { float *tab = nullptr; int *kb = nullptr; int o = 0, n = 0, w = 0, Kt = 0; };
static inline void formant_table_compact(size_t o, size_t n, std::vector<float> &ht, std::vector<int> &kb, int *w_out, int *Kt_out)
{
    std::vector<float> h; size_t w, K;
    formant_table(o, n, h, &w, &K);
    kb.assign(n, 0);
    int Kt = 1;
    for (size_t j = 0; j < n; j++) {
        int a = -1, z = -1;
        for (size_t k = 0; k < K; k++) if (h[j * K + k] != 0.f) { if (a < 0) a = (int)k; z = (int)k; }
        if (a < 0) { a = 0; z = 0; }
        kb[j] = a;
        Kt = std::max(Kt, z - a + 1);
    }
    ht.assign(n * (size_t)Kt, 0.f);
    for (size_t j = 0; j < n; j++)
        for (int t = 0; t < Kt && (size_t)(kb[j] + t) < K; t++) ht[j * Kt + t] = h[j * K + kb[j] + t];
    *w_out = (int)w; *Kt_out = Kt;
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

// Back to the model rate, per stream from its descriptor (StreamState::f_*, so that the streams of one plan may differ and a captured
// graph stays valid when the shift changes): y[q n + j] = sum_t ht[j][t] x[q o + kb[j] + t - w], x = y2[0 : nx] and zero outside;
// an identity stream (upp_res = upp) copies y2[0 : N].  One thread per output sample.
static __global__ __launch_bounds__(256) void formant_resample_kernel(const float *x, long long xbs, float *y, long long ybs, int N, const StreamState *st)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const StreamState &s = st[b];
    const float *row = x + (long long)b * xbs;
    float *out = y + (long long)b * ybs;
    if (s.f_ident) { out[i] = row[i]; return; }
    const int n = s.f_n, q = i / n, j = i - q * n, Kt = s.f_kt, nx = s.f_nx;
    const float *h = s.f_tab + (long long)j * Kt;
    const int base = q * s.f_o + s.f_kb[j] - s.f_w;
    float acc = 0.f;
    for (int t = 0; t < Kt; t++) {
        const int k = base + t;
        const float v = (k >= 0 && k < nx) ? row[k] : 0.f;
        acc = fmaf(h[t], v, acc);
    }
    out[i] = acc;
}

}  // namespace rvc
