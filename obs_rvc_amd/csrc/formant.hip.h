// formant.hip.h -- formant shift (the plugin's resonance shift, obs-rvc/src/lib.rs:80,103,176,369-375,446-451): geometry and the
// windowed-sinc filter table of the synthesizer's formant stage (DESIGN.md "Formant shift"; host code only, the two kernels: synth.hip.h).
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

}  // namespace rvc
