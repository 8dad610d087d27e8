// formant_table.h -- the Hann-windowed sinc filter table (width 6, rolloff 0.99) of the formant stage's resampler (formant.hip.h) and of the whole-signal
// converter (resample_whole.hip.h), in its full and its compact form.  Plain C++, no HIP: tests/tools/resample_host_check.cpp compiles it on its own under
// the sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace rvc {

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

// Compact form of a table: row j keeps only its span of nonzero fp32 taps, [kb[j], kb[j] + Kt).  The taps left out are exact zeros, so
// the sum is the same sum over the full row.
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
