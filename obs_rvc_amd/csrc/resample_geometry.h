// resample_geometry.h -- the host-only arithmetic of the whole-signal sample-rate converter and of the whole-file volume envelope:
// ratio, filter width, output length, argument checks.  Plain C++, no HIP: rvc_resample_geometry, rvc_resample and rvc_change_rms call it, and
// tests/tools/resample_host_check.cpp compiles it on its own under the sanitizers.
#pragma once
#include "formant_table.h"

namespace rvc {

// g = gcd(rate_in, rate_out), o = rate_in / g, n = rate_out / g; b = 0.99 min(o, n), w = ceil(6 o / b), K = 2 w + o (formant_table's);
// n_out = ceil(n_in n / o);  y[i n + j] = sum_{k < K} h[j][k] x[i o + k - w], x zero outside [0, n_in)
struct ResampleGeometry { size_t o = 0, n = 0, w = 0, K = 0, n_out = 0; };
constexpr size_t RESAMPLE_MAX_RATIO = 2048;                  // o and n: the full table is n K floats on the host
constexpr size_t RESAMPLE_MAX_SAMPLES = (size_t)1 << 40;     // as the file converter's: keeps every product below in 64 bits

// -> nullptr, or what is wrong with the arguments
static inline const char *resample_geometry(size_t rate_in, size_t rate_out, size_t n_in, ResampleGeometry *g)
{
    if (rate_in == 0 || rate_out == 0) return "resample: a sample rate of 0";
    const size_t d = formant_gcd(rate_in, rate_out);
    g->o = rate_in / d; g->n = rate_out / d;
    if (g->o > RESAMPLE_MAX_RATIO || g->n > RESAMPLE_MAX_RATIO) return "resample: the reduced ratio has a term above 2048";
    if (n_in == 0) return "resample: empty signal";
    if (n_in > RESAMPLE_MAX_SAMPLES) return "resample: signal too long";
    const double b = 0.99 * (double)(g->o < g->n ? g->o : g->n);
    g->w = (size_t)std::ceil(6.0 * (double)g->o / b);
    g->K = 2 * g->w + g->o;
    const size_t p = n_in * g->n;
    g->n_out = p / g->o + (p % g->o != 0);
    return nullptr;
}

// The volume envelope (upstream's change_rms): signal s at rate sr has RMS frames of L = 2 (sr / 2) samples every hop = sr / 2, F = 1 + N / hop of them over
// the signal zero-padded by L / 2 on both sides.
struct RmsGeometry { size_t L = 0, hop = 0, F = 0; };
constexpr size_t CHANGE_RMS_MAX_RATE = (size_t)1 << 20, CHANGE_RMS_MAX_SAMPLES = (size_t)1 << 30;      // frame, hop and sample indices are ints in post_rms_kernel
static inline const char *change_rms_geometry(size_t n, size_t rate, RmsGeometry *g)
{
    if (rate < 2) return "change_rms: a sample rate below 2";
    if (rate > CHANGE_RMS_MAX_RATE) return "change_rms: a sample rate above 2^20";
    if (n == 0) return "change_rms: empty signal";
    if (n > CHANGE_RMS_MAX_SAMPLES) return "change_rms: signal longer than 2^30 samples";
    g->hop = rate / 2; g->L = 2 * g->hop; g->F = 1 + n / g->hop;
    return nullptr;
}
static inline bool change_rms_rate_ok(double rate) { return rate >= 0.0 && rate <= 1.0; }      // (false for NaN)

}  // namespace rvc
