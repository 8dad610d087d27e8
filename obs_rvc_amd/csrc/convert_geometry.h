// convert_geometry.h -- the host-only arithmetic of the file converter: window geometry, argument checks and the high-pass taps.
// Plain C++, no HIP: rvc_convert_geometry and rvc_convert call it, and tests/tools/convert_host_check.cpp compiles it on its own under the sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace rvc {

// Everything in frames of 10 ms (160 samples at 16 kHz, zc = sample_rate / 100 at the model rate).  One window = one infer call:
//   F  = 32 k - 1                 frames per window; n = 160 F input samples
//   sf = 5120 (k - 1)             sample_frame_16k_size: the f0 front end's fr = 5120 ((sf + 799) / 5120 + 1) - 160 (rmvpe.rs:256) is then n,
//                                 Tm = 1 + fr / 160 = 32 k <= 1024, ContentVec yields T = 16 k - 1 frames and hubert_length = 2 T + 1 = F (rvc.rs:153)
//   skip_head = C, H = F - 2 C - X - Q, return_length = H + X + Q     (Q = 1: the plugin's 10 ms SOLA search)
// Pitch cache (rvc.rs:168-179): shifted by sf / 160, f0 rows [3, Tm - 1) stored at [1028 - Tm, 1024) -- the last 32 k - 4 = F - 3 entries -- and the call
// reads [1024 - F + C, 1024 - C).  With C >= 3 every row a window reads was computed from that window.
struct ConvertGeometry {
    size_t k = 0, C = 0, X = 0, Q = 1;
    size_t F = 0, n = 0, sf = 0, skip_head = 0, return_length = 0, H = 0, zc = 0;
    size_t Nf = 0, windows = 0, out_samples = 0;
};
constexpr size_t CONVERT_MAX_FRAMES = (size_t)1 << 40;      // far beyond any recording; keeps every product below in 64 bits

// The default window: with C = 48 a window returns 32 k - 97 frames, and the synthesizer's text-encoder attention keeps K and V of a head in LDS (plan.hip
// add_relpos_attention: (112 R + 1536) floats at RVC's head size 96, 160 KB) -- at most 351 frames, which is k = 14 exactly; k = 16 would ask for 415
constexpr size_t CONVERT_DEFAULT_K = 14;
// -> nullptr, or what is wrong with the arguments (k, C, X: 0 = the default 14 / 48 / 5)
static inline const char *convert_geometry(size_t n16k, size_t sample_rate, size_t k, size_t context, size_t crossfade, ConvertGeometry *g)
{
    if (k == 0) k = CONVERT_DEFAULT_K;
    if (context == 0) context = 48;
    if (crossfade == 0) crossfade = 5;
    if (k < 2 || k > 32) return "convert: the window size k is outside [2, 32]";
    if (context < 3) return "convert: the context must be at least 3 frames (the pitch rows of a window must be its own)";
    if (sample_rate == 0 || sample_rate % 100 != 0 || sample_rate > 384000) return "convert: the model's sample rate is not a multiple of 100";
    g->k = k; g->C = context; g->X = crossfade; g->Q = 1;
    g->F = 32 * k - 1; g->n = 160 * g->F; g->sf = 5120 * (k - 1); g->skip_head = context; g->zc = sample_rate / 100;
    // H = F - 2 C - X - Q >= X, written without a negative intermediate (F <= 1023 bounds the accepted context and crossfade)
    if (context > g->F || crossfade > g->F || 2 * context + 2 * crossfade + g->Q > g->F) return "convert: hop = F - 2 context - crossfade - 1 is shorter than the crossfade";
    g->H = g->F - 2 * context - crossfade - g->Q;
    g->return_length = g->H + crossfade + g->Q;
    if (g->Q * g->zc > 1023) return "convert: the SOLA search (one frame of the model rate) is longer than 1023 samples";
    g->Nf = n16k / 160 + (n16k % 160 != 0);
    if (g->Nf > CONVERT_MAX_FRAMES) return "convert: recording too long";
    g->windows = g->Nf / g->H + (g->Nf % g->H != 0);
    g->out_samples = g->Nf * g->zc;
    return nullptr;
}

// the high-pass taps h[2 M + 1] (highpass.hip.h): fp64 throughout, rounded once
constexpr int HP_M = 1024;
static inline std::vector<float> highpass_taps()
{
    const int M = HP_M, L = 2 * M + 1;
    const double fc = 48.0 / 16000.0, pi = 3.14159265358979323846;
    std::vector<double> lp(L);
    double sum = 0.0;
    for (int j = 0; j < L; j++) {
        const double a = 2.0 * fc * (double)(j - M) * pi;
        const double sinc = j == M ? 1.0 : sin(a) / a;
        const double w = 0.42 - 0.5 * cos(2.0 * pi * (double)j / (double)(2 * M)) + 0.08 * cos(4.0 * pi * (double)j / (double)(2 * M));
        lp[j] = 2.0 * fc * sinc * w;
        sum += lp[j];
    }
    std::vector<float> h(L);
    for (int j = 0; j < L; j++) h[j] = (float)((j == M ? 1.0 : 0.0) - lp[j] / sum);
    return h;
}

}  // namespace rvc
