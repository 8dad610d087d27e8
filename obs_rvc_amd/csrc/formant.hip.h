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
#include "formant_table.h"

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

// (FormantDesc, a stream's descriptor of the stage: state.hip.h)
// Device form of a table: row j keeps only its span of nonzero fp32 taps, [kb[j], kb[j] + Kt).  The taps left out are exact zeros, so
// the sum is the same sum over the full row.
struct FormantTable { float *tab = nullptr; int *kb = nullptr; int o = 0, n = 0, w = 0, Kt = 0; };
}  // namespace rvc
