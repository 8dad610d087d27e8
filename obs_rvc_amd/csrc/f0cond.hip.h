// f0cond.hip.h -- per-stream conditioning of the f0 window inside the pitch tail (pitch_post_kernel, rmvpe.hip.h; DESIGN.md "Pitch controls"):
//   gate     a voiced row outside [lo, hi] Hz becomes unvoiced (0)
//   median   scipy.signal.medfilt(f, 2 r + 1), r <= 7: rows outside the window count as 0, unvoiced zeros take part as values
//   snap     n = 69 + 12 log2(f / 440); target = the nearest MIDI note whose pitch class is in the mask (a tie goes to the lower note);
//            f' = f 2^(s (target - n) / 12)
// The semitone transpose is no stage of its own: the host folds (float)2^(st / 12) into StreamCtl::uppower (engine.hip push_call_params).
// The stream's settings are four words of StreamState (StreamCtl::c); on == 0 = every control neutral, and the tail skips the stage on that one word.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include "state.hip.h"

namespace rvc {

constexpr double PITCH_SEMITONES_MAX = 24.0;
constexpr int F0_MEDIAN_MAX = 7;

// (F0Cond, the conditioning words as the host writes them: state.hip.h)
constexpr uint32_t F0C_GATE = 1u << 16;
static inline F0Cond f0cond_pack(float lo, float hi, int radius, uint32_t mask, float strength)
{
    F0Cond c{0u, 0.f, 0.f, 0.f};
    if (lo > 0.f || hi < INFINITY) { c.on |= F0C_GATE; c.lo = lo; c.hi = hi; }
    c.on |= (uint32_t)radius & 15u;
    if (mask != 0u && strength > 0.f) { c.on |= (mask & 0xFFFu) << 4; c.strength = strength; }
    return c;
}

__device__ __forceinline__ float f0cond_gate(float f, uint32_t on, float lo, float hi)
{
    return ((on & F0C_GATE) && f > 0.f && (f < lo || f > hi)) ? 0.f : f;
}

// Median of rows [row - r, row + r] of f[0 : Tm] (zero outside).  The window always has 15 slots: the 7 - r slots on either side that the radius
// leaves out hold -inf / +inf, so the rank-7 element of the 15 is the rank-r element of the 2 r + 1.  Pure selection: every element's rank under the
// total order (value, slot) is counted, and the one with rank 7 is returned as it was read.
__device__ __forceinline__ float f0cond_median(const float *f, int Tm, int row, int r)
{
    if (r == 0) return f[row];
    float v[15];
#pragma unroll
    for (int k = 0; k < 15; k++) {
        const int d = k - 7, i = row + d;
        v[k] = d < -r ? -INFINITY : (d > r ? INFINITY : ((i >= 0 && i < Tm) ? f[i] : 0.f));
    }
    float m = v[7];
#pragma unroll
    for (int i = 0; i < 15; i++) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 15; j++) rank += (v[j] < v[i] || (v[j] == v[i] && j < i)) ? 1 : 0;
        if (rank == 7) m = v[i];
    }
    return m;
}

__device__ __forceinline__ bool f0cond_allowed(uint32_t mask, int note)
{
    int pc = note % 12; pc += pc < 0 ? 12 : 0;
    return (mask >> pc) & 1u;
}

// m = n - 69 = 12 log2(f / 440) keeps the note number small (an ulp of n itself at n ~ 60 is 4e-6 semitones); the notes are searched as integers
__device__ __forceinline__ float f0cond_snap(float f, uint32_t mask, float s)
{
    if (!(f > 0.f) || mask == 0u) return f;
    const float m = 12.0f * log2f(f / 440.0f);
    const int base = (int)floorf(m) + 69;
    int below = base, above = base + 1;
    for (int k = 0; k < 12 && !f0cond_allowed(mask, below); k++) below--;
    for (int k = 0; k < 12 && !f0cond_allowed(mask, above); k++) above++;
    const float db = m - (float)(below - 69), da = (float)(above - 69) - m;      // both >= 0; the lower note wins a tie
    const float delta = db <= da ? -db : da;
    return f * exp2f(s * delta / 12.0f);
}

// steps 3-4 on the LDS-resident window of one stream; the caller has written the gated rows to f[] and passed a barrier
__device__ __forceinline__ float f0cond_row(const float *f, int Tm, int row, uint32_t on, float strength)
{
    return f0cond_snap(f0cond_median(f, Tm, row, (int)(on & 15u)), (on >> 4) & 0xFFFu, strength);
}

}  // namespace rvc
