// f0_hybrid.hip.h -- hybrid f0: up to four trackers run on the same audio, their unshifted f0 rows [B][Tm] (Hz on the common frame grid,
// 0 = unvoiced) are combined per stream and frame, and the combined row enters the unchanged pitch tail (pitch_post_kernel, rmvpe.hip.h) as its f0_in.  One
// kernel, one launch per chunk: RMVPE's salience decode as a stand-alone step (in the tail it exists only fused with the shift and the cache, and the tail must
// see the combined row, not RMVPE's), then the combination.  model_rmvpe.hip is the one unit that includes this header.
//
// A member is VOICED on a frame iff its value is > 0 (NaN and negative values are unvoiced).  With n members of which v are voiced:
//   RVC_HYBRID_VOTE    voiced iff 2 v > n, or 2 v == n and the lead (member 0) is voiced; an unvoiced frame gives 0, a voiced one the median of the v voiced values
//   RVC_HYBRID_MEDIAN  the median of all n values, unvoiced ones entering as 0 (the forks' plain median)
// The median of an even count is 0.5f * (a + b) of the two middle values, a <= b, in fp32.
#pragma once
#include <hip/hip_runtime.h>
#include "state.hip.h"

namespace rvc {

constexpr int HYBRID_MAX = 4;

struct HybridP {
    const float *row[HYBRID_MAX];   // member rows [B][Tm] in the caller's order, row[0] the lead's; the RMVPE member's entry is not read (its row is decoded here)
    int n, mode, Tm;
    int rm_at;                      // RMVPE's place among the members, -1 = not a member: no decode, sal is not read
    const float *sal; int sal_cs; long long sal_bs;   // RMVPE's salience [B][360][ld] (channel-major)
    float threshold;                // RMVPE's salience threshold (0.03, rvc.rs:122)
    StreamState *st;                // status words (ST_PANIC of the decode)
    float *rm_f0;                   // [B][Tm] RMVPE's decoded row, unshifted (null: not stored)
    float *out;                     // [B][Tm] the combined row
};

// the median of s[0 .. c) of four ascending values (c in 1 .. 4); selects, no indexing: the values stay in registers
static __device__ __forceinline__ float hybrid_median4(float s0, float s1, float s2, float s3, int c)
{
    const float lo = c <= 2 ? s0 : s1;                        // s[(c - 1) / 2]
    const float hi = c == 1 ? s0 : (c == 4 ? s2 : s1);        // s[c / 2]: c = 2 -> s1, c = 3 -> s1, c = 4 -> s2
    return (c & 1) ? hi : 0.5f * (lo + hi);
}

// One workgroup per stream.  With RMVPE among the members the launch has 1024 threads and the decode is pitch_post_kernel's, step for step and in its operation
// order: the bin scan of the zero-padded row split over bin groups ("first strictly greater wins"), the 9-bin weighted cents, the threshold behind the gather,
// 10 * 2^(cents / 1200), 10 -> 0; start + 8 >= 360 raises ST_PANIC on the stream.  Without RMVPE the launch has a thread per frame (rounded up to a wave) and
// no shared memory is touched.  Either way thread tt < Tm then combines the members' values of frame tt: at most four values, sorted by a five-exchange network.
static __global__ __launch_bounds__(1024) void f0_hybrid_kernel(HybridP p)
{
    __shared__ float bests[1024];
    __shared__ float maxes[1024];
    __shared__ int idxs[1024];
    const int b = blockIdx.x, t = threadIdx.x;
    float rm_hz = 0.f;
    if (p.rm_at >= 0) {
        int TT = 1; while (TT < p.Tm) TT <<= 1;
        TT = TT < 1024 ? TT : 1024;
        const int NG = 1024 / TT, BPG = (360 + NG - 1) / NG, tt = t & (TT - 1), grp = t / TT;
        {
            float best = 0.f, mx = -INFINITY; int start = 0;
            if (tt < p.Tm) {
                const float *col = p.sal + (long long)b * p.sal_bs + tt;
                const int i0 = grp * BPG, i1 = (i0 + BPG < 360) ? i0 + BPG : 360;
#pragma unroll 4
                for (int i = i0; i < i1; i++) { const float v = col[(long long)i * p.sal_cs]; if (v > best) { best = v; start = i + 4; } mx = fmaxf(mx, v); }
            }
            bests[t] = best; maxes[t] = mx; idxs[t] = start;
        }
        __syncthreads();
        if (grp == 0 && tt < p.Tm) {
            const float *col = p.sal + (long long)b * p.sal_bs + tt;
            int start = 0; float best = 0.f, mx = -INFINITY;
            for (int g = 0; g < NG; g++) {
                const float v = bests[g * TT + tt];
                if (v > best) { best = v; start = idxs[g * TT + tt]; }
                mx = fmaxf(mx, maxes[g * TT + tt]);
            }
            float hz = 0.f;
            if (start + 8 >= 360) { atomicOr(&p.st[b].status, (int)ST_PANIC); }
            else {
                float sv[9];
#pragma unroll
                for (int y = 0; y < 9; y++) sv[y] = col[(long long)(start + y) * p.sal_cs];
                float ps = 0.f, ws = 0.f;
#pragma unroll
                for (int y = 0; y < 9; y++) { const float cm = ((float)(start + y) - 4.f) * 20.f + 1997.3794084376191f; ps += sv[y] * cm; ws += sv[y]; }
                float cents = ps / ws;
                if (!(mx > p.threshold)) cents = 0.f;
                hz = 10.0f * powf(2.0f, cents / 1200.0f);
                if (hz == 10.0f) hz = 0.f;
            }
            rm_hz = hz;
            if (p.rm_f0) p.rm_f0[(long long)b * p.Tm + tt] = hz;
        }
        if (grp != 0) return;      // (no barrier follows)
    }
    if (t >= p.Tm) return;
    const long long at = (long long)b * p.Tm + t;
    // the members' values, unvoiced ones replaced: by +inf in VOTE (they sort behind the v voiced values) and by 0 in MEDIAN; places past n hold +inf in both
    float x[HYBRID_MAX]; int v = 0; bool lead = false;
#pragma unroll
    for (int i = 0; i < HYBRID_MAX; i++) {
        float f = INFINITY;
        if (i < p.n) {
            f = i == p.rm_at ? rm_hz : p.row[i][at];
            const bool voiced = f > 0.f;
            v += voiced ? 1 : 0;
            if (i == 0) lead = voiced;
            if (!voiced) f = p.mode == 0 ? INFINITY : 0.f;
        }
        x[i] = f;
    }
    // ascending order by five compare-exchanges (no NaN is left among the values: fminf / fmaxf are exact selections)
#define RVC_HYBRID_CX(i, j) { const float lo = fminf(x[i], x[j]), hi = fmaxf(x[i], x[j]); x[i] = lo; x[j] = hi; }
    RVC_HYBRID_CX(0, 1) RVC_HYBRID_CX(2, 3) RVC_HYBRID_CX(0, 2) RVC_HYBRID_CX(1, 3) RVC_HYBRID_CX(1, 2)
#undef RVC_HYBRID_CX
    float r;
    if (p.mode == 0) {
        const bool on = 2 * v > p.n || (2 * v == p.n && lead);
        r = on ? hybrid_median4(x[0], x[1], x[2], x[3], v) : 0.f;      // (on implies v >= 1)
    } else {
        r = hybrid_median4(x[0], x[1], x[2], x[3], p.n);
    }
    p.out[at] = r;
}

}  // namespace rvc
