// f0_override.hip.h -- f0 from outside, included by engine.hip: the grid of a recording's f0 curve, and the select of a tracker's rows
// against override rows in front of the pitch tail.  (The export of a conversion's conditioned f0 onto the 10 ms grid: windows.hip.h f0_export_many_kernel.)
// Plain vector loads and stores, no LDS, no atomics.  The definition is tests/f0_override_ref.py; the operation order below is part of it.
#pragma once
#include "f0_override.h"
#include <hip/hip_runtime.h>

namespace rvc {

// breakpoints (t seconds as double, hz) -> grid [Nf], row j = time j / 100 s, NaN = "keep the tracker's value".  One thread per row, binary search for the last
// breakpoint at or in front of the row.  Times are compared as T_i = 100 t_i, one rounded double product (never contracted with the subtraction behind it);
// a pitch never glides into 0: next to an unvoiced breakpoint the row is the nearer breakpoint's value, a tie goes to the earlier one; between two voiced
// breakpoints u = (float)(j - T_i) / (float)(T_i+1 - T_i) and the row is ONE fma, hz_i + (hz_i+1 - hz_i) u
static __global__ __launch_bounds__(256) void f0_curve_grid_kernel(const double *__restrict__ t, const float *__restrict__ hz, int n, float *__restrict__ grid, long long Nf)
{
#pragma clang fp contract(off)      // (the order above is the definition: no product is fused with the compare or the subtraction behind it)
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= Nf) return;
    const double x = (double)j;
    float v = __builtin_nanf("");
    if (n >= 1 && 100.0 * t[0] <= x && x <= 100.0 * t[n - 1]) {
        int lo = 0, hi = n - 1;          // invariant: T_lo <= x; the answer is in [lo, hi]
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (100.0 * t[mid] <= x) lo = mid; else hi = mid - 1;
        }
        const int i = lo;
        const float h0 = hz[i];
        if (i == n - 1) v = h0;
        else {
            const float h1 = hz[i + 1];
            const double T0 = 100.0 * t[i], T1 = 100.0 * t[i + 1];
            const double a = x - T0, b = T1 - x;
            if (h0 == 0.f || h1 == 0.f) v = a <= b ? h0 : h1;
            else {
                const float u = (float)a / (float)(T1 - T0);
                v = __builtin_fmaf(h1 - h0, u, h0);
            }
        }
    }
    grid[j] = v;
}

// out[b][t] = isnan(ov) ? f[b][t] : ov, pure selection.  Grid (ceil(Tm / 256), B).  map: the engine stream of the plan's stream b (a bucket plan), or null.
// mode 0: stream s has cnt[s] override rows in rows[s][0 .. cnt), aligned to the END of the window: row i of n is window row Tm - n + i, the window rows in
// front of them keep the tracker's value.  mode 1: gathered from the conversion's grid, see F0OvCall
static __global__ __launch_bounds__(256) void f0_override_kernel(const float *__restrict__ f, float *__restrict__ out, int Tm, const F0OvCall *__restrict__ call,
                                                                 const int *__restrict__ cnt, const float *__restrict__ rows, const int *__restrict__ map)
{
    const int tt = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (tt >= Tm) return;
    const F0OvCall c = *call;
    const int s = map ? map[b] : b;
    float o = __builtin_nanf("");
    if (c.mode == 1) {
        if (s < c.nw) {
            const long long g = (long long)(c.list ? c.list[c.w0 + s] : c.w0 + s) * c.H - c.C + tt;
            if (g >= 0 && g < c.Nf) o = c.grid[g];
        }
    } else {
        const int n = cnt[s], i = tt - (Tm - n);
        if (n > 0 && n <= F0_OV_ROWS && i >= 0 && i < n) o = rows[(long long)s * F0_OV_ROWS + i];
    }
    const float v = f[(long long)b * Tm + tt];
    out[(long long)b * Tm + tt] = o != o ? v : o;
}

}  // namespace rvc
