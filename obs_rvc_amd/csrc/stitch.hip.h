// stitch.hip.h -- the file converter's stitch (DESIGN.md sections 19 and 29): the plugin's SOLA step (chunk.hip.h post_sola_corr_kernel + post_sola_kernel,
// LINEAR crossfade) chained over the windows of every recording of a call, as two launches per batch of windows.  Included by engine.hip only, behind
// chunk.hip.h, whose correlation, arg-max and fade (sola_corr_lag, sola_argmax_last, sola_fade) both kernels call: the chain picks the offsets rvc_sola_step
// picks and the assembly produces its samples, bit for bit.  A single recording is a call of one file (F = 1: one chain workgroup, many_file_of returns 0).
//
// A step's saved tail is output[off + frame .. + sola_len) AFTER the blend has been written over output[off .. + sola_len); with frame >= sola_len
// (the converter's H >= X) the two ranges do not meet and the tail is the window's raw samples.  That is what takes the blend off the serial path:
// only the offsets depend on the window before, the samples do not.
//   tabs     the device tables of the call (convert_many_geometry.h ManyTables); the stitch reads P, out_off and out_n
//   tails    [Wtot + 1][sola_len]   row 0 stays zero: what the FIRST window of every file is correlated and blended with; row g + 1 = the tail global
//            window g leaves, which window g + 1 reads if it belongs to the same file
//   offsets  [Wtot], in global window order
#pragma once
#include "convert_many_geometry.h"

namespace rvc {

constexpr int STITCH_CHAIN_THREADS = 1024;      // 16 waves, one lag each per round
constexpr int STITCH_TILE = 1024;               // samples of a window's frame per workgroup of stitch_assemble_many_kernel

// Offset chains, one per FILE, side by side: workgroup b walks the windows file f_first + b has among globals [g0, g0 + nw), in order; y [nw][y_bs] holds the
// batch's model outputs (global g at y + (g - g0) y_bs, search + frame + sola_len valid samples each).  Per window: the search + 1 normalised
// cross-correlations against the tail in front of it, one wave per lag, the arg-max (last maximum wins), then the raw tail into row g + 1.  A file's first
// window meets the zero tail (row 0), a window that continues a file from the batch before meets the row that batch left behind.  Workgroups touch disjoint
// rows of tails and offsets.  search <= 1023 (the LDS array).
static __global__ __launch_bounds__(STITCH_CHAIN_THREADS) void stitch_chain_many_kernel(const float *y, long long y_bs, int g0, int nw, int f_first, ManyTables tabs, int sola_len,
                                                                                        int search, int frame, float *tails, int *offsets)
{
    __shared__ float cor[1024];
    __shared__ int s_off;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int f = f_first + blockIdx.x;
    if (f >= tabs.n_files) return;
    const int p0 = tabs.P[f], lo = max(p0, g0), hi = min(tabs.P[f + 1], g0 + nw);
    for (int g = lo; g < hi; g++) {
        const float *yw = y + (long long)(g - g0) * y_bs;
        const float *prev = g == p0 ? tails : tails + (long long)g * sola_len;
        float *next = tails + (long long)(g + 1) * sola_len;
        for (int l = wave; l <= search; l += STITCH_CHAIN_THREADS / 64) {
            const float c = sola_corr_lag(yw + l, prev, sola_len, lane);
            if (lane == 0) cor[l] = c;
        }
        __syncthreads();
        if (t == 0) { const int best = sola_argmax_last(cor, search); s_off = best; offsets[g] = best; }
        __syncthreads();
        const float *o = yw + s_off;
        for (int i = t; i < sola_len; i += STITCH_CHAIN_THREADS) next[i] = o[frame + i];
        // the file's next window reads `next` (global memory written by this workgroup) and overwrites cor / s_off
        __threadfence_block();
        __syncthreads();
    }
}

// Assembly: grid (tiles of a frame, nw).  Global window g = g0 + blockIdx.y = window w of file f: its `frame` samples from its offset on, the first sola_len
// of them blended with the tail in front of it by the sin^2 fade, written to out[out_off[f] + w frame ..); samples at or beyond out_n[f] (the file's last,
// partial hop) are not written, so nothing lands in the next file's region
static __global__ __launch_bounds__(256) void stitch_assemble_many_kernel(const float *y, long long y_bs, int g0, ManyTables tabs, int sola_len, int frame, const float *tails,
                                                                          const int *offsets, float *out)
{
    const int j = blockIdx.y, g = g0 + j, f = many_file_of(tabs.P, tabs.n_files, g), w = g - tabs.P[f];
    const float *o = y + (long long)j * y_bs + offsets[g];
    const float *prev = w == 0 ? tails : tails + (long long)g * sola_len;
    const long long base = (long long)w * frame, n_out = tabs.out_n[f];
    float *dst = out + tabs.out_off[f];
    const int i0 = blockIdx.x * STITCH_TILE;
    for (int i = i0 + threadIdx.x; i < i0 + STITCH_TILE && i < frame; i += 256) {
        if (base + i >= n_out) break;
        dst[base + i] = i < sola_len ? sola_fade(o[i], prev[i], i, sola_len) : o[i];
    }
}

// the two stitch launches for globals [g0, g0 + nw), which lie in files [f_first, f_last]
static void launch_stitch_many(hipStream_t st, const float *y, long long y_bs, int g0, int nw, int f_first, int f_last, const ManyTables &tabs, int sola_len, int search, int frame,
                               float *tails, int *offsets, float *out)
{
    hipLaunchKernelGGL(stitch_chain_many_kernel, dim3((unsigned)(f_last - f_first + 1)), dim3(STITCH_CHAIN_THREADS), 0, st, y, y_bs, g0, nw, f_first, tabs, sola_len, search, frame, tails,
                       offsets);
    hipLaunchKernelGGL(stitch_assemble_many_kernel, dim3((unsigned)((frame + STITCH_TILE - 1) / STITCH_TILE), (unsigned)nw), dim3(256), 0, st, y, y_bs, g0, tabs, sola_len, frame,
                       (const float *)tails, (const int *)offsets, out);
}

}  // namespace rvc
