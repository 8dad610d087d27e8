// stitch.hip.h -- the file converter's stitch: the plugin's SOLA step (chunk.hip.h post_sola_corr_kernel + post_sola_kernel, LINEAR
// crossfade) chained over the windows of a recording, as two launches per batch of windows.  Included by engine.hip only, behind chunk.hip.h, whose
// correlation, arg-max and fade (sola_corr_lag, sola_argmax_last, sola_fade) both kernels call: the chain picks the offsets rvc_sola_step picks and
// the assembly produces its samples, bit for bit.
//
// A step's saved tail is output[off + frame .. + sola_len) AFTER the blend has been written over output[off .. + sola_len); with frame >= sola_len
// (the converter's H >= X) the two ranges do not meet and the tail is the window's raw samples.  That is what takes the blend off the serial path:
// only the offsets depend on the window before, the samples do not.
//   tails   [n_windows + 1][sola_len]   tails[w] = the tail window w is correlated and blended with (tails[0]: zeros), tails[w + 1] = the tail it leaves
//   offsets [n_windows]
#pragma once

namespace rvc {

constexpr int STITCH_CHAIN_THREADS = 1024;      // 16 waves, one lag each per round
constexpr int STITCH_TILE = 1024;               // samples of a window's frame per workgroup of stitch_assemble_kernel

// Offset chain: ONE workgroup walks windows [w0, w0 + nw) of the file in order; y [nw][y_bs] holds their model outputs (window w0 + j at y + j y_bs,
// search + frame + sola_len valid samples each).  Per window: the search + 1 normalised cross-correlations against tails[w], one wave per lag, the
// arg-max (last maximum wins), then the raw tail into tails[w + 1].  search <= 1023 (the LDS array).
static __global__ __launch_bounds__(STITCH_CHAIN_THREADS) void stitch_chain_kernel(const float *y, long long y_bs, int w0, int nw, int sola_len, int search, int frame,
                                                                                   float *tails, int *offsets)
{
    __shared__ float cor[1024];
    __shared__ int s_off;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int j = 0; j < nw; j++) {
        const float *yw = y + (long long)j * y_bs;
        const float *prev = tails + (long long)(w0 + j) * sola_len;
        float *next = tails + (long long)(w0 + j + 1) * sola_len;
        for (int l = wave; l <= search; l += STITCH_CHAIN_THREADS / 64) {
            const float c = sola_corr_lag(yw + l, prev, sola_len, lane);
            if (lane == 0) cor[l] = c;
        }
        __syncthreads();
        if (t == 0) { const int best = sola_argmax_last(cor, search); s_off = best; offsets[w0 + j] = best; }
        __syncthreads();
        const float *o = yw + s_off;
        for (int i = t; i < sola_len; i += STITCH_CHAIN_THREADS) next[i] = o[frame + i];
        // the next window's correlations read `next` (global memory written by this workgroup) and overwrite cor / s_off
        __threadfence_block();
        __syncthreads();
    }
}

// Assembly: grid (tiles of a frame, nw).  Window w = w0 + blockIdx.y: its `frame` samples from its offset on, the first sola_len of them blended with
// tails[w] by the sin^2 fade, written to out[w frame ..); samples at or beyond n_out (the file's last, partial hop) are not written.
static __global__ __launch_bounds__(256) void stitch_assemble_kernel(const float *y, long long y_bs, int w0, int sola_len, int frame, const float *tails,
                                                                     const int *offsets, float *out, long long n_out)
{
    const int j = blockIdx.y, w = w0 + j;
    const float *o = y + (long long)j * y_bs + offsets[w];
    const float *prev = tails + (long long)w * sola_len;
    const long long base = (long long)w * frame;
    const int i0 = blockIdx.x * STITCH_TILE;
    for (int i = i0 + threadIdx.x; i < i0 + STITCH_TILE && i < frame; i += 256) {
        if (base + i >= n_out) break;
        out[base + i] = i < sola_len ? sola_fade(o[i], prev[i], i, sola_len) : o[i];
    }
}

}  // namespace rvc
