// silence.hip.h -- the file converter's silence gate (the upstream client's response threshold, slicer2's job), included by windows.hip.h
// (engine.hip's unit), whose gather and f0 export read the gate's win_of list.  The definition is tests/silence_ref.py.
//
// With rvc_set_convert_silence in force a conversion measures the signal the model will see first and runs only the windows that hold something:
//   loud[i]    frame i (10 ms, 160 samples) whose 40 ms of signal from its start on reach the threshold: sumsq(x[160 i, 160 i + 640)) >= 640 thr, fp64
//   kept[i]    a loud frame lies within `hang` frames of i
//   active[w]  a kept frame lies in the frames window w returns, [w H, w H + H + X + Q) n [0, Nf)
//   place[w]   the rank of w among the active windows, -1 for a skipped one;  win_of[place[w]] = w
// The active windows run compacted -- the j-th of them on stream j % S of batch j / S, across files in rvc_convert_many -- and a skipped window enters the stitch
// as a window of zeros.  Everything is decided on the device; the host reads three counters once per call (the active count sizes the batch loop).
// Every fp64 sum has a fixed order: 160 samples by one wave (lane l adds samples l, l + 64, l + 128, then the xor butterfly of reduce.hip.h), four block sums
// left to right.  The counts are integers.  None of these kernels is launched while the gate is off.
#pragma once
#include "convert_many_geometry.h"
#include "stitch.hip.h"

namespace rvc {

constexpr int SILENCE_SCAN_THREADS = 1024;
constexpr int SILENCE_MAX_HANG = 1000;
constexpr double SILENCE_OFF_DB = -60.0;                         // at or below: the gate is off (the session gate's convention)
constexpr long long SILENCE_MAX_FRAMES = (1LL << 31) - 1025;     // the prefix counts are ints, and a scan round may look 1023 past the end

// 640 thr in the linear domain: frame i is loud iff its 640-sample sum of squares reaches this
static inline double silence_threshold(double threshold_db) { return 640.0 * std::max(std::pow(10.0, threshold_db / 10.0), 1e-10); }

// bs[b] = sum of squares of block b = x[160 b, 160 b + 160), zero beyond N; one wave per block, 4 per workgroup
static __global__ __launch_bounds__(256) void silence_block_kernel(const float *__restrict__ sig, long long N, long long Nf, double *__restrict__ bs)
{
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= Nf) return;      // (the whole wave)
    double s = 0.0;
    for (int j = lane; j < 160; j += 64) {
        const long long q = 160 * b + j;
        const double v = q < N ? (double)sig[q] : 0.0;
        s += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) bs[b] = s;
}

// inclusive scan of one flag per thread over the workgroup (SILENCE_SCAN_THREADS threads); *total: the flags of the whole round.  ws: 16 ints of LDS
__device__ __forceinline__ int silence_scan_round(int flag, int *ws, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int v = flag;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
    __syncthreads();      // (the round before has read ws)
    if (lane == 63) ws[wave] = v;
    __syncthreads();
    int pre = 0, tot = 0;
    for (int k = 0; k < SILENCE_SCAN_THREADS / 64; k++) { const int x = ws[k]; tot += x; if (k < wave) pre += x; }
    *total = tot;
    return pre + v;
}

// loud[i] and its inclusive prefix count cnt[i] over the Nf frames of one recording: ONE workgroup walks the frames 1024 at a time and carries the count.
// counts[1] += the recording's loud frames
static __global__ __launch_bounds__(SILENCE_SCAN_THREADS) void silence_loud_scan_kernel(const double *__restrict__ bs, long long Nf, double thr, unsigned char *__restrict__ loud,
                                                                                        int *__restrict__ cnt, unsigned long long *counts)
{
    __shared__ int ws[SILENCE_SCAN_THREADS / 64];
    int carry = 0;
    for (long long base = 0; base < Nf; base += SILENCE_SCAN_THREADS) {
        const long long i = base + threadIdx.x;
        int f = 0;
        if (i < Nf) {
            double s = bs[i];
            for (int k = 1; k < 4; k++) s += i + k < Nf ? bs[i + k] : 0.0;
            f = s >= thr;
            loud[i] = (unsigned char)f;
        }
        int tot;
        const int inc = silence_scan_round(f, ws, &tot);
        if (i < Nf) cnt[i] = carry + inc;
        carry += tot;
    }
    if (threadIdx.x == 0) atomicAdd(&counts[1], (unsigned long long)carry);
}

// loud frames in [a, b] n [0, Nf) from the inclusive prefix count (a may be negative, b beyond the end; b >= 0)
__device__ __forceinline__ int silence_loud_in(const int *cnt, long long Nf, long long a, long long b)
{
    return cnt[b < Nf - 1 ? b : Nf - 1] - (a > 0 ? cnt[a - 1] : 0);
}

// kept[i] = a loud frame within hang of i; counts[2] += the recording's kept frames (one integer atomic per wave)
static __global__ __launch_bounds__(256) void silence_kept_kernel(const int *__restrict__ cnt, long long Nf, int hang, unsigned char *__restrict__ kept, unsigned long long *counts)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int k = 0;
    if (i < Nf) { k = silence_loud_in(cnt, Nf, i - hang, i + hang) > 0; kept[i] = (unsigned char)k; }
    const unsigned long long m = __ballot(k);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&counts[2], (unsigned long long)__popcll(m));
}

// active[w] for the Wf windows of one recording: a kept frame in [w H, min(w H + R, Nf)), that is a loud frame within hang of that range
static __global__ __launch_bounds__(256) void silence_active_kernel(const int *__restrict__ cnt, long long Nf, int hang, int H, int R, int Wf, int *__restrict__ active)
{
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= Wf) return;
    const long long lo = (long long)w * H, hi = (lo + R < Nf ? lo + R : Nf) - 1;
    active[w] = silence_loud_in(cnt, Nf, lo - hang, hi + hang) > 0;
}

// the compaction over the W windows of the call (global window order): place[w] = exclusive count of active windows in front of w, or -1; win_of[place[w]] = w;
// counts[0] = the active count.  One workgroup, as the loud scan
static __global__ __launch_bounds__(SILENCE_SCAN_THREADS) void silence_compact_kernel(const int *__restrict__ active, int W, int *__restrict__ place, int *__restrict__ win_of,
                                                                                      unsigned long long *counts)
{
    __shared__ int ws[SILENCE_SCAN_THREADS / 64];
    int carry = 0;
    for (long long base = 0; base < W; base += SILENCE_SCAN_THREADS) {
        const long long w = base + threadIdx.x;
        const int f = w < W ? active[w] != 0 : 0;
        int tot;
        const int inc = silence_scan_round(f, ws, &tot);
        if (w < W) {
            const int p = carry + inc - 1;
            place[w] = f ? p : -1;
            if (f) win_of[p] = (int)w;
        }
        carry += tot;
    }
    if (threadIdx.x == 0) counts[0] = (unsigned long long)carry;
}

// the global windows a compacted batch completes: those behind the last active window of the batch before, up to its own last active window -- and up to the
// end of the call for the last batch (j0 + nw >= A; with A = 0 one launch of j0 = nw = 0 covers everything)
__device__ __forceinline__ void silence_batch_range(const int *win_of, int j0, int nw, int A, int W, int *lo, int *hi)
{
    *lo = j0 == 0 ? 0 : win_of[j0 - 1] + 1;
    *hi = j0 + nw >= A ? W : win_of[j0 + nw - 1] + 1;
}

// stitch_chain_many_kernel over a range that contains skipped windows: the same walk, a skipped window read from `zero` (search + frame + sola_len zeros)
// instead of a row of y; y [nw][y_bs] holds the batch's outputs, active window g at row place[g] - j0.  Workgroup b takes files f_first + b, + gridDim.x, ..
static __global__ __launch_bounds__(STITCH_CHAIN_THREADS) void stitch_chain_gated_kernel(const float *y, long long y_bs, const float *zero, const int *__restrict__ place,
                                                                                         const int *__restrict__ win_of, int j0, int nw, int A, int W, ManyTables tabs, int sola_len,
                                                                                         int search, int frame, float *tails, int *offsets)
{
    __shared__ float cor[1024];
    __shared__ int s_off;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int g_lo, g_hi;
    silence_batch_range(win_of, j0, nw, A, W, &g_lo, &g_hi);
    const int f_first = many_file_of(tabs.P, tabs.n_files, g_lo), f_last = many_file_of(tabs.P, tabs.n_files, g_hi - 1);
    for (int f = f_first + (int)blockIdx.x; f <= f_last; f += (int)gridDim.x) {
        const int p0 = tabs.P[f], lo = max(p0, g_lo), hi = min(tabs.P[f + 1], g_hi);
        for (int g = lo; g < hi; g++) {
            const int pl = place[g];
            const float *yw = pl >= 0 ? y + (long long)(pl - j0) * y_bs : zero;
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
}

// stitch_assemble_many_kernel over the same range: grid (tiles of a frame, rows); row r takes global windows g_lo + r, + gridDim.y, ..
static __global__ __launch_bounds__(256) void stitch_assemble_gated_kernel(const float *y, long long y_bs, const float *zero, const int *__restrict__ place,
                                                                           const int *__restrict__ win_of, int j0, int nw, int A, int W, ManyTables tabs, int sola_len, int frame,
                                                                           const float *tails, const int *offsets, float *out)
{
    int g_lo, g_hi;
    silence_batch_range(win_of, j0, nw, A, W, &g_lo, &g_hi);
    const int i0 = blockIdx.x * STITCH_TILE;
    for (int g = g_lo + (int)blockIdx.y; g < g_hi; g += (int)gridDim.y) {
        const int f = many_file_of(tabs.P, tabs.n_files, g), w = g - tabs.P[f], pl = place[g];
        const float *o = (pl >= 0 ? y + (long long)(pl - j0) * y_bs : zero) + offsets[g];
        const float *prev = w == 0 ? tails : tails + (long long)g * sola_len;
        const long long base = (long long)w * frame, n_out = tabs.out_n[f];
        float *dst = out + tabs.out_off[f];
        for (int i = i0 + threadIdx.x; i < i0 + STITCH_TILE && i < frame; i += 256) {
            if (base + i >= n_out) break;
            dst[base + i] = i < sola_len ? sola_fade(o[i], prev[i], i, sola_len) : o[i];
        }
    }
}

// The analysis of a call and what its batches read.  queue_file per recording (files in order), then finish: the compaction and the call's one read
struct SilenceWork {
    DevBuf<double> bs; DevBuf<int> cnt, active, place, win_of; DevBuf<unsigned char> loud, kept; DevBuf<unsigned long long> counts; DevBuf<float> zero;
    size_t W = 0, frames = 0, A = 0, n_loud = 0, n_kept = 0;
    double thr = 0.0; int hang = 0;
    DevTimer timer; double ms = 0.0;
    size_t batches(size_t S) const { return (A + S - 1) / S; }

    // frames / windows: of the whole call; zero_len: the samples of a stitch window (0: no stitch follows)
    void begin(hipStream_t st, size_t frames_total, size_t windows_total, double threshold_db, int hang_frames, size_t zero_len)
    {
        if (frames_total > (size_t)SILENCE_MAX_FRAMES) throw ShapeError("convert: recording too long for the silence gate (2^31 frames)");
        frames = frames_total; W = windows_total; thr = silence_threshold(threshold_db); hang = hang_frames;
        bs.alloc(frames); cnt.alloc(frames); loud.alloc(frames); kept.alloc(frames); active.alloc(W); place.alloc(W); win_of.alloc(W); counts.alloc(4);
        timer.start(st);
        HIPCHK(hipMemsetAsync(counts.get(), 0, 4 * sizeof(unsigned long long), st));
        if (zero_len) { zero.alloc(zero_len); HIPCHK(hipMemsetAsync(zero.get(), 0, zero_len * sizeof(float), st)); }
    }
    // one recording: sig [N], its Nf frames at frame_off and its Wf windows at win_off of the call's arrays
    void queue_file(hipStream_t st, const float *sig, size_t N, size_t Nf, size_t frame_off, size_t Wf, size_t win_off, const ConvertGeometry &g)
    {
        hipLaunchKernelGGL(silence_block_kernel, dim3((unsigned)((Nf + 3) / 4)), dim3(256), 0, st, sig, (long long)N, (long long)Nf, bs.get() + frame_off);
        hipLaunchKernelGGL(silence_loud_scan_kernel, dim3(1), dim3(SILENCE_SCAN_THREADS), 0, st, (const double *)(bs.get() + frame_off), (long long)Nf, thr, loud.get() + frame_off,
                           cnt.get() + frame_off, counts.get());
        hipLaunchKernelGGL(silence_kept_kernel, dim3((unsigned)((Nf + 255) / 256)), dim3(256), 0, st, (const int *)(cnt.get() + frame_off), (long long)Nf, hang, kept.get() + frame_off,
                           counts.get());
        hipLaunchKernelGGL(silence_active_kernel, dim3((unsigned)((Wf + 255) / 256)), dim3(256), 0, st, (const int *)(cnt.get() + frame_off), (long long)Nf, hang, (int)g.H,
                           (int)g.return_length, (int)Wf, active.get() + win_off);
    }
    // the compaction, then the three counters come to the host: the stream is synchronised
    void finish(hipStream_t st)
    {
        hipLaunchKernelGGL(silence_compact_kernel, dim3(1), dim3(SILENCE_SCAN_THREADS), 0, st, (const int *)active.get(), (int)W, place.get(), win_of.get(), counts.get());
        timer.stop(st);
        unsigned long long c[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(c, counts.get(), sizeof c, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        A = (size_t)c[0]; n_loud = (size_t)c[1]; n_kept = (size_t)c[2];
        if (A > W) throw std::runtime_error("silence gate: the active count exceeds the window count");
        ms = (double)timer.ms();
    }
    // the two stitch launches behind the batch of active windows [j0, j0 + nw) (nw = 0: a call without an active window)
    void stitch(hipStream_t st, const float *y, long long y_bs, size_t j0, int nw, const ManyTables &tabs, int sola_len, int search, int frame, float *tails, int *offsets, float *out) const
    {
        const unsigned chains = (unsigned)std::min(tabs.n_files, 64), rows = (unsigned)std::min<size_t>(W, 64);
        hipLaunchKernelGGL(stitch_chain_gated_kernel, dim3(chains), dim3(STITCH_CHAIN_THREADS), 0, st, y, y_bs, (const float *)zero.get(), (const int *)place.get(),
                           (const int *)win_of.get(), (int)j0, nw, (int)A, (int)W, tabs, sola_len, search, frame, tails, offsets);
        hipLaunchKernelGGL(stitch_assemble_gated_kernel, dim3((unsigned)((frame + STITCH_TILE - 1) / STITCH_TILE), rows), dim3(256), 0, st, y, y_bs, (const float *)zero.get(),
                           (const int *)place.get(), (const int *)win_of.get(), (int)j0, nw, (int)A, (int)W, tabs, sola_len, frame, (const float *)tails, (const int *)offsets, out);
    }
};

}  // namespace rvc
