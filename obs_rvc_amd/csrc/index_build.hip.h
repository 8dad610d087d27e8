// index_build.hip.h -- the kernels of the index builder: ContentVec frames of one window into the row store of a build, rows that
// hold a NaN or an Inf squeezed out on the device.  Included by retrieval.hip only.
#pragma once
#include <hip/hip_runtime.h>

namespace rvc {

#define IB_TILE 32                     // index_append_kernel: a 32 x 32 tile of (channel, frame) per workgroup, staged in LDS as 32 x 33

// ---- append: rows[cursor + t][c] = cv[c][t], bit for bit; bad[t] |= 1 when frame t holds a value with x - x != 0 ----
// cv is the plan's ContentVec output, channel-major: C rows of T used columns with leading dimension ld.  A workgroup (256 threads = 8 x 32) reads its tile with
// the 32 lanes of a half-wave along t (one 128-byte segment per channel) and writes it with the 32 lanes along c (one 128-byte segment per store row); the tile
// sits in LDS with a row stride of 33 words, so the transposed read walks 32 different banks.  In the write phase a wave holds two store rows, one per
// half-wave: one ballot over the wave gives each half its finite flag, and the half's first lane raises the frame's word (an integer OR: any order).
// cursor is read from the device (cnt[0]): the host never learns it between the windows of one add.  The host sizes the store for an upper bound of the cursor
// (no row dropped); the kernel still refuses a window that would not fit.
struct IndexAppendP {
    const float *cv; int C, T, ld;
    float *rows; long long capacity;      // store [capacity][C]
    const int *cnt;                       // cnt[0] = rows the store holds
    int *bad;                             // [T], zero on entry
};
static __global__ __launch_bounds__(256) void index_append_kernel(IndexAppendP p)
{
    __shared__ unsigned tile[IB_TILE][IB_TILE + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int t0 = blockIdx.x * IB_TILE, c0 = blockIdx.y * IB_TILE;
    const long long cursor = p.cnt[0];
    if (cursor < 0 || cursor + p.T > p.capacity) return;
    const unsigned *src = reinterpret_cast<const unsigned *>(p.cv);
    unsigned *dst = reinterpret_cast<unsigned *>(p.rows);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = c0 + ty + 8 * k, t = t0 + tx;
        tile[ty + 8 * k][tx] = (c < p.C && t < p.T) ? src[(long long)c * p.ld + t] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int t = t0 + ty + 8 * k, c = c0 + tx;
        const bool in = t < p.T && c < p.C;
        const unsigned v = tile[tx][ty + 8 * k];
        const float x = __uint_as_float(v);
        if (in) dst[(cursor + t) * p.C + c] = v;
        const unsigned long long m = __ballot(in && !(x - x == 0.f));
        const unsigned half = (threadIdx.x & 32) ? (unsigned)(m >> 32) : (unsigned)m;
        if (tx == 0 && half && t < p.T) atomicOr(&p.bad[t], 1);
    }
}

// ---- compact: one workgroup behind index_append_kernel ----
// Phase 1: an exclusive prefix over the window's keep flags (256 frames per step, a running base across steps) turns bad[t] into the frame's place among the
// kept ones, -1 for a dropped frame.  Phase 2, only when a frame was dropped: frames in ascending t move down to cursor + place[t]; a frame's place is never
// above t, so a move overwrites a row that has already been moved (or dropped), and the barrier between two moves keeps a source row from being overwritten
// while other threads still read it.  Then cnt[0] += kept, cnt[1] += dropped, and bad[] is zero again for the next window.
static __global__ __launch_bounds__(256) void index_compact_kernel(float *rows, int C, long long capacity, int *bad, int T, int *cnt)
{
    __shared__ int s[256];
    __shared__ int s_base;
    const int tid = threadIdx.x;
    const long long cursor = cnt[0];
    if (cursor < 0 || cursor + T > capacity) return;         // (the append refused the window as well)
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int t0 = 0; t0 < T; t0 += 256) {
        const int t = t0 + tid;
        const int keep = (t < T && bad[t] == 0) ? 1 : 0;
        s[tid] = keep;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {                  // inclusive scan
            const int v = tid >= o ? s[tid - o] : 0;
            __syncthreads();
            s[tid] += v;
            __syncthreads();
        }
        const int base = s_base;
        if (t < T) bad[t] = keep ? base + s[tid] - 1 : -1;
        __syncthreads();
        if (tid == 255) s_base = base + s[255];
        __syncthreads();
    }
    const int kept = s_base;
    if (kept != T) {
        unsigned *r = reinterpret_cast<unsigned *>(rows) + cursor * C;
        for (int t = 0; t < T; t++) {
            const int d = bad[t];                             // (written by this workgroup before the barriers above; the same word for every thread)
            if (d < 0 || d == t) continue;
            for (int c = tid; c < C; c += 256) r[(long long)d * C + c] = r[(long long)t * C + c];
            __syncthreads();
        }
    }
    __syncthreads();
    for (int t = tid; t < T; t += 256) bad[t] = 0;
    if (tid == 0) { cnt[0] = (int)(cursor + kept); cnt[1] += T - kept; }
}

}  // namespace rvc
