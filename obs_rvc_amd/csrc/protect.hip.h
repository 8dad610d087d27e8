// protect.hip.h -- consonant protection (upstream RVC's `protect`; DESIGN.md "Consonant protection"): on the unvoiced rows of a chunk the
// index-blended features are mixed back towards the raw ContentVec features,
//   phone[c][r] = p phone[c][r] + (1 - p) raw[c][r]        for every row r with pitchf[r] < 1.0f,   p = StreamCtl::protect
// one launch behind the join of the two front branches, on the plans that use the index and have a stream with p < 0.5 (engine.hip get_plan).
// raw[c][r] is the element gather_phone_kernel wrote before the retrieval: the ContentVec output is never written by the retrieval, so it is read
// again through the same column rule (phone_src_col) instead of being copied.
#pragma once
#include <hip/hip_runtime.h>
#include "state.hip.h"

namespace rvc {

// the ContentVec column behind row r of `phone`: feats[min((skip_head + r) / 2, T - 1)]   (rvc.rs:99-109 + 155; Q2, Q8).  gather_phone_kernel and
// protect_mix_kernel both go through this, so that what protection calls "raw" is what the gather wrote
__device__ __forceinline__ int phone_src_col(int skip_head, int r, int T)
{
    int s = (skip_head + r) / 2;
    return s < T - 1 ? s : T - 1;
}

// A workgroup takes PROTECT_ROWS consecutive rows and PROTECT_CH consecutive channels of one stream: threadIdx.x is the row, so a wave's loads and stores
// of one channel are 64 consecutive floats of `phone` (channel-major) and 32 consecutive floats of the ContentVec output; threadIdx.y picks the channel,
// PROTECT_PER channels per thread, PROTECT_LANES apart.  A thread issues all its loads (2 PROTECT_PER) before its first store, so it pays one memory round
// trip, not one per channel; `phone` and `cv` never overlap (__restrict__).  The channel slices are a grid dimension, so one stream's R C elements are
// spread over C / PROTECT_CH workgroups instead of walked by one.  The voicing test is per thread: a voiced row's threads leave without touching memory,
// so its bits stay.  No LDS, no atomics; grid (ceil(R / PROTECT_ROWS), streams, ceil(C / PROTECT_CH)).
constexpr int PROTECT_ROWS = 64, PROTECT_LANES = 4, PROTECT_PER = 4, PROTECT_CH = PROTECT_LANES * PROTECT_PER;
static inline dim3 protect_grid(int R, int B, int C) { return dim3((R + PROTECT_ROWS - 1) / PROTECT_ROWS, B, (C + PROTECT_CH - 1) / PROTECT_CH); }
static __global__ void __launch_bounds__(PROTECT_ROWS * PROTECT_LANES)
protect_mix_kernel(const StreamState *__restrict__ st, const float *__restrict__ pitchf, const float *__restrict__ cv, int cv_cs, long long cv_bs, int C, int T,
                   int skip_head, int R, float *__restrict__ phone, int ph_cs, long long ph_bs)
{
    const int b = blockIdx.y;
    const float p = st[b].ctl.protect;
    if (!(p < (float)PROTECT_OFF)) return;                      // this stream is off (uniform over the workgroup)
    const int r = blockIdx.x * PROTECT_ROWS + threadIdx.x;
    if (r >= R) return;
    if (!(pitchf[(long long)b * R + r] < 1.0f)) return;         // voiced
    const float q = 1.0f - p;
    float *ph = phone + (long long)b * ph_bs + r;
    const float *raw = cv + (long long)b * cv_bs + phone_src_col(skip_head, r, T);
    const int c0 = blockIdx.z * PROTECT_CH + threadIdx.y;
    float x[PROTECT_PER], w[PROTECT_PER];
#pragma unroll
    for (int k = 0; k < PROTECT_PER; k++) {
        const int c = c0 + k * PROTECT_LANES;
        if (c < C) { x[k] = ph[(long long)c * ph_cs]; w[k] = raw[(long long)c * cv_cs]; }
    }
#pragma unroll
    for (int k = 0; k < PROTECT_PER; k++) {
        const int c = c0 + k * PROTECT_LANES;
        if (c < C) ph[(long long)c * ph_cs] = p * x[k] + q * w[k];
    }
}

}  // namespace rvc
