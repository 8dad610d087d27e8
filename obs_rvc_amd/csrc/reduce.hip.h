// reduce.hip.h -- wave / block reductions (64-wide wavefronts).  __device__ __forceinline__ functions only, no __global__ function: any kernel header
// may include it.
#pragma once
#include <hip/hip_runtime.h>

namespace rvc {

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// the smallest (value, index) pair of the wave, ties by the lower index, left in every lane
__device__ __forceinline__ void wave_min_pair(float &d, int &i)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(d, o, 64); const int oi = __shfl_xor(i, o, 64);
        if (od < d || (od == d && oi < i)) { d = od; i = oi; }
    }
}
// blockDim.x must be a multiple of 64 and <= 1024; red must hold 16 floats
__device__ __forceinline__ float block_sum(float v, float *red)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < nw; i++) t += red[i];
    return t;
}
// ... and the largest value of the block, under the same conditions
__device__ __forceinline__ float block_max(float v, float *red)
{
    v = wave_max(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float t = red[0];
    for (int i = 1; i < nw; i++) t = fmaxf(t, red[i]);
    return t;
}

}  // namespace rvc
