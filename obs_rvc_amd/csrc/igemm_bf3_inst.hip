// igemm_bf3_inst.hip -- instantiation of the exploratory split-bf16 GEMM (igemm_bf3_kernel, igemm_bf3.hip.h) and of its weight packer.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "igemm_launch.h"
#include "igemm_bf3.hip.h"

namespace rvc {

void launch_igemm_bf3(bool lin, bool pre, const IgemmP &p, dim3 grid, size_t lds, hipStream_t s, hipEvent_t ea, hipEvent_t eb)
{
    if (lin) launch_k(igemm_bf3_kernel<2, 2, 2, 2, true, false>, p, grid, dim3(256), lds, s, ea, eb);
    else if (pre) launch_k(igemm_bf3_kernel<2, 2, 2, 2, false, true>, p, grid, dim3(256), lds, s, ea, eb);
    else launch_k(igemm_bf3_kernel<2, 2, 2, 2, false, false>, p, grid, dim3(256), lds, s, ea, eb);
}

static __global__ void bf3_pack_kernel(const float *wfrag, int M, int nchunks, bf16x8 *out, long long total)
{
    // out element (blk32, chunk, half, lane): eight bf16 of row blk32 * 32 + (lane & 31), k = chunk * 16 + (lane >> 5) * 8 + i, from the fp32
    // fragment packing [m_tile16][chunk][lane16x4][4]
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int lane = (int)(e & 63), half = (int)((e >> 6) & 1);
    const long long bc = e >> 7;
    const int chunk = (int)(bc % nchunks), blk = (int)(bc / nchunks);
    const int m = blk * 32 + (lane & 31), mt16 = (M + 15) >> 4;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int kk = (lane >> 5) * 8 + i;
        v[i] = (m >> 4) < mt16 ? wfrag[((((long long)(m >> 4) * nchunks + chunk) * 64) + (kk >> 2) * 16 + (m & 15)) * 4 + (kk & 3)] : 0.f;
    }
    bf16x8 hi, lo;
    bf3_split(v, hi, lo);
    out[e] = half ? lo : hi;
}

// fp32 fragment-major panel [ceil(M / 16)][nchunks][64][4] -> split panels [ceil(M / 32)][nchunks][hi | lo][64][8 bf16]; bytes of the result = M32 * nchunks * 2048
void bf3_pack(const float *wfrag, int M, int nchunks, void *out, hipStream_t s)
{
    const long long total = (long long)((M + 31) / 32) * nchunks * 128;
    hipLaunchKernelGGL(bf3_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, wfrag, M, nchunks, reinterpret_cast<bf16x8 *>(out), total);
}

}  // namespace rvc
