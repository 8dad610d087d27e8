// f0_select_many.hip.h -- f0_select.hip.h's exact order statistics for many recordings at once, included by f0_analyze_many.hip.h
// (engine.hip's unit).
//
// The rows of F recordings lie end to end in one arena, off [F + 1] their prefix sums.  One launch: workgroup f runs, over rows [off[f], off[f + 1]), the one-launch
// path of f0_select_kernel -- four 8-bit digit passes from the top, the histograms (8 quantiles x 256 bins) in LDS, after each pass the wave-per-quantile scan that
// picks the digit holding the quantile's rank -- and writes its nq values and its voiced count.  Same rule (voiced iff 1 <= bits <= 0x7F7FFFFF; rank
// floor(p (v - 1)) with the product in double), so the answer is rvc_f0_stats of the file's rows bit for bit.  Only integers are summed: the result depends on
// the input alone.  The row loop strides the workgroup over the segment, so a file of any length runs (the one-launch path of f0_select_kernel stops at 8192
// rows); a segment starts at an arbitrary row of the arena, so the loads are scalar -- no alignment is assumed.  Nothing is shared between workgroups.
#pragma once
#include "f0_select.hip.h"

namespace rvc {

constexpr int F0_SEL_MANY_STRIDE = F0_SEL_MAXQ + 1;      // words per file in the result: out [8] as float bits | v

struct F0SelManyP {
    const uint32_t *x;                            // the arena as bit patterns
    const long long *off;                         // [F + 1], device
    int nq; double quant[F0_SEL_MAXQ];
    uint32_t *res;                                // [F][F0_SEL_MANY_STRIDE]
};

static __global__ __launch_bounds__(F0_SEL_THREADS) void f0_select_many_kernel(const F0SelManyP p)
{
    __shared__ uint32_t h[F0_SEL_MAXQ][256];
    __shared__ uint32_t s_prefix[F0_SEL_MAXQ], s_rank[F0_SEL_MAXQ], s_own[F0_SEL_MAXQ], s_v;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nq = p.nq;
    const long long r0 = p.off[blockIdx.x], n = p.off[blockIdx.x + 1] - r0;
    const uint32_t *x = p.x + r0;
    for (int P = 0; P <= F0_SEL_PASSES; P++) {
        if (P > 0) {
            // ---- the scan behind pass P - 1: for every quantile the digit that holds its rank, the rank inside that digit
            uint32_t digit[2] = {0u, 0u}, rank[2] = {0u, 0u}, vtot = 0u;
            for (int j = 0; j < 2; j++) {          // wave w scans quantiles w and w + 4: lane l holds bins 4 l .. 4 l + 3
                const int q = wave + 4 * j;
                if (q >= nq) continue;
                const uint32_t *hq = h[P == 1 ? 0 : s_own[q]];
                const uint32_t c0 = hq[4 * lane], c1 = hq[4 * lane + 1], c2 = hq[4 * lane + 2], c3 = hq[4 * lane + 3];
                uint32_t inc = c0 + c1 + c2 + c3;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const uint32_t up = __shfl_up(inc, o, 64); if (lane >= o) inc += up; }
                const uint32_t total = __shfl(inc, 63, 64);
                uint32_t k;
                if (P == 1) {                      // v is known now: the rank of the quantile, the one product that is not integer arithmetic
                    vtot = total;
                    k = total ? (uint32_t)(long long)floor(p.quant[q] * (double)(total - 1u)) : 0u;
                    if (total && k > total - 1u) k = total - 1u;
                } else k = s_rank[q];
                const unsigned long long holds = __ballot(inc > k);       // lanes whose bins end behind rank k: the first one holds it
                const int l0 = holds ? __ffsll((long long)holds) - 1 : 63;
                uint32_t before = __shfl(inc - (c0 + c1 + c2 + c3), l0, 64);
                const uint32_t d0 = __shfl(c0, l0, 64), d1 = __shfl(c1, l0, 64), d2 = __shfl(c2, l0, 64);
                uint32_t d = 4u * (uint32_t)l0;
                if (holds) {
                    if (k >= before + d0) { before += d0; d++; if (k >= before + d1) { before += d1; d++; if (k >= before + d2) { before += d2; d++; } } }
                    k -= before;
                } else k = 0u;                     // (no voiced row at all: the answer is 0, whatever the digits say)
                digit[j] = d; rank[j] = k;
            }
            __syncthreads();                       // every wave has read the state of the pass before
            for (int j = 0; j < 2; j++) {
                const int q = wave + 4 * j;
                if (q < nq && lane == 0) { s_prefix[q] = (P == 1 ? 0u : s_prefix[q] << 8) | digit[j]; s_rank[q] = rank[j]; if (P == 1 && q == 0) s_v = vtot; }
            }
            __syncthreads();
            if (tid < nq) {                        // the owner of a quantile's histogram: the first quantile with the same prefix
                int own = tid;
                for (int o = tid - 1; o >= 0; o--) if (s_prefix[o] == s_prefix[tid]) own = o;
                s_own[tid] = (uint32_t)own;
            }
            __syncthreads();
            if (P == F0_SEL_PASSES) {
                uint32_t *res = p.res + (size_t)blockIdx.x * F0_SEL_MANY_STRIDE;
                if (tid < F0_SEL_MAXQ) res[tid] = tid < nq && s_v ? s_prefix[tid] : 0u;
                if (tid == 0) res[F0_SEL_MAXQ] = s_v;
                return;
            }
        }
        // ---- digit pass P: the histogram of digit P over the voiced rows that carry a quantile's prefix (pass 0: every voiced row, one histogram)
        for (int i = tid; i < F0_SEL_MAXQ * 256; i += F0_SEL_THREADS) h[i >> 8][i & 255] = 0u;
        __syncthreads();
        const int shift = 24 - 8 * P;
        for (long long i = tid; i < n; i += F0_SEL_THREADS) {
            const uint32_t key = x[i];
            if (!f0_sel_voiced(key)) continue;
            const uint32_t d = (key >> shift) & 255u;
            if (P == 0) { atomicAdd(&h[0][d], 1u); continue; }
            const uint32_t hi = key >> (shift + 8);
            for (int q = 0; q < nq; q++) if (s_own[q] == (uint32_t)q && s_prefix[q] == hi) atomicAdd(&h[q][d], 1u);
        }
        __syncthreads();
    }
}

// one select per file over the arena x (device) cut at off [F + 1] (device) on stream s -> res [F][F0_SEL_MANY_STRIDE] (device)
static void launch_f0_select_many(hipStream_t s, const float *x, const long long *off, size_t n_files, const double *quant, int nq, uint32_t *res)
{
    F0SelManyP p{};
    p.x = (const uint32_t *)x; p.off = off; p.nq = nq; p.res = res;
    for (int i = 0; i < nq; i++) p.quant[i] = quant[i];
    hipLaunchKernelGGL(f0_select_many_kernel, dim3((unsigned)n_files), dim3(F0_SEL_THREADS), 0, s, p);
}

}  // namespace rvc
