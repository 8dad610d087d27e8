// f0_select.hip.h -- exact order statistics of the voiced rows of an f0 track, included by engine.hip through f0_analyze.hip.h.
//
// A row is voiced iff it is finite and > 0: as a bit pattern, 1 <= key <= 0x7F7FFFFF.  On that range the IEEE order is the unsigned order of the bits, so the
// element of rank k among the v voiced rows is found by a radix select on the bits: four digit passes of 8 bits from the top, each a histogram of the rows
// that still agree with the digits chosen so far, followed by a scan that picks the digit holding rank k.  Up to 8 quantiles are selected at once, each with a
// prefix and a remaining rank of its own; quantiles whose prefixes agree share one histogram.  Everything is integer arithmetic on the bits -- the answer is an
// element of the input, bit for bit -- except the rank itself, floor(p (v - 1)) with the product in double, as the definition has it.
//
// One kernel, two launch shapes.  Up to F0_SEL_ONE_BLOCK rows (a stream's 1024-row pitch cache): one workgroup runs the five phases (four histograms, the
// final scan) in one launch, the histograms never leaving LDS.  Beyond: one launch per phase on a grid of up to 2048 workgroups; a workgroup histograms its
// share in LDS, adds its non-empty bins to the phase's global histogram with integer atomics (integer addition commutes: the sums do not depend on the order),
// and the NEXT launch -- every workgroup of it, redundantly -- scans them; workgroup 0 stores the scan's result (prefix, rank, histogram owner, v) with plain
// vector stores for the launch behind it.  Nothing is handed from workgroup to workgroup inside a launch, nothing returns to the host between the passes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rvc {

constexpr int F0_SEL_MAXQ = 8;                    // quantiles per call
constexpr int F0_SEL_PASSES = 4;                  // 8-bit digits of a key
constexpr int F0_SEL_THREADS = 256;
constexpr size_t F0_SEL_ONE_BLOCK = 8192;         // rows up to which one workgroup does everything in one launch
constexpr int F0_SEL_ROWS_PER_BLOCK = 4096;       // beyond: rows a workgroup takes per pass (16 per thread, as 4 loads of 16 bytes), the grid capped at ...
constexpr int F0_SEL_MAX_BLOCKS = 2048;           // ... eight workgroups per CU; further rows are grid-strided
// the workspace, in 32-bit words: the global histograms [pass][quantile][256], then the scan results of phase P = 1 .. 4 (prefix [8] | rank [8] | owner [8] | v),
// then the answer: out [8] as float bits | v
constexpr int F0_SEL_STATE_STRIDE = 32;
constexpr int F0_SEL_HIST_WORDS = F0_SEL_PASSES * F0_SEL_MAXQ * 256;
constexpr int F0_SEL_STATE_AT = F0_SEL_HIST_WORDS;
constexpr int F0_SEL_OUT_AT = F0_SEL_STATE_AT + (F0_SEL_PASSES + 1) * F0_SEL_STATE_STRIDE;
constexpr int F0_SEL_WS_WORDS = F0_SEL_OUT_AT + 16;

struct F0SelP {
    const uint32_t *x; long long n;               // the rows as bit patterns (16-byte aligned)
    int nq; double quant[F0_SEL_MAXQ];
    int phase0, nphase;                           // the phases this launch runs: 0 .. 3 = digit passes, 4 = the final scan (one workgroup: 0, 5; else P, 1)
    uint32_t *ws;
};

__device__ __forceinline__ bool f0_sel_voiced(uint32_t key) { return key - 1u < 0x7F7FFFFFu; }

static __global__ __launch_bounds__(F0_SEL_THREADS) void f0_select_kernel(const F0SelP p)
{
    __shared__ uint32_t h[F0_SEL_MAXQ][256];
    __shared__ uint32_t s_prefix[F0_SEL_MAXQ], s_rank[F0_SEL_MAXQ], s_own[F0_SEL_MAXQ], s_v;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nq = p.nq;
    const bool multi = p.nphase == 1;
    for (int P = p.phase0; P < p.phase0 + p.nphase; P++) {
        if (P > 0) {
            // ---- the scan behind pass P - 1: for every quantile the digit that holds its rank, the rank inside that digit
            if (multi) {
                const uint32_t *gh = p.ws + (size_t)(P - 1) * F0_SEL_MAXQ * 256;
                for (int i = tid; i < F0_SEL_MAXQ * 256; i += F0_SEL_THREADS) h[i >> 8][i & 255] = gh[i];
                if (P > 1 && tid < F0_SEL_MAXQ) {
                    const uint32_t *st = p.ws + F0_SEL_STATE_AT + (P - 1) * F0_SEL_STATE_STRIDE;
                    s_prefix[tid] = st[tid]; s_rank[tid] = st[8 + tid]; s_own[tid] = st[16 + tid];
                    if (tid == 0) s_v = st[24];
                }
                __syncthreads();
            }
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
                if (blockIdx.x == 0 && tid < F0_SEL_MAXQ) p.ws[F0_SEL_OUT_AT + tid] = tid < nq && s_v ? s_prefix[tid] : 0u;
                if (blockIdx.x == 0 && tid == 0) p.ws[F0_SEL_OUT_AT + 8] = s_v;
                return;
            }
            if (multi && blockIdx.x == 0 && tid < F0_SEL_MAXQ) {
                uint32_t *st = p.ws + F0_SEL_STATE_AT + P * F0_SEL_STATE_STRIDE;
                st[tid] = s_prefix[tid]; st[8 + tid] = s_rank[tid]; st[16 + tid] = s_own[tid];
                if (tid == 0) st[24] = s_v;
            }
        }
        // ---- digit pass P: the histogram of digit P over the voiced rows that carry a quantile's prefix (pass 0: every voiced row, one histogram)
        for (int i = tid; i < F0_SEL_MAXQ * 256; i += F0_SEL_THREADS) h[i >> 8][i & 255] = 0u;
        __syncthreads();
        const int shift = 24 - 8 * P;
        auto take = [&](uint32_t key) {
            if (!f0_sel_voiced(key)) return;
            const uint32_t d = (key >> shift) & 255u;
            if (P == 0) { atomicAdd(&h[0][d], 1u); return; }
            const uint32_t hi = key >> (shift + 8);
            for (int q = 0; q < nq; q++) if (s_own[q] == (uint32_t)q && s_prefix[q] == hi) atomicAdd(&h[q][d], 1u);
        };
        const long long n4 = p.n >> 2;
        const uint4 *x4 = (const uint4 *)p.x;
        for (long long i = (long long)blockIdx.x * F0_SEL_THREADS + tid; i < n4; i += (long long)gridDim.x * F0_SEL_THREADS) {
            const uint4 k4 = x4[i];
            take(k4.x); take(k4.y); take(k4.z); take(k4.w);
        }
        if (blockIdx.x == 0 && tid < (int)(p.n & 3)) take(p.x[(n4 << 2) + tid]);
        __syncthreads();
        if (multi) {
            uint32_t *gh = p.ws + (size_t)P * F0_SEL_MAXQ * 256;
            const int rows = P == 0 ? 1 : nq;
            for (int i = tid; i < rows * 256; i += F0_SEL_THREADS) { const uint32_t c = h[i >> 8][i & 255]; if (c) atomicAdd(&gh[i], c); }
        }
    }
}

// tracked[j] = isnan(curve[j]) ? tracked[j] : curve[j]: the f0 that will be transposed when a curve is in force (plain selection, in place)
static __global__ __launch_bounds__(256) void f0_merge_kernel(float *__restrict__ tracked, const float *__restrict__ curve, long long n)
{
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const float c = curve[j];
    if (c == c) tracked[j] = c;
}

// the launches of one select over n rows at x (device, 16-byte aligned) on stream s: ws (F0_SEL_WS_WORDS words) ends with out [8] | v
static void launch_f0_select(hipStream_t s, const float *x, size_t n, const double *quant, int nq, uint32_t *ws)
{
    F0SelP p{};
    p.x = (const uint32_t *)x; p.n = (long long)n; p.nq = nq; p.ws = ws;
    for (int i = 0; i < nq; i++) p.quant[i] = quant[i];
    if (n <= F0_SEL_ONE_BLOCK) {
        p.phase0 = 0; p.nphase = F0_SEL_PASSES + 1;
        hipLaunchKernelGGL(f0_select_kernel, dim3(1), dim3(F0_SEL_THREADS), 0, s, p);
        return;
    }
    HIPCHK(hipMemsetAsync(ws, 0, F0_SEL_HIST_WORDS * sizeof(uint32_t), s));
    const size_t blocks = std::min<size_t>((n + F0_SEL_ROWS_PER_BLOCK - 1) / F0_SEL_ROWS_PER_BLOCK, F0_SEL_MAX_BLOCKS);
    p.nphase = 1;
    for (int P = 0; P <= F0_SEL_PASSES; P++) {
        p.phase0 = P;
        hipLaunchKernelGGL(f0_select_kernel, dim3(P == F0_SEL_PASSES ? 1u : (unsigned)blocks), dim3(F0_SEL_THREADS), 0, s, p);
    }
}

}  // namespace rvc
