// igemm32.hip.h -- igemm32_kernel, the workgroup-tiled 32x32x2 throughput kernel (instantiated by igemm_tiled_inst.hip; igemm32l.hip.h borrows its occupancy rule)
#pragma once
#include "igemm_common.hip.h"

namespace rvc {

// ------------------------------------------------------------------------------------------------------------------------
// igemm32_kernel -- throughput-mode implicit GEMM on v_mfma_f32_32x32x2_f32 (many streams: N = streams * positions is large).
// A 256-thread workgroup owns a (WM*MT*32) x (WN*NT*32) tile; every wave a (MT*32) x (NT*32) block of 32x32 accumulators
// (16 registers each).  Per K step of 16:
//   * the gathered activation tile [16][BN] goes global -> registers -> LDS once per workgroup (double-buffered, ONE barrier per
//     step, fused input LeakyReLU applied once per element) and is read back as MFMA B operands by all four waves;
//   * the weights stream global -> registers straight from the 16-row fragment packing the latency kernels use: for a 32-row
//     MFMA the lane (row r, k-slot s) reads the float4 of fragment r>>4, quad q = 2u+s (u = 0, 1), so the eight MFMAs of a step
//     take k = (2u+s)*4 + j -- A and B agree on that order, no repacking, no shuffles;
//   * 32x32x2 halves the MFMA instruction count of the 16x16x4 form and has no dependent-issue gap (64-cycle issue = 64-cycle
//     accumulator latency), so one wave per SIMD already saturates the pipe while the next step's loads are in flight.
// Epilogue: C/D layout col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5): a lane owns 16 rows of ONE column, so
// the column part of the address (stream, row, validity) is computed once per 32-column block.
// Wide register tiles were measured in round 5 and are not instantiated: MT x NT = 4 x 2 (a wave owns 128 x 64 outputs, 222 registers, two waves per
// SIMD) runs the 64-stream layers at the speed of the 2 x 2 tile (+-1 %; +5 % on the one layer whose grid it rounds better), 4 x 4 (256 accumulator
// registers) spills -- DESIGN.md section 7 round 5.  The occupancy rule and the loop below stay general.  The K loop is unrolled by two so that the weight
// registers of consecutive steps alternate instead of being copied.
template <int MT, int NT> struct G32Occ { static constexpr int W = MT * NT >= 16 ? 1 : (MT * NT >= 8 ? 2 : 3); };
template <int WM, int WN, int MT, int NT, bool PRE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(G32Occ<MT, NT>::W, G32Occ<MT, NT>::W))) void igemm32_kernel(IgemmP p)
{
    static_assert(WM * WN == 4, "four waves per workgroup");
    constexpr int BM = WM * MT * 32, BN = WN * NT * 32;
    // The staged activation tile is kept COLUMN-major, [BN][16 k + 4 pad]: the four k-values (2u + ks) * 4 + j, j = 0..3, that a lane feeds to four
    // consecutive MFMAs are one ds_read_b128, and a staging thread owns EPT consecutive k rows of one column (ds_write_b128).  On this chip an fp32
    // MFMA hides none of its SIMD's other instructions (tests/tools/mfma_overlap_probe.hip: +16 clocks per ds_read_b32, +4 per VALU, +32 per 16-byte
    // vector load, at any occupancy), so the row-major tile's 16 ds_read_b32 + 8 ds_write_b32 per K step were a sixth of the step.
    constexpr int RSK = 20;                        // column stride in floats: 16-byte aligned, 16 lanes x 16 bytes on disjoint banks
    constexpr int KR = 256 / BN > 0 ? 256 / BN : 1;    // staging threads per column
    constexpr int EPT = 16 / KR;                   // consecutive k rows per staging thread per K step (4, 8 or 16)
    static_assert(BN <= 256 && 256 % BN == 0, "BN must divide 256");
    extern __shared__ __attribute__((aligned(16))) int s_mem[];
    RVC_KP(0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int tid_x = p.m_fast == 1 ? xcd_tile_id((int)blockIdx.x, (int)gridDim.x, (int)(blockIdx.y * gridDim.x)) : (int)blockIdx.x;
    const int tn = p.m_fast ? tid_x / p.ntm : tid_x % p.ntn, tm = p.m_fast ? tid_x % p.ntm : tid_x / p.ntn;
    int z = blockIdx.y;
    const int phase = z % p.nphase;
    const int b = z / p.nphase;
    const PhaseD ph = p.nphase == 1 ? p.ph0 : p.ph[phase];
    const int nchunks = ph.nchunks;
    {
        const int4 *src = reinterpret_cast<const int4 *>(p.koff + ph.koff_off);
        int4 *dst = reinterpret_cast<int4 *>(s_mem);
        for (int i = threadIdx.x; i < nchunks * 4; i += 256) dst[i] = src[i];
    }
    float *bt = reinterpret_cast<float *>(s_mem + nchunks * 16);     // [2][BN][RSK]
    const int c32 = lane & 31, ks = lane >> 5;                       // MFMA column (B) / row (A) and k-slot of this lane
    const char *xb = reinterpret_cast<const char *>(p.x + (long long)b * p.x_bs + ph.x_off) - p.koff_bias;
    // staging role: column n_s of the tile, k rows kr0 .. kr0 + EPT - 1
    const int n_s = threadIdx.x % BN, kr0 = (threadIdx.x / BN) * EPT;
    unsigned xo_s;
    {
        int n = tn * BN + n_s;
        n = n < p.N ? n : p.N - 1;
        int bb = 0;
        if (p.fold_n) { bb = n / p.fold_n; n -= bb * p.fold_n; }
        int nh = 0, nw = n;
        if (p.x_hs) { nh = n / p.NW; nw = n - nh * p.NW; }
        xo_s = (unsigned)(bb * (int)p.x_bs + nh * p.x_hs + nw * p.x_ws) * 4u;
    }
    // weights: 16-row fragment packing [m_tile16][chunk][lane16x4][4]; this lane's float4 of quad q sits at ((q * 16 + r16) * 4)
    const float *wrow[MT];
    const int mtiles = (p.M + 15) >> 4;
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        int t16 = ((tm * WM + wm) * MT + mt) * 2 + (c32 >> 4);
        t16 = t16 < mtiles ? t16 : mtiles - 1;
        wrow[mt] = p.w + ph.w_off + (long long)t16 * nchunks * 256 + (ks * 16 + (c32 & 15)) * 4;
    }
    f32x16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[mt][nt][r] = 0.f;
    const float pre_slope = p.pre_slope;
    __syncthreads();
    RVC_KP(1);
    const int *kof = s_mem;
    float sb[EPT];
    f32x4 a_ev[MT][2], a_od[MT][2];          // weights of the even / odd K steps (the loop below is unrolled by two: no copies)
#pragma unroll
    for (int i = 0; i < EPT; i++) sb[i] = *reinterpret_cast<const float *>(xb + (xo_s + (unsigned)kof[kr0 + i]));
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int u = 0; u < 2; u++) a_ev[mt][u] = *reinterpret_cast<const f32x4 *>(wrow[mt] + u * 128);
#pragma unroll
    for (int i = 0; i < EPT; i += 4) {
        f32x4 v4;
#pragma unroll
        for (int q = 0; q < 4; q++) v4[q] = PRE ? fmaxf(sb[i + q], sb[i + q] * pre_slope) : sb[i + q];
        *reinterpret_cast<f32x4 *>(bt + n_s * RSK + kr0 + i) = v4;
    }
    __syncthreads();
    RVC_KP(2);
    // B operand of MFMA (u, j) for column block nt: row k = (2u + ks) * 4 + j of the staged tile
    const float *br = bt + (wn * NT * 32 + c32) * RSK + ks * 4;
    // one K step: request the next step's operands (global -> registers), run this step's MFMAs from a_c and the staged tile, stage the next tile
    auto kstep = [&](const int c, f32x4 (&a_c)[MT][2], f32x4 (&a_n)[MT][2]) {
        const int cn = c + 1 < nchunks ? c + 1 : c;
        const float *bcur = br + (c & 1) * BN * RSK;
        float *bnxt = bt + ((c + 1) & 1) * BN * RSK;
#pragma unroll
        for (int i = 0; i < EPT; i++) sb[i] = *reinterpret_cast<const float *>(xb + (xo_s + (unsigned)kof[cn * 16 + kr0 + i]));
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int u = 0; u < 2; u++) a_n[mt][u] = *reinterpret_cast<const f32x4 *>(wrow[mt] + cn * 256 + u * 128);
        __builtin_amdgcn_sched_barrier(0);      // (the next step's requests stay in FRONT of this step's MFMAs: left to itself the scheduler sinks them behind most of them)
#pragma unroll
        for (int u = 0; u < 2; u++) {
            f32x4 bv[NT];
#pragma unroll
            for (int nt = 0; nt < NT; nt++) bv[nt] = *reinterpret_cast<const f32x4 *>(bcur + nt * 32 * RSK + u * 8);
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int nt = 0; nt < NT; nt++)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_c[mt][u][j], bv[nt][j], acc[mt][nt], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < EPT; i += 4) {
            f32x4 v4;
#pragma unroll
            for (int q = 0; q < 4; q++) v4[q] = PRE ? fmaxf(sb[i + q], sb[i + q] * pre_slope) : sb[i + q];
            *reinterpret_cast<f32x4 *>(bnxt + n_s * RSK + kr0 + i) = v4;
        }
        __syncthreads();
    };
    {
        int c = 0;
        for (; c + 2 <= nchunks; c += 2) { kstep(c, a_ev, a_od); kstep(c + 1, a_od, a_ev); }
        if (c < nchunks) kstep(c, a_ev, a_od);
    }
    RVC_KP(3);
    const float *resb = p.res ? p.res + (long long)b * p.res_bs : nullptr;
    float *yb = p.y + (long long)b * p.y_bs;
    ColOut cols[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) cols[nt] = col_locate(p, ph, tn * BN + (wn * NT + nt) * 32 + c32);
    const int row0 = (tm * WM + wm) * MT * 32 + ks * 4;          // + mt * 32 + (reg & 3) + 8 * (reg >> 2)
    // Epilogue operands are loaded in batches that contain no store: a load may not be moved above an earlier store (the pointers
    // may alias), so "load bias, store, load bias, store, ..." is one memory round trip per element -- 64 of them per lane, measured
    // 68 us of a 300 us wave lifetime on the ContentVec convolutions.  Batched: one round trip for the 16 biases of a 32-row block,
    // one per 32x32 block for the residual / accumulate operands (none for most layers).  The batches are kept this small on
    // purpose: a whole-tile batch took the kernel from 164 to 268 registers (3 -> 1 waves per SIMD, 1.5x slower overall).
    const bool has_aux = resb != nullptr || p.accumulate;
    const bool full_m = row0 - ks * 4 + MT * 32 <= p.M;          // every row of this wave's tile exists (wave-uniform)
    if (full_m) {
        // The common case, kept small on purpose: straight-line code per element is what the 64-element unrolled epilogue costs
        // in instruction-cache footprint (the general version below is ~10x larger; with every workgroup of the chip walking
        // through it at a different point the epilogue took 43 us per wave, most of it instruction fetch).  One predicate per
        // 32-column block, the block's residual operands (if any) in one batch, 16 stores at scalar row offsets from one
        // per-lane base address.
        const float slope = p.slope, scale = p.scale;
        const long long cs = p.y_cs, rcs = p.res_cs;
        RVC_ACT_DISPATCH(
            _Pragma("unroll") for (int mt = 0; mt < MT; mt++) {
                const int m0 = row0 + mt * 32;
                float bias_r[16];
                _Pragma("unroll") for (int r = 0; r < 16; r++)
                    bias_r[r] = p.bias ? p.bias[ph.bias_off + m0 + (r & 3) + 8 * (r >> 2)] : 0.f;
                _Pragma("unroll") for (int nt = 0; nt < NT; nt++) {
                    if (cols[nt].yo >= 0) {
                        float rr[16];
                        _Pragma("unroll") for (int r = 0; r < 16; r++) rr[r] = 0.f;
                        if (resb) {
                            const float *rp = resb + cols[nt].ro + (long long)(p.res_nogroup ? m0 : m0 + ph.y_c0) * rcs;
                            _Pragma("unroll") for (int r = 0; r < 16; r++) rr[r] = rp[((r & 3) + 8 * (r >> 2)) * rcs];
                        }
                        float *yc = yb + cols[nt].yo + (long long)(m0 + ph.y_c0) * cs;
                        float yo_[16];          // (round 6: accumulating launches take this path too -- the previous output as one more store-free batch)
                        _Pragma("unroll") for (int r = 0; r < 16; r++) yo_[r] = 0.f;
                        if (p.accumulate) { _Pragma("unroll") for (int r = 0; r < 16; r++) yo_[r] = yc[((r & 3) + 8 * (r >> 2)) * cs]; }
                        _Pragma("unroll") for (int r = 0; r < 16; r++)
                            yc[((r & 3) + 8 * (r >> 2)) * cs] = epi2_value<A_>(acc[mt][nt][r], bias_r[r], rr[r], yo_[r], slope, scale);
                    }
                }
            }
        )
        RVC_KP(6);
        return;
    }
    RVC_ACT_DISPATCH(
        _Pragma("unroll") for (int mt = 0; mt < MT; mt++) {
            float bias_r[16];
            _Pragma("unroll") for (int r = 0; r < 16; r++) {
                const int m = row0 + mt * 32 + (r & 3) + 8 * (r >> 2);
                bias_r[r] = (p.bias && m < p.M) ? p.bias[ph.bias_off + m] : 0.f;
            }
            _Pragma("unroll") for (int nt = 0; nt < NT; nt++) {
                _Pragma("unroll") for (int h = 0; h < 16; h += 8) {
                    Epi2 e_[8];
                    _Pragma("unroll") for (int r = 0; r < 8; r++)
                        e_[r] = epi2_aux(p, ph, resb, yb, cols[nt], row0 + mt * 32 + ((h + r) & 3) + 8 * ((h + r) >> 2), bias_r[h + r]);
                    _Pragma("unroll") for (int r = 0; r < 8; r++) epi2_finish<A_>(p, yb, acc[mt][nt][h + r], e_[r]);
                }
            }
        }
    )
    RVC_KP(6);
}

}  // namespace rvc
