// igemm_lds.hip.h -- igemm_lds_kernel, the workgroup-tiled 16x16x4 throughput kernel (instantiated by igemm_tiled_inst.hip)
#pragma once
#include "igemm_common.hip.h"

namespace rvc {

// Throughput-mode implicit GEMM (many streams batched: N = B*T is large).  Classic CDNA anatomy: a 256-thread
// workgroup owns a (WM*MF*16) x (WN*NF*16) tile; per K step of 16 the gathered activation tile [16][BN] is staged
// global -> registers -> LDS (double-buffered, one barrier per step, fused input LeakyReLU applied once per element)
// and read back as MFMA B fragments by all waves; weight fragments stream global -> registers in fragment order.
// Each activation element is fetched once per workgroup instead of once per wave.
template <int WM, int WN, int MF, int NF, bool PRE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void igemm_lds_kernel(IgemmP p)
{
    constexpr int BM = WM * MF * 16, BN = WN * NF * 16;
    constexpr int RS = BN + 4;                 // LDS row stride: the 4 k-rows read by one MFMA operand fall on disjoint bank groups
    constexpr int KR = 256 / BN > 0 ? 256 / BN : 1;   // k rows staged per pass
    constexpr int EPT = 16 / KR;               // staged elements per thread per K step
    static_assert(BN <= 256 && 256 % BN == 0, "BN must divide 256");
    extern __shared__ __attribute__((aligned(16))) int s_mem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WN, wn = wave % WN;
    // m fastest when the streams are folded into N, over XCD-local tile ids (xcd_tile_id): the m-tiles of ONE activation tile run on one XCD
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
    float *bt = reinterpret_cast<float *>(s_mem + nchunks * 16);     // [2][16][RS]
    const int li = lane & 15, kq = lane >> 4;
    const char *xb = reinterpret_cast<const char *>(p.x + (long long)b * p.x_bs + ph.x_off) - p.koff_bias;
    // staging role: column n_s of the tile, k rows kr0, kr0 + KR, ...
    const int n_s = threadIdx.x % BN, kr0 = threadIdx.x / BN;
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
    const float *wrow[MF];
    const int mtiles = (p.M + 15) >> 4;
#pragma unroll
    for (int mf = 0; mf < MF; mf++) {
        int mt = (tm * WM + wm) * MF + mf;
        mt = mt < mtiles ? mt : mtiles - 1;
        wrow[mf] = p.w + ph.w_off + (long long)mt * nchunks * 256 + lane * 4;
    }
    f32x4 acc[MF][NF];
#pragma unroll
    for (int mf = 0; mf < MF; mf++)
#pragma unroll
        for (int nf = 0; nf < NF; nf++) acc[mf][nf] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float pre_slope = p.pre_slope;
    __syncthreads();
    const int *kof = s_mem;
    float sb[EPT];
    f32x4 a_cur[MF], a_nxt[MF];
#pragma unroll
    for (int i = 0; i < EPT; i++) sb[i] = *reinterpret_cast<const float *>(xb + (xo_s + (unsigned)kof[kr0 + i * KR]));
#pragma unroll
    for (int mf = 0; mf < MF; mf++) a_cur[mf] = *reinterpret_cast<const f32x4 *>(wrow[mf]);
#pragma unroll
    for (int i = 0; i < EPT; i++) {
        const float v = sb[i];
        bt[(kr0 + i * KR) * RS + n_s] = PRE ? fmaxf(v, v * pre_slope) : v;
    }
    __syncthreads();
    const float *br = bt + wn * NF * 16 + li + kq * 4 * RS;
    for (int c = 0; c < nchunks; c++) {
        const int cn = c + 1 < nchunks ? c + 1 : c;
        const float *bcur = br + (c & 1) * 16 * RS;
        float *bnxt = bt + ((c + 1) & 1) * 16 * RS;
        // prefetch the next K step (global -> registers)
#pragma unroll
        for (int i = 0; i < EPT; i++) sb[i] = *reinterpret_cast<const float *>(xb + (xo_s + (unsigned)kof[cn * 16 + kr0 + i * KR]));
#pragma unroll
        for (int mf = 0; mf < MF; mf++) a_nxt[mf] = *reinterpret_cast<const f32x4 *>(wrow[mf] + cn * 256);
        float bv[NF][4];
#pragma unroll
        for (int nf = 0; nf < NF; nf++)
#pragma unroll
            for (int j = 0; j < 4; j++) bv[nf][j] = bcur[j * RS + nf * 16];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int mf = 0; mf < MF; mf++)
#pragma unroll
                for (int nf = 0; nf < NF; nf++)
                    acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[mf][j], bv[nf][j], acc[mf][nf], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < EPT; i++) {
            const float v = sb[i];
            bnxt[(kr0 + i * KR) * RS + n_s] = PRE ? fmaxf(v, v * pre_slope) : v;
        }
#pragma unroll
        for (int mf = 0; mf < MF; mf++) a_cur[mf] = a_nxt[mf];
        __syncthreads();
    }
    const float *resb = p.res ? p.res + (long long)b * p.res_bs : nullptr;
    float *yb = p.y + (long long)b * p.y_bs;
    ColOut cols[NF];
#pragma unroll
    for (int nf = 0; nf < NF; nf++) cols[nf] = col_locate(p, ph, tn * BN + (wn * NF + nf) * 16 + li);
    // operands in store-free batches (see igemm32_kernel's epilogue): the four biases of a 16-row fragment, then per 16x16 block
    if (p.glu) {
#pragma unroll
        for (int mf = 0; mf < MF; mf++) {
            float gb[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = ((tm * WM + wm) * MF + mf) * 16 + kq * 4 + r;
                gb[r] = m < p.M ? p.bias[ph.bias_off + m] : 0.f;
            }
#pragma unroll
            for (int nf = 0; nf < NF; nf++)
#pragma unroll
                for (int r = 0; r < 2; r++)
                    glu_from_col_b(p, ph, yb, cols[nf], ((tm * WM + wm) * MF + mf) * 16 + kq * 4 + r, acc[mf][nf][r], acc[mf][nf][r + 2], gb[r], gb[r + 2]);
        }
        return;
    }
    const bool has_aux = resb != nullptr || p.accumulate;
    if (!p.accumulate && (tm * WM + wm + 1) * MF * 16 <= p.M) {
        // common case: small straight-line code (see igemm32_kernel's epilogue)
        const float slope = p.slope, scale = p.scale;
        const long long cs = p.y_cs, rcs = p.res_cs;
        RVC_ACT_DISPATCH(
            _Pragma("unroll") for (int mf = 0; mf < MF; mf++) {
                const int m0 = ((tm * WM + wm) * MF + mf) * 16 + kq * 4;
                float bias_r[4];
                _Pragma("unroll") for (int r = 0; r < 4; r++) bias_r[r] = p.bias ? p.bias[ph.bias_off + m0 + r] : 0.f;
                float rr[NF][4];
                _Pragma("unroll") for (int nf = 0; nf < NF; nf++)
                    _Pragma("unroll") for (int r = 0; r < 4; r++) rr[nf][r] = 0.f;
                if (resb) {
                    _Pragma("unroll") for (int nf = 0; nf < NF; nf++)
                        if (cols[nf].yo >= 0) {
                            const float *rp = resb + cols[nf].ro + (long long)(p.res_nogroup ? m0 : m0 + ph.y_c0) * rcs;
                            _Pragma("unroll") for (int r = 0; r < 4; r++) rr[nf][r] = rp[r * rcs];
                        }
                }
                _Pragma("unroll") for (int nf = 0; nf < NF; nf++)
                    if (cols[nf].yo >= 0) {
                        float *yc = yb + cols[nf].yo + (long long)(m0 + ph.y_c0) * cs;
                        _Pragma("unroll") for (int r = 0; r < 4; r++)
                            yc[r * cs] = epi2_value<A_>(acc[mf][nf][r], bias_r[r], rr[nf][r], 0.f, slope, scale);
                    }
            }
        )
        return;
    }
    RVC_ACT_DISPATCH(
        _Pragma("unroll") for (int mf = 0; mf < MF; mf++) {
            float bias_r[4];
            _Pragma("unroll") for (int r = 0; r < 4; r++) {
                const int m = ((tm * WM + wm) * MF + mf) * 16 + kq * 4 + r;
                bias_r[r] = (p.bias && m < p.M) ? p.bias[ph.bias_off + m] : 0.f;
            }
            _Pragma("unroll") for (int nf = 0; nf < NF; nf++) {
                if (!has_aux) {
                    _Pragma("unroll") for (int r = 0; r < 4; r++) {
                        const int m = ((tm * WM + wm) * MF + mf) * 16 + kq * 4 + r;
                        const Epi2 e1 = epi2_plain(bias_r[r], (m < p.M && cols[nf].yo >= 0) ? cols[nf].yo + (m + ph.y_c0) * p.y_cs : -1);
                        epi2_finish<A_>(p, yb, acc[mf][nf][r], e1);
                    }
                } else {
                    Epi2 e_[4];
                    _Pragma("unroll") for (int r = 0; r < 4; r++)
                        e_[r] = epi2_aux(p, ph, resb, yb, cols[nf], ((tm * WM + wm) * MF + mf) * 16 + kq * 4 + r, bias_r[r]);
                    _Pragma("unroll") for (int r = 0; r < 4; r++) epi2_finish<A_>(p, yb, acc[mf][nf][r], e_[r]);
                }
            }
        }
    )
}

}  // namespace rvc
