// igemm2w.hip.h -- igemm2w_kernel, register-direct 32x32x2 tiles for the table-free 1x1 layers at a few streams (instantiated by igemm2w_inst.hip)
#pragma once
#include "igemm_common.hip.h"

namespace rvc {

typedef float f32x16w __attribute__((ext_vector_type(16)));
// ------------------------------------------------------------------------------------------------------------------------
// igemm2w_kernel -- register-direct implicit GEMM on v_mfma_f32_32x32x2_f32 for the table-free 1x1 layers (every Linear of the
// transformers) at a FEW streams (round 5: the regime between the one-stream latency kernels and the many-stream LDS-staged tiles).
// One wave owns a (32 MT) x (32 NT) output tile; the KS waves of a workgroup split K and meet in a fixed-order LDS reduction
// (deterministic).  No LDS staging: with the streams folded into N a layer has too few tiles for a workgroup tile to share its
// activation operand across enough rows, and an in-workgroup K split of a staged tile multiplies the staging per MFMA; here the
// K split costs nothing but the final reduction.  What the 32x32x2 form buys over igemm2_kernel's 16x16x4 fragments: one activation
// gather (a dword per lane: 32 consecutive columns of two k rows) feeds a 64-clock MFMA instead of a 32-clock one, and a weight
// float4 feeds NT * 4 of them -- 20 vector-memory instructions per 32 MFMAs of 64 clocks (2 x 2 blocks) against 10 per 16 of 32
// clocks: half the instructions per matrix-pipe clock, and an fp32 MFMA hides none of them (tests/tools/mfma_overlap_probe.hip).
// Operand order inside a 16-deep chunk: MFMA (u, j) takes k = (2u + ks) * 4 + j, ks = lane >> 5 -- the weights come straight from the
// 16-row fragment packing (lane (row r, k-slot ks) reads the float4 of fragment r >> 4, quad 2u + ks), as in igemm32_kernel.
// LNB (round 6; 32 x 32 tile, K split only): the layer consumes a NOT yet normalised tensor -- igemm2_kernel's folded LayerNorm (IgemmP::ln_wsum) on this
// kernel, for the one-stream QKV / first FFN projections (isolated 12.4 / 13.4 -> 9.5 / 10.0 us against igemm2_kernel's LNB tiles).  A lane adds up its
// operand values relative to the column's first element (2 of the 4 k rows of every MFMA are this lane's, the partner lane holds the others), the K shares
// meet in LDS next to the partial tiles in wave order, and the correction rstd * (acc - mean * wsum[m]) is applied in front of the epilogue.
template <int MT, int NT, int KS, bool LNB = false>
__global__ __launch_bounds__(KS * 64) void igemm2w_kernel(IgemmP p)
{
    static_assert(!LNB || (MT == 1 && NT == 1 && KS > 1), "LayerNorm-consumer instantiations: 32 x 32 wave tile with the in-workgroup K split");
    constexpr int D = MT * NT >= 4 ? 2 : 3;             // chunks in flight per wave
    constexpr int TE = MT * NT * 1024;                  // elements of the wave tile
    constexpr int PE = KS > 1 ? (TE + KS * 64 - 1) / (KS * 64) : 1;     // elements a thread finishes after the reduction
    extern __shared__ __attribute__((aligned(16))) float s_red[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int fast = (int)blockIdx.x, slow = (int)blockIdx.y;
    const int tm = p.m_fast ? fast : slow, tn = p.m_fast ? slow : fast;
    if (tm >= p.ntm || tn >= p.ntn) return;             // padding of the XCD-aware order (uniform per workgroup)
    const PhaseD &ph = p.ph0;
    const int nchunks = ph.nchunks;
    int c0 = 0, nc = nchunks;
    if (KS > 1) {
        const int cpw = (nchunks + KS - 1) / KS;
        c0 = wave * cpw;
        int c1 = c0 + cpw;
        c1 = c1 < nchunks ? c1 : nchunks;
        nc = c1 > c0 ? c1 - c0 : 0;
    }
    const int c32 = lane & 31, ks = lane >> 5;
    const float *resb = p.res;
    float *yb = p.y + ph.y_off;
    // activations: wave-uniform base + 32-bit byte offset per lane (column of this lane, k rows c0 * 16 + ks * 4 ...)
    const char *xb = reinterpret_cast<const char *>(p.x + ph.x_off);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(xb), 0, 0x7ffff000, 0x00020000);      // raw buffer, 32-bit data format
    const unsigned lin1 = (unsigned)p.lin_cs4;
    // (one byte offset per gather of a chunk, fixed for the whole launch: the chunk's position goes into the wave-uniform base pointer, so a gather
    //  costs no vector ALU instruction)
    unsigned xo[NT][8];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        int n = (tn * NT + nt) * 32 + c32;
        n = n < p.N ? n : p.N - 1;
        int bb = 0;
        if (p.fold_n) { bb = n / p.fold_n; n -= bb * p.fold_n; }
        const unsigned o = (unsigned)(bb * (int)p.x_bs + n * p.x_ws) * 4u + (unsigned)(c0 * 16 + ks * 4) * lin1;
#pragma unroll
        for (int q = 0; q < 8; q++) xo[nt][q] = o + (unsigned)((q >> 2) * 8 + (q & 3)) * lin1;
    }
    // weights: the same addressing (all vector-memory instructions of the loop are buffer loads: one kind of load, so the compiler's
    // s_waitcnt counts stay exact -- with global loads for the weights next to buffer loads for the activations it waited for the NEWEST
    // stage's loads before the oldest stage's MFMAs)
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.w + ph.w_off), 0, 0x7ffff000, 0x00020000);
    unsigned wo[MT];
    const int mtiles = (p.M + 15) >> 4;
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        int t16 = (tm * MT + mt) * 2 + (c32 >> 4);
        t16 = t16 < mtiles ? t16 : mtiles - 1;
        wo[mt] = (unsigned)(((long long)t16 * nchunks + c0) * 256 + (ks * 16 + (c32 & 15)) * 4) * 4u;
    }
    f32x16w acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[mt][nt][r] = 0.f;
    // LNB: sums of (value - first element of the column) and of its square over this lane's k rows (a buffer load like every other load of the kernel)
    float ln_s = 0.f, ln_ss = 0.f, ln_c = 0.f;
    float ln_ws[LNB ? PE : 1];                      // wsum of the rows this thread finishes: requested now, consumed behind the reduction
    if (LNB) {
        ln_c = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, (int)(xo[0][0] - (unsigned)(c0 * 16 + ks * 4) * lin1), 0, 0));
        const __amdgpu_buffer_rsrc_t sr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.ln_wsum + ph.bias_off), 0, 0x7ffff000, 0x00020000);
#pragma unroll
        for (int q = 0; q < PE; q++) {
            const int e = (int)threadIdx.x + q * KS * 64;
            int m_ = tm * 32 + ((e >> 6) & 3) + 8 * (((e >> 6) & 15) >> 2) + 4 * ((e & 63) >> 5);
            m_ = m_ < p.M ? m_ : p.M - 1;
            ln_ws[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(sr, m_ * 4, 0, 0));
        }
    }
    f32x4 a_st[D][MT][2];
    float b_st[D][NT][8];
    auto load = [&](f32x4 (&a)[MT][2], float (&b)[NT][8], const int c) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int u = 0; u < 2; u++) a[mt][u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wr, (int)wo[mt], c * 1024 + u * 512, 0));
        // buffer loads: per-lane byte offset in a VGPR that never changes, the chunk's offset in an SGPR -- no vector ALU work per gather
        const int so = (int)((unsigned)c * 16u * lin1);
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int q = 0; q < 8; q++) b[nt][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, (int)xo[nt][q], so, 0));
    };
    auto compute = [&](const f32x4 (&a)[MT][2], const float (&b)[NT][8]) {
        if (LNB) {
#pragma unroll
            for (int q = 0; q < 8; q++) { const float d_ = b[0][q] - ln_c; ln_s += d_; ln_ss = fmaf(d_, d_, ln_ss); }
        }
#pragma unroll
        for (int u = 0; u < 2; u++)
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int nt = 0; nt < NT; nt++)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt][u][j], b[nt][u * 4 + j], acc[mt][nt], 0, 0, 0);
    };
    // (the first D stages leave unconditionally and in stage order: the compiler's s_waitcnt counts at the loop head are the more conservative of the
    //  ways into the loop, and with a conditional prologue -- a path on which the second stage was never requested -- every iteration waited for the
    //  NEWEST stage's loads before computing the oldest)
#pragma unroll
    for (int s = 0; s < D; s++) {
        load(a_st[s], b_st[s], s < nc ? s : (nc > 0 ? nc - 1 : 0));      // unconditional (a stage past the wave's range re-reads its last chunk and is never used)
        __builtin_amdgcn_sched_barrier(0);
    }
    int c = 0;
    for (; c + 2 * D <= nc; c += D) {
#pragma unroll
        for (int s = 0; s < D; s++) {
            compute(a_st[s], b_st[s]);
            __builtin_amdgcn_sched_barrier(0);
            load(a_st[s], b_st[s], c + s + D);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    for (; c < nc; c += D) {
#pragma unroll
        for (int s = 0; s < D; s++) {
            if (c + s < nc) {
                compute(a_st[s], b_st[s]);
                if (c + s + D < nc) load(a_st[s], b_st[s], c + s + D);
            }
        }
    }
    // C / D layout of the 32x32 block: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    if (KS > 1) {
        // fixed-order reduction of the KS partial tiles through LDS; every thread then finishes its share of the tile (consecutive
        // threads = consecutive columns: coalesced stores)
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
#pragma unroll
                for (int r = 0; r < 16; r++) s_red[wave * TE + ((mt * NT + nt) * 16 + r) * 64 + lane] = acc[mt][nt][r];
        float *lst = s_red + KS * TE;               // LNB: [KS][32 columns][2] sums of this wave's K share
        if (LNB) {
            const float s_ = ln_s + __shfl_xor(ln_s, 32, 64), q_ = ln_ss + __shfl_xor(ln_ss, 32, 64);        // the partner lane holds the other two k rows of every MFMA
            if (ks == 0) { lst[(wave * 32 + c32) * 2] = s_; lst[(wave * 32 + c32) * 2 + 1] = q_; }
        }
        __syncthreads();
        // LNB: statistics of this thread's column -- every element a thread finishes lies in column threadIdx.x & 31 = this lane's operand column --, the
        // K shares summed in wave order; the tm == 0 workgroups publish (mean, rstd) for the later layer whose residual is LayerNorm(y)
        float ln_mean = 0.f, ln_rstd = 0.f;
        if (LNB) {
            float s_ = 0.f, q_ = 0.f;
#pragma unroll
            for (int w = 0; w < KS; w++) { s_ += lst[(w * 32 + c32) * 2]; q_ += lst[(w * 32 + c32) * 2 + 1]; }
            const float msh = s_ * p.ln_inv_rows;
            const float var = fmaxf(q_ * p.ln_inv_rows - msh * msh, 0.f);
            ln_mean = ln_c + msh; ln_rstd = 1.0f / sqrtf(var + p.ln_eps);
            const int n_ = tn * 32 + c32;
            if (p.ln_stats_out && tm == 0 && threadIdx.x < 32 && n_ < p.N) { p.ln_stats_out[2 * n_] = ln_mean; p.ln_stats_out[2 * n_ + 1] = ln_rstd; }
        }
        // (batches of eight: a whole-share batch of 32 elements took the 64 x 64 tile with two waves to 288 registers)
        constexpr int EB = PE < 8 ? PE : 8;
        RVC_ACT_DISPATCH(
            for (int q0 = 0; q0 < PE; q0 += EB) {
                float v[EB];
                Epi2 ep[EB];
                _Pragma("unroll") for (int qq = 0; qq < EB; qq++) {
                    const int e = (int)threadIdx.x + (q0 + qq) * KS * 64;
                    const bool in = q0 + qq < PE && e < TE;
                    float sum = 0.f;
                    if (in) {
                        _Pragma("unroll") for (int w = 0; w < KS; w++) sum += s_red[w * TE + e];
                    }
                    const int l = e & 63; const int r = (e >> 6) & 15; const int f = e >> 10; const int mt = f / NT; const int nt = f - mt * NT;
                    if (LNB && in) sum = ln_rstd * (sum - ln_mean * ln_ws[LNB ? q0 + qq : 0]);          // the folded LayerNorm: out = rstd[n] * (acc - mean[n] * wsum[m]) (+ the folded bias in the epilogue)
                    v[qq] = sum;
                    ep[qq] = in ? epi2_prefetch(p, ph, resb, yb, (tm * MT + mt) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), (tn * NT + nt) * 32 + (l & 31)) : epi2_none();
                }
                _Pragma("unroll") for (int qq = 0; qq < EB; qq++) epi2_finish<A_>(p, yb, v[qq], ep[qq]);
            }
        )
        return;
    }
    ColOut cols[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) cols[nt] = col_locate(p, ph, (tn * NT + nt) * 32 + c32);
    RVC_ACT_DISPATCH(
        _Pragma("unroll") for (int mt = 0; mt < MT; mt++) {
            float bias_r[16];
            _Pragma("unroll") for (int r = 0; r < 16; r++) {
                const int m = (tm * MT + mt) * 32 + ks * 4 + (r & 3) + 8 * (r >> 2);
                bias_r[r] = (p.bias && m < p.M) ? p.bias[ph.bias_off + m] : 0.f;
            }
            _Pragma("unroll") for (int nt = 0; nt < NT; nt++) {
                _Pragma("unroll") for (int h = 0; h < 16; h += 8) {
                    Epi2 e_[8];
                    _Pragma("unroll") for (int r = 0; r < 8; r++)
                        e_[r] = epi2_aux(p, ph, resb, yb, cols[nt], (tm * MT + mt) * 32 + ks * 4 + ((h + r) & 3) + 8 * ((h + r) >> 2), bias_r[h + r]);
                    _Pragma("unroll") for (int r = 0; r < 8; r++) epi2_finish<A_>(p, yb, acc[mt][nt][h + r], e_[r]);
                }
            }
        }
    )
}

}  // namespace rvc
