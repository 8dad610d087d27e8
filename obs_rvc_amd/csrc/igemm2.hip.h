// igemm2.hip.h -- igemm2_kernel, the register-direct 16x16x4 kernel of the one-stream latency chain (instantiated by igemm2_inst.hip, one unit per tile)
#pragma once
#include "igemm_common.hip.h"

namespace rvc {

// ------------------------------------------------------------------------------------------------------------------------
// igemm2_kernel -- the tile computation of igemm_splitk_kernel (the first-generation kernel) with a lean launch prologue / epilogue for the one-stream
// latency chain (measured with tests/tools/kprobe.py: of the 16 us a 0.5 GFLOP ContentVec GEMM took, 2.0 us went from wave
// entry to the first barrier -- scalar divisions for the tile index, a dependent global -> LDS copy of the offset table,
// 64-bit address arithmetic -- and 1.3 us into a branchy per-element epilogue):
//   * tile coordinates come from a 2-D grid (x = fast axis, y = slow axis, z = batch * nphase + phase): no divisions.  With
//     m_fast the fast axis is m and gridDim.x is a multiple of 8, so workgroup (x, y) still runs on XCD x % 8;
//   * the offset table is requested FIRST and written to LDS only after the index arithmetic, the epilogue operand requests
//     and the first D weight loads have been issued; with KS > 1 every wave stages just its own K slice (no workgroup barrier);
//   * LIN layers (1x1 convolution on a 1-D tensor = every Linear of the transformers) need no table at all: the k-th operand
//     row is k * channel stride, so the activation gathers leave together with the weight loads;
//   * epilogue addresses are 32-bit element offsets from per-batch bases, the activation is dispatched once per tile.
// Grid-level split-K (a table too long for LDS) stays on igemm_splitk_kernel.
// Minimum waves per SIMD the register allocation has to leave room for.  LNB: 264 registers otherwise -- one wave per SIMD.  The two others are the
// instantiations that round 5's two-path K loop pushed over an occupancy step (132 registers for the lone fragment with four K shares: three waves
// per SIMD instead of four, and RMVPE's 128-workgroup launches on the 32-CU partition took a second round: 81 -> 116 us per chunk; 172 for the 2 x 4
// tile with the fused input activation).
template <int MF, int NF, int KS, bool PRE, bool LIN, bool LNB> struct Ig2Occ {
    static constexpr int W = LNB ? 2 : ((MF * NF == 1 && KS == 4 && !PRE && !LIN) ? 4 : ((MF * NF == 8 && KS == 1 && PRE) ? 3 : 1));
};
template <int MF, int NF, int D, int KS, bool PRE, bool LIN, bool LNB = false>
__global__ __launch_bounds__((KS > 1 ? KS : 4) * 64) __attribute__((amdgpu_waves_per_eu(Ig2Occ<MF, NF, KS, PRE, LIN, LNB>::W)))
void igemm2_kernel(IgemmP p)
{
    static_assert(!LNB || (LIN && !PRE && KS > 1), "LayerNorm-consumer instantiations: table-free 1x1 layers with the in-workgroup K split");
    constexpr int WAVES = KS > 1 ? KS : 4;
    constexpr int NACC = (MF * NF == 1) ? 2 : 1;   // a lone fragment alternates two accumulators (MFMA dependency)
    constexpr int TE = MF * NF * 256;
    constexpr int PE = (KS > 1) ? ((TE + WAVES * 64 - 1) / (WAVES * 64)) : 1;
    constexpr bool PF = (KS > 1) || (MF * NF <= 4);
    constexpr int KR = 2;                         // offset-table entries (int4) a thread can hold between request and LDS write
    extern __shared__ __attribute__((aligned(16))) int s_koff[];
    RVC_KP(0);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int fast = KS > 1 ? (int)blockIdx.x : (int)blockIdx.x * 4 + wave, slow = (int)blockIdx.y;
    const int tm = p.m_fast ? fast : slow, tn = p.m_fast ? slow : fast;
    int phase = 0, b = 0;
    {
        const int z = (int)blockIdx.z;
        if (p.nphase == 1) b = z;
        else if (p.nbatch == 1) phase = z;
        else { b = z / p.nphase; phase = z - b * p.nphase; }
    }
    PhaseD ph = p.ph0;
    if (phase) ph = p.ph[phase];
    const int nchunks = ph.nchunks;
    // this wave's chunk range (KS > 1: the waves of the workgroup split K)
    int c0 = 0, nc = nchunks;
    if (KS > 1) {
        const int cpw = (nchunks + KS - 1) / KS;
        c0 = wave * cpw;
        int c1 = c0 + cpw;
        c1 = c1 < nchunks ? c1 : nchunks;
        nc = c1 > c0 ? c1 - c0 : 0;
    }
    // 1. request the offset-table slice (KS > 1: this wave's; KS == 1: the workgroup's) -- consumed after everything else is in flight
    int4 kr[KR];
    const int kt_n = LIN ? 0 : (KS > 1 ? nc * 4 : nchunks * 4);          // int4 entries to stage
    const int kt_i = KS > 1 ? lane : (int)threadIdx.x;
    constexpr int KT_STRIDE = KS > 1 ? 64 : WAVES * 64;
    const int4 *ksrc = reinterpret_cast<const int4 *>(p.koff + ph.koff_off) + (KS > 1 ? c0 * 4 : 0);
    int4 *kdst = reinterpret_cast<int4 *>(s_koff) + (KS > 1 ? c0 * 4 : 0);
    if (!LIN) {
#pragma unroll
        for (int r = 0; r < KR; r++) { const int i = kt_i + r * KT_STRIDE; if (i < kt_n) kr[r] = ksrc[i]; }
    }
    RVC_KP(8);
    const bool live = tm < p.ntm && tn < p.ntn;
    const int li = lane & 15, kq = lane >> 4;
    const float *resb = p.res ? p.res + (long long)b * p.res_bs : nullptr;
    float *yb = p.y + (long long)b * p.y_bs + ph.y_off;
    const int act_sel = ph.act_p1 ? ph.act_p1 - 1 : p.act;

    RVC_KP(9);
    // gathered-activation addressing: wave-uniform base + unsigned 32-bit BYTE offset per lane
    const char *xb = reinterpret_cast<const char *>(p.x + (long long)b * p.x_bs + ph.x_off) - (LIN ? 0 : p.koff_bias);
    unsigned xo[NF];
#pragma unroll
    for (int nf = 0; nf < NF; nf++) {
        int n = tn * 16 * NF + nf * 16 + li;
        n = n < p.N ? n : p.N - 1;
        int bb = 0;
        if (p.fold_n) { bb = n / p.fold_n; n -= bb * p.fold_n; }
        int nh = 0, nw = n;
        if (p.x_hs) { nh = n / p.NW; nw = n - nh * p.NW; }
        xo[nf] = (unsigned)(bb * (int)p.x_bs + nh * p.x_hs + nw * p.x_ws) * 4u;
        if (LIN) xo[nf] += (unsigned)((c0 * 16 + kq * 4) * p.lin_cs4);
    }
    // weights: MFMA-fragment order [m_tile][chunk][lane][4]
    const float *wrow[MF];
    const int mtiles = (p.M + 15) >> 4;
#pragma unroll
    for (int mf = 0; mf < MF; mf++) {
        int mt = tm * MF + mf;
        mt = mt < mtiles ? mt : mtiles - 1;
        wrow[mf] = p.w + ph.w_off + ((long long)mt * nchunks + c0) * 256 + lane * 4;
    }
    const int4 *kol = reinterpret_cast<const int4 *>(s_koff) + c0 * 4 + kq;
    const float pre_slope = p.pre_slope;
    const unsigned lin1 = (unsigned)p.lin_cs4, lin16 = 16u * (unsigned)p.lin_cs4;

    f32x4 acc[NACC][MF][NF];
#pragma unroll
    for (int a = 0; a < NACC; a++)
#pragma unroll
        for (int mf = 0; mf < MF; mf++)
#pragma unroll
            for (int nf = 0; nf < NF; nf++) acc[a][mf][nf] = (f32x4){0.f, 0.f, 0.f, 0.f};
    RVC_KP(10);

    f32x4 a_st[D][MF];
    float b_st[D][NF][4];
    // LNB: column sums of the operand values this lane feeds to the matrix core, taken relative to the column's FIRST element (every
    // lane and wave of a column loads the same one): the one-pass variance E[d^2] - E[d]^2 then cancels against a shift of the order
    // of the spread, not of the mean (a column with |mean| >> std would otherwise lose its variance to rounding)
    float ln_s[LNB ? NF : 1], ln_ss[LNB ? NF : 1], ln_c[LNB ? NF : 1];
#pragma unroll
    for (int nf = 0; nf < (LNB ? NF : 1); nf++) {
        ln_s[nf] = 0.f; ln_ss[nf] = 0.f;
        ln_c[nf] = LNB ? *reinterpret_cast<const float *>(xb + (xo[LNB ? nf : 0] - (unsigned)((c0 * 16 + kq * 4) * p.lin_cs4))) : 0.f;
    }
    int4 ko_nx = make_int4(0, 0, 0, 0);
#define RVC_LOAD_A(S, C)                                                                               \
    {                                                                                                  \
        _Pragma("unroll") for (int mf = 0; mf < MF; mf++) a_st[S][mf] = *reinterpret_cast<const f32x4 *>(wrow[mf] + (C) * 256); \
    }
#define RVC_LOAD_B(S, C)                                                                               \
    {                                                                                                  \
        const int cc_ = (C);                                                                           \
        int4 ko_;                                                                                      \
        if (LIN) { const unsigned kb_ = (unsigned)cc_ * lin16; ko_ = make_int4((int)kb_, (int)(kb_ + lin1), (int)(kb_ + 2u * lin1), (int)(kb_ + 3u * lin1)); } \
        else { ko_ = ko_nx; ko_nx = kol[(cc_ + 1 < nc ? cc_ + 1 : cc_) * 4]; }                         \
        _Pragma("unroll") for (int nf = 0; nf < NF; nf++) {                                            \
            b_st[S][nf][0] = *reinterpret_cast<const float *>(xb + (xo[nf] + (unsigned)ko_.x));        \
            b_st[S][nf][1] = *reinterpret_cast<const float *>(xb + (xo[nf] + (unsigned)ko_.y));        \
            b_st[S][nf][2] = *reinterpret_cast<const float *>(xb + (xo[nf] + (unsigned)ko_.z));        \
            b_st[S][nf][3] = *reinterpret_cast<const float *>(xb + (xo[nf] + (unsigned)ko_.w));        \
        }                                                                                              \
    }
#define RVC_COMPUTE_STAGE(S)                                                                          \
    {                                                                                                  \
        _Pragma("unroll") for (int j = 0; j < 4; j++)                                                  \
            _Pragma("unroll") for (int nf = 0; nf < NF; nf++) {                                        \
                const float bv_ = PRE ? fmaxf(b_st[S][nf][j], b_st[S][nf][j] * pre_slope) : b_st[S][nf][j]; \
                if (LNB) { const float d_ = bv_ - ln_c[LNB ? nf : 0]; ln_s[LNB ? nf : 0] += d_; ln_ss[LNB ? nf : 0] = fmaf(d_, d_, ln_ss[LNB ? nf : 0]); } \
                _Pragma("unroll") for (int mf = 0; mf < MF; mf++)                                      \
                    acc[j % NACC][mf][nf] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_st[S][mf][j], bv_, acc[j % NACC][mf][nf], 0, 0, 0); \
            }                                                                                          \
    }
#define RVC_LOAD_STAGE(S, C) { RVC_LOAD_A(S, C) RVC_LOAD_B(S, C) }
    // The K loop has TWO code paths (round 5).  The compiler's s_waitcnt counts at a loop head are the most conservative of all ways into the loop: with
    // the first D stages requested under `if (s < nc)` there is a path on which only stage 0 was requested, so the head of the steady-state loop (and
    // every stage of the tail loop) waited with vmcnt(0) -- for the loads issued a few MFMAs earlier, once per round of D chunks: the D-deep register
    // ring was drained every round and a one-stream wave (12-18 chunks) spent its life in two or three full memory round trips.  Now a wave with at
    // least D chunks takes a path on which every request of the prologue is unconditional and in stage order, the steady-state loop has that prologue
    // as its only way in (exact counts: stage s waits until (D - 1) stages' loads are outstanding), and the remainder is two straight-line drain
    // rounds; a wave with fewer chunks takes the short conditional path.
    // 3b (both paths). epilogue operands: requested BEHIND the first weight / activation loads (their address arithmetic alone is 0.8 us at a
    //     4-element share per thread; in front of the main loads it delayed every launch by that much)
    Epi2 pre_w[(KS > 1 || !PF) ? 1 : MF][(KS > 1 || !PF) ? 1 : NF][4];
    Epi2 pre_r[PE];
    float pre_ws[LNB ? PE : 1];
#define RVC_EPI_PREFETCH                                                                               \
    if (PF && live && !p.glu) {                                                                        \
        if (KS > 1) {                                                                                  \
            _Pragma("unroll") for (int q = 0; q < PE; q++) {                                           \
                const int e = threadIdx.x + q * WAVES * 64;                                            \
                const int l = e & 63; const int r = (e >> 6) & 3; const int f = e >> 8; const int mf = f / NF; const int nf = f - mf * NF; \
                pre_r[q] = (e < TE) ? epi2_prefetch(p, ph, resb, yb, tm * 16 * MF + mf * 16 + (l >> 4) * 4 + r, tn * 16 * NF + nf * 16 + (l & 15)) : epi2_none(); \
                if (LNB) { const int m_ = tm * 16 * MF + mf * 16 + (l >> 4) * 4 + r; pre_ws[LNB ? q : 0] = (e < TE && m_ < p.M) ? p.ln_wsum[ph.bias_off + m_] : 0.f; } \
            }                                                                                          \
        } else {                                                                                       \
            _Pragma("unroll") for (int nf = 0; nf < ((KS > 1 || !PF) ? 1 : NF); nf++) {                \
                const ColOut col = col_locate(p, ph, tn * 16 * NF + nf * 16 + li);                     \
                _Pragma("unroll") for (int mf = 0; mf < ((KS > 1 || !PF) ? 1 : MF); mf++)              \
                    _Pragma("unroll") for (int r = 0; r < 4; r++)                                      \
                        pre_w[mf][nf][r] = epi2_from_col(p, ph, resb, yb, col, tm * 16 * MF + mf * 16 + kq * 4 + r); \
            }                                                                                          \
        }                                                                                              \
    }
    // 4 (both paths). publish the offset table: registers -> LDS (the rare long tables finish with a plain copy loop)
#define RVC_PUBLISH_TABLE                                                                              \
    if (!LIN) {                                                                                        \
        _Pragma("unroll") for (int r = 0; r < KR; r++) { const int i = kt_i + r * KT_STRIDE; if (i < kt_n) kdst[i] = kr[r]; } \
        for (int i = kt_i + KR * KT_STRIDE; i < kt_n; i += KT_STRIDE) kdst[i] = ksrc[i];               \
        if (KS > 1) __builtin_amdgcn_s_waitcnt(0xC07F);      /* wave-private slice: LDS writes done (lgkmcnt(0)), no barrier */ \
        else lds_only_barrier();                                                                       \
    }
    // steady state of the fused form: every operand register is reloaded right after its last use, so the loads of the next round are interleaved
    // with the MFMAs of this one instead of forming a block during which the matrix pipe drains (measured at 64 streams: the 768 x 3072 projection
    // 75 -> 92 TF/s, the 768 x 768 one 61 -> 78 TF/s; no change at one stream)
#define RVC_FUSED_STAGE(S, C)                                                                          \
    {                                                                                                  \
        const int cc_ = (C);                                                                           \
        int4 ko_;                                                                                      \
        if (LIN) { const unsigned kb_ = (unsigned)cc_ * lin16; ko_ = make_int4((int)kb_, (int)(kb_ + lin1), (int)(kb_ + 2u * lin1), (int)(kb_ + 3u * lin1)); } \
        else { ko_ = ko_nx; ko_nx = kol[(cc_ + 1 < nc ? cc_ + 1 : cc_) * 4]; }                         \
        const unsigned kov_[4] = {(unsigned)ko_.x, (unsigned)ko_.y, (unsigned)ko_.z, (unsigned)ko_.w}; \
        _Pragma("unroll") for (int j = 0; j < 4; j++)                                                  \
            _Pragma("unroll") for (int nf = 0; nf < NF; nf++) {                                        \
                const float bv_ = PRE ? fmaxf(b_st[S][nf][j], b_st[S][nf][j] * pre_slope) : b_st[S][nf][j]; \
                if (LNB) { const float d_ = bv_ - ln_c[LNB ? nf : 0]; ln_s[LNB ? nf : 0] += d_; ln_ss[LNB ? nf : 0] = fmaf(d_, d_, ln_ss[LNB ? nf : 0]); } \
                _Pragma("unroll") for (int mf = 0; mf < MF; mf++)                                      \
                    acc[j % NACC][mf][nf] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_st[S][mf][j], bv_, acc[j % NACC][mf][nf], 0, 0, 0); \
                b_st[S][nf][j] = *reinterpret_cast<const float *>(xb + (xo[nf] + kov_[j]));            \
            }                                                                                          \
        /* the weights are reloaded BEHIND their last use (round 5).  Requested at the top of the stage into the same array, the new value lived in a \
           second register set next to a copy of the old one, and the loop-carried copies back (v_mov on registers a load had just been issued \
           into) were placed at the loop head: every round began by waiting for ALL outstanding loads */ \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        _Pragma("unroll") for (int mf = 0; mf < MF; mf++) a_st[S][mf] = *reinterpret_cast<const f32x4 *>(wrow[mf] + cc_ * 256); \
        __builtin_amdgcn_sched_barrier(0);                                                             \
    }
    // Not for the lone-fragment tile: with its two alternating accumulators (NACC = 2) the fused form computes garbage as soon as the loop is
    // entered (K >= 24 chunks; `test_every_tile_configuration_computes_the_same_convolution` with -DRVC_FUSE_ALL), with or without
    // scheduling barriers between the stages, while the same source with one accumulator per fragment is exact -- a code-generation
    // problem of that instantiation as far as could be determined.  Its 12-deep prefetch hides the load block anyway.
#ifdef RVC_FUSE_ALL
    constexpr bool kFuse = true;      // investigation build only
#else
    constexpr bool kFuse = NACC == 1;
#endif
    if (live && nc >= D) {
        // ---- the long path: at least D chunks for this wave (wave-uniform; uniform per workgroup when KS == 1, where all waves share nchunks)
        // 2. first D stages, unconditional and in stage order: weights (and, without a table, the activations) leave first
#pragma unroll
        for (int s = 0; s < D; s++) { RVC_LOAD_A(s, s) if (LIN) RVC_LOAD_B(s, s) }
        RVC_EPI_PREFETCH
        RVC_KP(11);
        RVC_PUBLISH_TABLE
        RVC_KP(1);
        if (!LIN) {
            ko_nx = kol[0];
#pragma unroll
            for (int s = 0; s < D; s++) RVC_LOAD_B(s, s)
        }
        RVC_KP(2);
        int c = 0;
        if (kFuse) {
            for (; c + 2 * D <= nc; c += D) {
#pragma unroll
                for (int s = 0; s < D; s++) RVC_FUSED_STAGE(s, c + s + D)
            }
        } else {
            for (; c + 2 * D <= nc; c += D) {
#pragma unroll
                for (int s = 0; s < D; s++) {
                    RVC_COMPUTE_STAGE(s)
                    __builtin_amdgcn_sched_barrier(0);
                    RVC_LOAD_STAGE(s, c + s + D)
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        // drain: D <= nc - c < 2 D.  Round one computes the D loaded stages and requests the last nc - c - D chunks; round two computes those.
        const int rem = nc - c - D;
#pragma unroll
        for (int s = 0; s < D; s++) {
            RVC_COMPUTE_STAGE(s)
            if (s < rem) RVC_LOAD_STAGE(s, c + s + D)
        }
#pragma unroll
        for (int s = 0; s < D; s++) {
            if (s < rem) RVC_COMPUTE_STAGE(s)
        }
    } else {
        // ---- the short path: fewer than D chunks (or a dead tile: nothing but the barrier the workgroup shares)
        if (live) {
#pragma unroll
            for (int s = 0; s < D; s++)
                if (s < nc) { RVC_LOAD_A(s, s) if (LIN) RVC_LOAD_B(s, s) }
        }
        RVC_EPI_PREFETCH
        RVC_KP(11);
        RVC_PUBLISH_TABLE
        RVC_KP(1);
        if (!live) { if (KS > 1) { /* whole workgroup is dead: uniform */ } return; }
        if (!LIN) {
            ko_nx = nc > 0 ? kol[0] : make_int4(0, 0, 0, 0);
#pragma unroll
            for (int s = 0; s < D; s++)
                if (s < nc) RVC_LOAD_B(s, s)
        }
        RVC_KP(2);
#pragma unroll
        for (int s = 0; s < D; s++) {
            if (s < nc) RVC_COMPUTE_STAGE(s)
        }
    }
#undef RVC_FUSED_STAGE
#undef RVC_EPI_PREFETCH
#undef RVC_PUBLISH_TABLE
#undef RVC_COMPUTE_STAGE
#undef RVC_LOAD_STAGE
#undef RVC_LOAD_A
#undef RVC_LOAD_B
    if (NACC == 2) {
#pragma unroll
        for (int mf = 0; mf < MF; mf++)
#pragma unroll
            for (int nf = 0; nf < NF; nf++) acc[0][mf][nf] += acc[NACC - 1][mf][nf];
    }
    RVC_KP(3);

    if (KS > 1) {
        // fixed-order reduction of the KS partial tiles through LDS, then every thread finishes its share of the tile
        float *red = reinterpret_cast<float *>(s_koff + (LIN ? 0 : nchunks * 16));     // [KS][TE]
#pragma unroll
        for (int mf = 0; mf < MF; mf++)
#pragma unroll
            for (int nf = 0; nf < NF; nf++)
#pragma unroll
                for (int r = 0; r < 4; r++) red[wave * TE + ((mf * NF + nf) * 4 + r) * 64 + lane] = acc[0][mf][nf][r];
        float *lst = red + KS * TE;                 // LNB: [KS][NF * 16][2] column sums of this wave's K slice
        if (LNB) {
#pragma unroll
            for (int nf = 0; nf < NF; nf++) {
                float s_ = ln_s[LNB ? nf : 0], q_ = ln_ss[LNB ? nf : 0];
                s_ += __shfl_xor(s_, 16, 64); q_ += __shfl_xor(q_, 16, 64);
                s_ += __shfl_xor(s_, 32, 64); q_ += __shfl_xor(q_, 32, 64);
                if (kq == 0) { lst[(wave * NF * 16 + nf * 16 + li) * 2] = s_; lst[(wave * NF * 16 + nf * 16 + li) * 2 + 1] = q_; }
            }
        }
        RVC_KP(4);
        __syncthreads();
        RVC_KP(5);
        if (p.glu) {
#pragma unroll
            for (int q = 0; q < PE; q++) {
                const int e = threadIdx.x + q * WAVES * 64;
                if (e >= TE) break;
                const int l = e & 63, r = (e >> 6) & 3, f = e >> 8, mf = f / NF, nf = f - mf * NF;
                if (r >= 2) continue;
                float v = 0.f, v2 = 0.f;
#pragma unroll
                for (int w = 0; w < KS; w++) { v += red[w * TE + e]; v2 += red[w * TE + e + 128]; }
                glu_store(p, ph, b, tm * 16 * MF + mf * 16 + (l >> 4) * 4 + r, tn * 16 * NF + nf * 16 + (l & 15), v, v2);
            }
            return;
        }
        // LNB: statistics of this lane's NF columns, summed over the waves' K slices in a fixed order
        float ln_mean[LNB ? NF : 1], ln_rstd[LNB ? NF : 1];
        if (LNB) {
#pragma unroll
            for (int nf = 0; nf < NF; nf++) {
                const int cl = nf * 16 + li;
                float s_ = 0.f, q_ = 0.f;
#pragma unroll
                for (int w = 0; w < KS; w++) { s_ += lst[(w * NF * 16 + cl) * 2]; q_ += lst[(w * NF * 16 + cl) * 2 + 1]; }
                const float msh = s_ * p.ln_inv_rows;                       // mean of (y - first element)
                const float var = fmaxf(q_ * p.ln_inv_rows - msh * msh, 0.f);
                const float mean = ln_c[LNB ? nf : 0] + msh;
                const float rstd = 1.0f / sqrtf(var + p.ln_eps);
                ln_mean[LNB ? nf : 0] = mean; ln_rstd[LNB ? nf : 0] = rstd;
                const int n_ = tn * 16 * NF + cl;
                if (p.ln_stats_out && tm == 0 && threadIdx.x < 16 && n_ < p.N) { p.ln_stats_out[2 * n_] = mean; p.ln_stats_out[2 * n_ + 1] = rstd; }
            }
        }
        float vsum[PE];
#pragma unroll
        for (int q = 0; q < PE; q++) {
            const int e = threadIdx.x + q * WAVES * 64;
            float v = 0.f;
            if (e < TE) {
#pragma unroll
                for (int w = 0; w < KS; w++) v += red[w * TE + e];
            }
            if (LNB && e < TE) {          // the folded LayerNorm: see IgemmP::ln_wsum (an element's column is (nf, lane & 15))
                const int nf = (e >> 8) % NF;
                v = ln_rstd[LNB ? nf : 0] * (v - ln_mean[LNB ? nf : 0] * pre_ws[LNB ? q : 0]);
            }
            vsum[q] = v;
        }
        RVC_ACT_DISPATCH_SEL(act_sel, 
            _Pragma("unroll") for (int q = 0; q < PE; q++) epi2_finish<A_>(p, yb, vsum[q], pre_r[q]);
        )
        RVC_KP(6);
        return;
    }
    // D layout of v_mfma_f32_16x16x4_f32: col = lane & 15, row = (lane >> 4) * 4 + reg
    if (p.glu) {
        float gb[MF][4];                 // the gate's biases: rows kq * 4 + {0, 1} (tanh half) and + {2, 3} (sigmoid half)
#pragma unroll
        for (int mf = 0; mf < MF; mf++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = tm * 16 * MF + mf * 16 + kq * 4 + r;
                gb[mf][r] = m < p.M ? p.bias[ph.bias_off + m] : 0.f;
            }
#pragma unroll
        for (int nf = 0; nf < NF; nf++) {
            const ColOut col = col_locate(p, ph, tn * 16 * NF + nf * 16 + li);
#pragma unroll
            for (int mf = 0; mf < MF; mf++)
#pragma unroll
                for (int r = 0; r < 2; r++)
                    glu_from_col_b(p, ph, yb, col, tm * 16 * MF + mf * 16 + kq * 4 + r, acc[0][mf][nf][r], acc[0][mf][nf][r + 2], gb[mf][r], gb[mf][r + 2]);
        }
        return;
    }
    if (PF) {
        RVC_ACT_DISPATCH_SEL(act_sel, 
            _Pragma("unroll") for (int mf = 0; mf < MF; mf++)
                _Pragma("unroll") for (int nf = 0; nf < NF; nf++)
                    _Pragma("unroll") for (int r = 0; r < 4; r++)
                        epi2_finish<A_>(p, yb, acc[0][mf][nf][r], pre_w[PF ? mf : 0][PF ? nf : 0][r]);
        )
    } else {
        // operands in store-free batches (a load cannot be hoisted above an earlier, possibly aliasing store: element-by-element
        // "load, store" costs one memory round trip per element -- see igemm32_kernel)
        ColOut cols[NF];
#pragma unroll
        for (int nf = 0; nf < NF; nf++) cols[nf] = col_locate(p, ph, tn * 16 * NF + nf * 16 + li);
        const bool has_aux = resb != nullptr || p.accumulate;
        if (!p.accumulate && (tm + 1) * 16 * MF <= p.M) {
            // common case (every row of the tile exists, plain store): small straight-line code, one predicate per 16-column block,
            // the residual loaded for a whole 16-row fragment before its stores (see igemm32_kernel's epilogue)
            const float slope = p.slope, scale = p.scale;
            const long long cs = p.y_cs, rcs = p.res_cs;
            RVC_ACT_DISPATCH_SEL(act_sel, 
                _Pragma("unroll") for (int mf = 0; mf < MF; mf++) {
                    const int m0 = tm * 16 * MF + mf * 16 + kq * 4;
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
                                yc[r * cs] = epi2_value<A_>(acc[0][mf][nf][r], bias_r[r], rr[nf][r], 0.f, slope, scale);
                        }
                }
            )
            RVC_KP(6);
            return;
        }
        RVC_ACT_DISPATCH_SEL(act_sel, 
            _Pragma("unroll") for (int mf = 0; mf < MF; mf++) {
                float bias_r[4];
                _Pragma("unroll") for (int r = 0; r < 4; r++) {
                    const int m = tm * 16 * MF + mf * 16 + kq * 4 + r;
                    bias_r[r] = (p.bias && m < p.M) ? p.bias[ph.bias_off + m] : 0.f;
                }
                _Pragma("unroll") for (int nf = 0; nf < NF; nf++) {
                    if (!has_aux) {
                        _Pragma("unroll") for (int r = 0; r < 4; r++) {
                            const int m = tm * 16 * MF + mf * 16 + kq * 4 + r;
                            const Epi2 e1 = epi2_plain(bias_r[r], (m < p.M && cols[nf].yo >= 0) ? cols[nf].yo + (m + ph.y_c0) * p.y_cs : -1);
                            epi2_finish<A_>(p, yb, acc[0][mf][nf][r], e1);
                        }
                    } else {
                        Epi2 e_[4];
                        _Pragma("unroll") for (int r = 0; r < 4; r++)
                            e_[r] = epi2_aux(p, ph, resb, yb, cols[nf], tm * 16 * MF + mf * 16 + kq * 4 + r, bias_r[r]);
                        _Pragma("unroll") for (int r = 0; r < 4; r++) epi2_finish<A_>(p, yb, acc[0][mf][nf][r], e_[r]);
                    }
                }
            }
        )
    }
    RVC_KP(6);
}

}  // namespace rvc
