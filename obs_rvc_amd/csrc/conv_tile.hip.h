// conv_tile.hip.h -- stride-1 1-D convolutions of ONE stream whose output is long (the HiFiGAN decoder's ResBlock chains: N = 2 520 .. 10 080
// columns, 32 .. 128 channels) as an implicit GEMM whose activation operand is staged ONCE per workgroup.
//
// Why (measured, tests/tools/ta_probe.hip + kprobe.py): the register-direct kernel (igemm2) gathers the B operand with one dword load per
// MFMA k-step and 16-column fragment -- a CU retires such a load every 9-12 clocks, so a 2 x 2 fragment tile spends ~500 clocks of
// vector-memory issue per 16-deep K chunk beside its 512 clocks of MFMA, after a 5 us prologue of table / address / first-gather latency.
// Here the workgroup copies the raw input rows it needs -- [Cin][BN + (KW - 1) * dil] floats -- into LDS with LDS-DMA loads
// (global_load_lds_dword: no registers, everything in flight at once), applies the fused input LeakyReLU once and turns the tile to
// channel-contiguous columns in the same pass.  K is walked tap-major in chunks of 16 channels (the weights are repacked to that order at
// plan time), so the four k-values a lane feeds to an MFMA are ONE ds_read_b128 at a wave-uniform offset from a per-lane base: no offset
// table, no per-element address arithmetic (a first version with [channel][column] rows, an LDS offset table and four ds_read_b32 per
// fragment spent ~40 issue slots per 8 MFMAs and ran at 460 clocks per chunk against 256 of MFMA time -- a wave hides about five
// instructions per MFMA).  The only vector-memory traffic of the main loop is the weight stream (fragment-major, 1 KB per load,
// prefetched DA chunks ahead).  The four waves split M (and N for 32-channel layers): no K split, no reduction, no barrier in the loop.
//
// Work items (phase, m-tile, n-tile) are handed to workgroups through a table built at plan time: the hardware places workgroup b on
// CU b % 256 (tests/tools/place_probe.hip), so the table pairs long items (kernel size 11) with short ones (kernel size 3) on a CU
// instead of leaving the balance to the dispatch order.
//
// Two bodies share the item table, the IgemmP / PhaseD fields and the epilogue semantics (bias -> activation -> residual -> scale -> accumulate, y_c0
// grouping, per-phase activation and output, nothing written outside the output interior):
//   conv_tile_kernel    16x16x4 fragments, the whole [Cin][BN + reach] input staged once (above); LDS grows with Cin (up to 100 KB).
//   conv_tile32_kernel  32x32x2 fragments, conv32s_kernel's scheme cut to one-stream items: K is walked (32-channel block, tap, channel group)-major
//                       from the per-model panels of c32s_panel (no repack per plan), the block [32][BN + reach] is staged once per block with the
//                       input LeakyReLU applied once, the B operand is one ds_read_b128 per four k-steps.  A 32x32x2 MFMA needs half the operand
//                       reads per flop of a 16x16x4 one, and a tile stages BN + reach columns for BN = 32 .. 128 outputs instead of 16 .. 64.
//                       Every wave owns ONE 32 x 32 accumulator; tiles (WM x WN waves, KS K shares; four waves always):
//                         128 x 32 (4, 1, 1), 64 x 64 (2, 2, 1), 32 x 128 (1, 4, 1): the waves split M, then N;
//                         64 x 32 (2, 1, 2), 32 x 64 (1, 2, 2): half the height, the freed waves take the odd 16-deep chunk of every tap (channel
//                         group 1 of the block), summed in one fixed-order LDS reduction at the end -- the forms whose item count and length match
//                         the 16x16x4 tiles', i.e. the ones the one-stream item table balances.
//                       LDS: two buffers (block b + 1 is written while block b is read: one barrier per block change) of (BN + reach) x 36 floats,
//                       reach = (KW - 1) * dil <= 64, independent of Cin; at the decoder's reach of 50: BN = 32 23 616 B, BN = 64 32 832 B,
//                       BN = 128 51 264 B (the K shares' reduction, 8 KB, reuses them).
#pragma once
#include "igemm_common.hip.h"
#include "conv32s.hip.h"

namespace rvc {

#define COMMA_ ,
#ifndef RVC_CT_DBG
#define RVC_CT_DBG 0          // ablation builds (tests/tools/ct_ablate.sh): 1 no weight reloads, 2 no B reads, 8 no MFMAs (timing only)
#endif
template <int ACT, int MF, int NF>
__device__ __forceinline__ void conv_tile_store(const IgemmP &p, const PhaseD &ph, const float *resb, float *yb, const ColOut (&cols)[NF], int m_base, const f32x4 (&acc)[MF][NF])
{
    const float slope = p.slope, scale = p.scale;
    const long long cs = p.y_cs, rcs = p.res_cs;
#pragma unroll
    for (int mf = 0; mf < MF; mf++) {
        const int m0 = m_base + mf * 16;
        float bias_r[4];
#pragma unroll
        for (int r = 0; r < 4; r++) bias_r[r] = (p.bias && m0 + r < p.M) ? p.bias[ph.bias_off + m0 + r] : 0.f;
#pragma unroll
        for (int nf = 0; nf < NF; nf++) {
            if (cols[nf].yo < 0) continue;
            float rr[4] = {0.f, 0.f, 0.f, 0.f}, yo[4] = {0.f, 0.f, 0.f, 0.f};
            float *yc = yb + cols[nf].yo + (long long)(m0 + ph.y_c0) * cs;
            if (resb) {
                const float *rp = resb + cols[nf].ro + (long long)(p.res_nogroup ? m0 : m0 + ph.y_c0) * rcs;
#pragma unroll
                for (int r = 0; r < 4; r++) if (m0 + r < p.M) rr[r] = rp[r * rcs];
            }
            if (p.accumulate) {
#pragma unroll
                for (int r = 0; r < 4; r++) if (m0 + r < p.M) yo[r] = yc[r * cs];
            }
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (m0 + r < p.M) yc[r * cs] = epi2_value<ACT>(acc[mf][nf][r], bias_r[r], rr[r], yo[r], slope, scale);
        }
    }
}

// KS = 2: eight waves, the two waves that share a SIMD take the even / odd K chunks of the same fragments (one wave per SIMD cannot hide its own
// weight loads: their issue blocks behind the CU's single vector-memory path for 20-40 clocks each) and are summed through LDS at the end.
template <int WM, int WN, int MF, int NF, int KS>
__global__ __launch_bounds__(64 * WM * WN * KS) __attribute__((amdgpu_waves_per_eu(2))) void conv_tile_kernel(IgemmP p)
{
    static_assert(KS == 1 || KS == 2, "one or two K shares");
    constexpr int WPS = WM * WN, NT = 64 * WPS * KS;       // waves per K share, threads
    constexpr int BM = WM * MF * 16, BN = WN * NF * 16;
    constexpr int DA = MF == 1 ? 8 : 6;            // weight chunks in flight per wave
    extern __shared__ __attribute__((aligned(16))) int s_mem[];
    const int item = p.items[2 * blockIdx.x];
    if (item < 0) return;
    RVC_KP(0);
    const int phase = item & 0xff, tm = (item >> 8) & 0xff, tn = item >> 16;
    const int b = p.items[2 * blockIdx.x + 1];
    const PhaseD ph = p.nphase == 1 ? p.ph0 : p.ph[phase];
    const int nchunks = ph.nchunks;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int kh = wave / WPS, w4 = wave % WPS;     // K share, wave inside the share
    const int wm = w4 / WN, wn = w4 % WN;
    const int li = lane & 15, kq = lane >> 4;
    const int cin = ph.t_cin, rt = ph.t_rs, kw = ph.t_tab & 0xff, dil = ph.t_tab >> 8;
    const int rl = BN + (kw - 1) * dil;             // input columns the tile reads
    const int cs = cin + 8;                         // channel-contiguous tile: column stride (16 lanes x 16 bytes of a ds_read_b128 on disjoint banks)
    const int G = cin >> 4;
    float *tmp = reinterpret_cast<float *>(s_mem);  // [cin][rt] as it arrives (rt odd)
    const int tmp_n = (cin * rt + 63) & ~63;
    float *fin = tmp + (tmp_n > WPS * MF * NF * 256 ? tmp_n : WPS * MF * NF * 256);     // [rl][cs] activated, channel-contiguous (tmp later holds the K shares' partial sums)
    // 1. input rows -> LDS (LDS-DMA: wave-uniform destination + lane * 4; coalesced along the rows)
    {
        const float *xb = p.x + (long long)b * p.x_bs + ph.x_off;
        const int n0 = tn * BN + ph.t_dmin;
        const int total = cin * rt;
        const float inv_rt = 1.0f / (float)rt;
        for (int q = wave; q * 64 < total; q += WPS * KS) {
            const int e = q * 64 + lane;
            int row = (int)(((float)e + 0.5f) * inv_rt);
            const int col = e - row * rt;
            row = row < cin ? row : cin - 1;
            int gc = n0 + col;
            gc = gc < p.x_lo ? p.x_lo : (gc > p.x_lim ? p.x_lim : gc);
            __builtin_amdgcn_global_load_lds(xb + (long long)row * p.x_ld + gc, (__attribute__((address_space(3))) void *)(tmp + q * 64), 4, 0, 0);
        }
    }
    RVC_KP(1);
    // 2. weights: MFMA-fragment order [m_tile][chunk][lane][4] in THIS kernel's K order (chunk = tap * G + channel group, k = 4 * kq + j the
    //    channel inside the group: repacked at plan time); the first DA chunks leave behind the staging loads
    const float *wrow[MF];
    const int mtiles = (p.M + 15) >> 4;
#pragma unroll
    for (int mf = 0; mf < MF; mf++) {
        int mt = (tm * WM + wm) * MF + mf;
        mt = mt < mtiles ? mt : mtiles - 1;
        wrow[mf] = p.w + ph.w_off + (long long)mt * nchunks * 256;          // wave-uniform; the lane's 16 bytes are added at the load
    }
    const int nloc = (nchunks - kh + KS - 1) / KS;     // this wave's chunks: kh, kh + KS, ...  (>= 1: nchunks >= KS is checked at plan time)
    const unsigned lane16 = (unsigned)lane * 16u;
    const float *wnext[MF];              // wave-uniform: the chunk whose weights are requested next (scalar base + lane offset: no per-load address VALU)
#pragma unroll
    for (int mf = 0; mf < MF; mf++) wnext[mf] = wrow[mf] + (long long)(kh + DA * KS) * 256;
    f32x4 a_st[DA][MF];
#pragma unroll
    for (int s = 0; s < DA; s++) {
        const int cc = kh + (s < nloc ? s : nloc - 1) * KS;
#pragma unroll
        for (int mf = 0; mf < MF; mf++) a_st[s][mf] = *reinterpret_cast<const f32x4 *>(wrow[mf] + cc * 256 + lane * 4);
    }
    f32x4 acc[MF][NF];
#pragma unroll
    for (int mf = 0; mf < MF; mf++)
#pragma unroll
        for (int nf = 0; nf < NF; nf++) acc[mf][nf] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float pre_slope = p.pre_slope;
    RVC_KP(11);
    __syncthreads();                                   // (carries the vmcnt(0) of the LDS-DMA pieces)
    // 3. one pass over the tile: fused input LeakyReLU (slope 1 = none) and the turn to channel-contiguous columns, so that a lane's four
    //    k-values of an MFMA B operand are ONE ds_read_b128 (read: lanes along the channels, odd row stride; write: consecutive floats)
    {
        const int total = cin * rl;
        const float inv_cin = 1.0f / (float)cin;
        for (int e = threadIdx.x; e < total; e += NT) {
            const int col = (int)(((float)e + 0.5f) * inv_cin), ci = e - col * cin;
            const float v = tmp[ci * rt + col];
            fin[col * cs + ci] = fmaxf(v, v * pre_slope);
        }
    }
    __syncthreads();
    RVC_KP(2);
    // 4. main loop over the chunks (tap-major): the B fragment of (tap t, channel group g), column n is fin[(n + t * dil) * cs + g * 16 + 4 kq .. + 3]
    const float *bl = fin + (wn * NF * 16 + li) * cs + kq * 4;
    const int last = nloc - 1;
    // (tap, group) of a chunk index, carried incrementally: requests run 1 (B) and DA (weights) of this wave's chunks ahead of the MFMAs
    int g_b = 0, off_b = 0;                             // chunk whose B fragments are requested next (floats from bl)
    const int wrap_b = dil * cs - 16 * G;               // from the last channel group of a tap to the first of the next
#define RVC_CT_ADV1() { g_b++; off_b += 16; if (g_b == G) { g_b = 0; off_b += wrap_b; } }
#define RVC_CT_ADV() { g_b += KS; off_b += 16 * KS; if (g_b >= G) { g_b -= G; off_b += wrap_b; } }      /* (KS <= G: checked at plan time) */
    if (kh) RVC_CT_ADV1()
    f32x4 bcur[NF];
#pragma unroll
    for (int nf = 0; nf < NF; nf++) bcur[nf] = *reinterpret_cast<const f32x4 *>(bl + off_b + nf * 16 * cs);
    RVC_CT_ADV()
    constexpr int T_ = MF * NF * 4;
#define RVC_CT_STEP(S, CC)                                                                              \
    {                                                                                                  \
        const int cc_ = (CC);                                                                          \
        const int ob_ = cc_ < last ? off_b : 0;                 /* the surplus request of the last chunk stays inside the tile */ \
        f32x4 bnx_[NF];                                                                                \
        _Pragma("unroll") for (int t = 0; t < T_; t++) {                                               \
            const int j = t / (NF * MF), nf = (t / MF) % NF, mf = t % MF;                              \
            if (!(RVC_CT_DBG & 8)) acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_st[S][mf][j], bcur[nf][j], acc[mf][nf], 0, 0, 0); \
            else acc[mf][nf][0] += a_st[S][mf][j] * bcur[nf][j];                                       \
            /* the next chunk's B fragments are requested between the MFMAs */                         \
            _Pragma("unroll") for (int r = t * NF / T_; r < (t + 1) * NF / T_; r++) {                  \
                if (!(RVC_CT_DBG & 2)) bnx_[r] = *reinterpret_cast<const f32x4 *>(bl + ob_ + r * 16 * cs); else bnx_[r] = bcur[r]; \
            }                                                                                          \
            __builtin_amdgcn_sched_barrier(0);                                                         \
        }                                                                                              \
        /* the weights are reloaded BEHIND their last use (round 5): requested between the MFMAs into the array they were still being read from, the \
           new value lived in a second register set and the loop-carried copies back (v_mov on registers a load had just been issued into) sat at \
           the loop head -- every round of DA chunks began by waiting for all weight loads in flight */ \
        if (!(RVC_CT_DBG & 1)) {                                                                       \
            _Pragma("unroll") for (int mf = 0; mf < MF; mf++) a_st[S][mf] = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const char *>(wnext[mf]) + lane16); \
        }                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        RVC_CT_ADV()                                                                                   \
        _Pragma("unroll") for (int mf = 0; mf < MF; mf++) wnext[mf] += KS * 256;      /* (requests past the wave's last chunk read the slack behind the panel) */ \
        _Pragma("unroll") for (int nf = 0; nf < NF; nf++) bcur[nf] = bnx_[nf];                         \
    }
    int c = 0;
    for (; c + DA <= nloc; c += DA) {
#pragma unroll
        for (int s = 0; s < DA; s++) RVC_CT_STEP(s, c + s)
    }
#pragma unroll
    for (int s = 0; s < DA; s++)
        if (c + s < nloc) RVC_CT_STEP(s, c + s)
#undef RVC_CT_STEP
#undef RVC_CT_ADV
#undef RVC_CT_ADV1
    RVC_KP(3);
    if (KS == 2) {
        // the odd-chunk waves hand their partial sums over through LDS (the arrival buffer is free since the turn pass)
        f32x4 *red = reinterpret_cast<f32x4 *>(tmp) + (w4 * MF * NF) * 64 + lane;
        if (kh) {
#pragma unroll
            for (int mf = 0; mf < MF; mf++)
#pragma unroll
                for (int nf = 0; nf < NF; nf++) red[(mf * NF + nf) * 64] = acc[mf][nf];
        }
        __syncthreads();
        if (kh) return;
#pragma unroll
        for (int mf = 0; mf < MF; mf++)
#pragma unroll
            for (int nf = 0; nf < NF; nf++) { const f32x4 o = red[(mf * NF + nf) * 64]; acc[mf][nf][0] += o[0]; acc[mf][nf][1] += o[1]; acc[mf][nf][2] += o[2]; acc[mf][nf][3] += o[3]; }
    }
    // 5. epilogue (the arithmetic of every kernel of the family: epi2_value)
    const float *resb = p.res ? p.res + (long long)b * p.res_bs : nullptr;
    float *yb = p.y + (long long)b * p.y_bs + ph.y_off;
    const int act_sel = ph.act_p1 ? ph.act_p1 - 1 : p.act;
    ColOut cols[NF];
#pragma unroll
    for (int nf = 0; nf < NF; nf++) cols[nf] = col_locate(p, ph, tn * BN + (wn * NF + nf) * 16 + li);
    RVC_ACT_DISPATCH_SEL(act_sel, conv_tile_store<A_ COMMA_ MF COMMA_ NF>(p, ph, resb, yb, cols, ((tm * WM + wm) * MF) * 16 + kq * 4, acc);)
    RVC_KP(6);
}
#undef COMMA_

// ------------------------------------------------------------------------------------------------------------------------
// conv_tile32_kernel -- the 32x32x2 body (header comment).  Weight layout: c32s_panel's [m_tile16][chunk][lane16x4][4], chunk = (block * KW + tap) * 2 + group.
// A wave walks ITS chunks i = 0 .. nloc - 1 (global chunk i * KS + kh: with two K shares the share is the channel group) with the weights of DA chunks in
// flight in a register ring and the next chunk's B operand requested between the MFMAs of the current one.
template <int WM, int WN, int KS>
__global__ __launch_bounds__(256) void conv_tile32_kernel(IgemmP p)
{
    static_assert(WM * WN * KS == 4 && (KS == 1 || KS == 2), "four waves: WM x WN accumulators, one or two K shares");
    constexpr int WPS = WM * WN;                    // waves per K share
    constexpr int BN = WN * 32;
    constexpr int CB = 32, CS = CB + 4;             // channels staged per block, LDS column stride in floats (conv32s_kernel's)
    constexpr int DA = 4;                           // weight chunks in flight per wave (DA * KS <= the 16 chunks of slack behind a panel)
    constexpr int NCP = BN + 64, NI = (CB / 4) * NCP / 256;      // staging item grid [CB / 4 channel quads][NCP columns], NI items per thread
    static_assert((CB / 4) * NCP % 256 == 0, "item grid must divide over the workgroup");
    extern __shared__ __attribute__((aligned(16))) float s_x32[];      // 2 x [BN + (KW - 1) * dil][CS]
    const int item = p.items[2 * blockIdx.x];
    if (item < 0) return;
    const int phase = item & 0xff, tm = (item >> 8) & 0xff, tn = item >> 16;
    const int b = p.items[2 * blockIdx.x + 1];
    const PhaseD ph = p.nphase == 1 ? p.ph0 : p.ph[phase];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int kh = wave / WPS, w4 = wave % WPS;     // K share, wave inside the share
    const int wm = w4 / WN, wn = w4 % WN;
    const int c32 = lane & 31, ks = lane >> 5;
    // (the phase descriptor comes through a select: its fields are forced scalar so that the loops below are scalar loops -- conv32s_buf_kernel)
    const int nchunks = __builtin_amdgcn_readfirstlane(ph.nchunks);
    const int t_tab = __builtin_amdgcn_readfirstlane(ph.t_tab);
    const int kw = t_tab & 0xff, dil = t_tab >> 8;
    const int nblk = __builtin_amdgcn_readfirstlane(ph.t_cin) / CB;
    const int ncol = BN + (kw - 1) * dil;
    const int bufsz = ncol * CS;                    // floats per staging buffer
    const int nq = kw * 2 / KS;                     // this wave's chunks per block
    const int nloc = nblk * nq;
    // weights: the lane's float4 of chunk c, half u (k-slot ks: channels (2u + ks) * 4 .. + 3 of the chunk) = wl[c * 256 + u * 128 ..]
    const int mtiles = (p.M + 15) >> 4;
    int t16 = (tm * WM + wm) * 2 + (c32 >> 4);
    t16 = t16 < mtiles ? t16 : mtiles - 1;
    const float *wl = p.w + ph.w_off + (long long)t16 * nchunks * 256 + (ks * 16 + (c32 & 15)) * 4 + kh * 256;
    f32x4 a_st[DA][2];
#pragma unroll
    for (int s = 0; s < DA; s++)
#pragma unroll
        for (int u = 0; u < 2; u++) a_st[s][u] = *reinterpret_cast<const f32x4 *>(wl + s * KS * 256 + u * 128);      // (past the wave's last chunk: the slack behind the panel)
    const float *wnext = wl + DA * KS * 256;
    // staging items of this thread: channel quad qd, staged column s_ (conv32s_kernel's request / commit with a per-thread item map: NCP is no multiple of 64 here)
    const float pre_slope = p.pre_slope;
    const float *xb = p.x + (long long)b * p.x_bs + ph.x_off;
    const int n0 = tn * BN + ph.t_dmin;
    int xo[NI], lo[NI];
#pragma unroll
    for (int r = 0; r < NI; r++) {
        const int e = r * 256 + (int)threadIdx.x;
        const int qd = e / NCP, s_ = e - qd * NCP;
        int gc = n0 + (s_ < ncol ? s_ : ncol - 1);       // (columns past the tile's reach re-read its last one and are not stored)
        gc = gc < p.x_lo ? p.x_lo : (gc > p.x_lim ? p.x_lim : gc);
        xo[r] = qd * 4 * p.x_ld + gc;
        lo[r] = s_ < ncol ? s_ * CS + qd * 4 : -1;
    }
    f32x4 pf[NI];
    auto request = [&](const int blk) {
        const float *xk = xb + (long long)blk * CB * p.x_ld;
#pragma unroll
        for (int r = 0; r < NI; r++)
#pragma unroll
            for (int jj = 0; jj < 4; jj++) pf[r][jj] = xk[xo[r] + jj * p.x_ld];
    };
    auto commit = [&](float *dst) {
#pragma unroll
        for (int r = 0; r < NI; r++) {
            f32x4 v;
#pragma unroll
            for (int jj = 0; jj < 4; jj++) v[jj] = fmaxf(pf[r][jj], pf[r][jj] * pre_slope);
            if (lo[r] >= 0) *reinterpret_cast<f32x4 *>(dst + lo[r]) = v;
        }
    };
    request(0);
    f32x16 acc[1][1];
#pragma unroll
    for (int r = 0; r < 16; r++) acc[0][0][r] = 0.f;
    const float *bl = s_x32 + (wn * 32 + c32) * CS + ks * 4 + (KS == 2 ? kh * 16 : 0);      // B operand base of this lane
    const int tap_step = dil * CS;
    int q = 0, blk = 0;                              // chunk inside the block, block
    const float *bq = bl;                            // B operand of the current chunk
    f32x4 bcur[2], bnx[2];
    bnx[0] = bnx[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // One chunk: (first of a block: write the staged rows -- requested a block earlier -- into the buffer the block before last was read from, barrier,
    // request the next block's rows), eight MFMAs with the next chunk's B operand requested behind the first, then the ring slot's reload.
#define RVC_CT32_STEP(S)                                                                               \
    {                                                                                                  \
        if (q == 0) {                                                                                  \
            float *dst_ = s_x32 + (blk & 1) * bufsz;                                                   \
            commit(dst_);                                                                              \
            __syncthreads();                                                                           \
            if (blk + 1 < nblk) request(blk + 1);                                                      \
            bq = bl + (blk & 1) * bufsz;                                                               \
            bcur[0] = *reinterpret_cast<const f32x4 *>(bq);                                            \
            bcur[1] = *reinterpret_cast<const f32x4 *>(bq + 8);                                        \
        }                                                                                              \
        const float *bqn_ = bq + (KS == 2 ? tap_step : ((q & 1) ? tap_step - 16 : 16));                \
        const bool more_ = q + 1 < nq;                                                                 \
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_st[S][0][0], bcur[0][0], acc[0][0], 0, 0, 0); \
        if (more_) {                                                                                   \
            bnx[0] = *reinterpret_cast<const f32x4 *>(bqn_);                                           \
            bnx[1] = *reinterpret_cast<const f32x4 *>(bqn_ + 8);                                       \
        }                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        _Pragma("unroll") for (int j = 1; j < 4; j++)                                                  \
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_st[S][0][j], bcur[0][j], acc[0][0], 0, 0, 0); \
        _Pragma("unroll") for (int j = 0; j < 4; j++)                                                  \
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_st[S][1][j], bcur[1][j], acc[0][0], 0, 0, 0); \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        /* the weights are reloaded BEHIND their last use (conv_tile_kernel, round 5) */               \
        a_st[S][0] = *reinterpret_cast<const f32x4 *>(wnext);                                          \
        a_st[S][1] = *reinterpret_cast<const f32x4 *>(wnext + 128);                                    \
        wnext += KS * 256;                                                                             \
        bq = bqn_; bcur[0] = bnx[0]; bcur[1] = bnx[1];                                                 \
        if (++q == nq) { q = 0; blk++; }                                                               \
    }
    int c = 0;
    for (; c + DA <= nloc; c += DA) {
#pragma unroll
        for (int s = 0; s < DA; s++) RVC_CT32_STEP(s)
    }
#pragma unroll
    for (int s = 0; s < DA; s++)
        if (c + s < nloc) RVC_CT32_STEP(s)
#undef RVC_CT32_STEP
    if (KS == 2) {
        // the odd-group waves hand their partial sums over through LDS, summed in one fixed order
        __syncthreads();                               // every wave has left the last block's tile
        f32x4 *red = reinterpret_cast<f32x4 *>(s_x32) + w4 * 4 * 64 + lane;
        if (kh) {
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) red[r4 * 64] = (f32x4){acc[0][0][r4 * 4], acc[0][0][r4 * 4 + 1], acc[0][0][r4 * 4 + 2], acc[0][0][r4 * 4 + 3]};
        }
        __syncthreads();
        if (kh) return;
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++) {
            const f32x4 o = red[r4 * 64];
#pragma unroll
            for (int j = 0; j < 4; j++) acc[0][0][r4 * 4 + j] += o[j];
        }
    }
    // epilogue: conv32s's body on this family's terms (per-phase output tensor and activation)
    ColOut cols[1];
    cols[0] = col_locate(p, ph, tn * BN + wn * 32 + c32);
    const int row_t = (tm * WM + wm) * 32;
    c32s_epilogue_at<1, 1>(p, ph, acc, cols, row_t + ks * 4, row_t + 32 <= p.M, p.res ? p.res + (long long)b * p.res_bs : nullptr, p.y + (long long)b * p.y_bs + ph.y_off,
                           ph.act_p1 ? ph.act_p1 - 1 : p.act);
}

}  // namespace rvc
