// igemm_common.hip.h -- what the implicit-GEMM kernel family shares, and what the non-GEMM kernels borrow from it: the parameter block (IgemmP / PhaseD),
// the activations, the epilogues and the tile-order helpers.  No kernel lives here: each has a header of its own (igemm2 / igemm2w / igemm_lds / igemm32 /
// igemm_bf3 / igemm_splitk .hip.h), included only by the unit that instantiates it, so that an edit to one kernel rebuilds that kernel's units alone.
// Part of the hand-written gfx950 (CDNA4) kernels for the RVC per-chunk hot path.
//
// Layout convention: every activation is channel-major [B][C][ld] with the time (or H*W)
// axis contiguous and a zero halo on both sides of every row, so convolution taps never
// need bounds checks (the halo is zeroed once at allocation and never written).
//
// The dense work (every Conv1d / ConvTranspose1d / Conv2d / ConvTranspose2d / Linear of
// ContentVec, RMVPE and the NSF-HiFiGAN synthesizer) runs through ONE implicit-GEMM
// kernel on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, exact f32, 157 TF peak):
//   D[m][n] = sum_k W[m][k] * X[koff[k] + noff(n)]
// where koff[] is a per-layer table of input offsets (channel stride, tap, dilation) and
// noff(n) is the per-lane offset of output position n.  Transposed convolutions are run
// as `stride` polyphase sub-convolutions ("phases"), grouped convolutions as one phase
// per group.  64-wide wavefronts: one wave owns a (16*MF) x (16*NF) output tile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rvc {

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_LRELU = 2, ACT_GELU = 3, ACT_TANH = 4, ACT_SIGMOID = 5 };

// GELU(erf) in ONE place (every kernel's epilogue and the fused ContentVec stem round the same way).
#ifdef RVC_FAST_GELU
// (round-6 experiment, never the default: erf as the 13 / 9-term rational polynomial of Eigen / XLA -- 15 vector instructions against libm's ~34 with both of its
//  branches taken inside a wave -- at 4e-7 absolute error instead of 3e-8)
__device__ __forceinline__ float erf_dev(float x)
{
    x = fminf(fmaxf(x, -4.f), 4.f);
    const float x2 = x * x;
    float p = -2.72614225801306e-10f;
    p = fmaf(p, x2, 2.77068142495902e-08f); p = fmaf(p, x2, -2.10102402082508e-06f); p = fmaf(p, x2, -5.69250639462346e-05f);
    p = fmaf(p, x2, -7.34990630326855e-04f); p = fmaf(p, x2, -2.95459980854025e-03f); p = fmaf(p, x2, -1.60960333262415e-02f);
    float q = -1.45660718464996e-05f;
    q = fmaf(q, x2, -2.13374055278905e-04f); q = fmaf(q, x2, -1.68282697438203e-03f); q = fmaf(q, x2, -7.37332916720468e-03f); q = fmaf(q, x2, -1.42647390514189e-02f);
    return x * p * __builtin_amdgcn_rcpf(q);
}
#else
__device__ __forceinline__ float erf_dev(float x) { return erff(x); }
#endif
__device__ __forceinline__ float gelu_dev(float v) { return 0.5f * v * (1.0f + erf_dev(v * 0.70710678118654752440f)); }

__device__ __forceinline__ float apply_act(float v, int act, float slope)
{
    switch (act) {
    case ACT_RELU: return v > 0.f ? v : 0.f;
    case ACT_LRELU: return v > 0.f ? v : v * slope;
    case ACT_GELU: return gelu_dev(v);
    case ACT_TANH: return tanhf(v);
    case ACT_SIGMOID: return 1.0f / (1.0f + expf(-v));
    default: return v;
    }
}

struct PhaseD {
    long long w_off;   // element offset of this phase's [M][Kp] weight panel
    int x_off;         // element offset added to the input base
    int y_c0;          // first output channel of this phase (grouped convs)
    int y_h0;          // output row of nh = 0 (polyphase 2-D transposed convs)
    int y_pos;         // output column of nw = 0 (polyphase transposed convs); checked against [0, OW)
    int bias_off;      // offset into bias
    int koff_off;      // offset into the koff table
    int nchunks;       // K/16 of this phase (fused launches of convs with different kernel sizes; filled by queue_igemm)
    // igemm2 only (register-direct kernel, launches that fuse two DIFFERENT convolutions of one input: RMVPE's 3x3 + shortcut):
    int act_p1;        // this phase's epilogue activation + 1 (0: the launch's IgemmP::act)
    int pad_;
    long long y_off;   // element offset of this phase's output tensor from IgemmP::y
    // conv_tile_kernel only (conv_tile.hip.h): the staged input tile of this phase
    int t_tab;         // offset of the phase's LDS-offset table in IgemmP::ttab (ints; padded to whole 256-int pieces)
    int t_cin;         // input rows staged
    int t_rs;          // LDS row stride (floats) = BN + reach of the taps, padded
    int t_dmin;        // column of the leftmost tap relative to the output column (<= 0)
};

struct IgemmP {
    const float *x, *w, *bias, *res;
    float *y, *part;
    const int *koff;
    const PhaseD *ph;
    PhaseD ph0;              // copy of ph[0]: single-phase layers skip the dependent table load
    int M, N, K;             // K already padded to a multiple of 16
    int NW;                  // n -> (nh, nw) = (n / NW, n % NW)
    int x_hs, x_ws;          // input offset of position n  = nh*x_hs + nw*x_ws
    int y_hm, y_ws;          // output coordinates of position n: row = nh*y_hm + y_h0, col = nw*y_ws + y_pos
    int OW;                  // valid iff 0 <= col < OW
    long long x_bs, y_bs, res_bs;
    int y_cs, res_cs;        // channel strides of the output / residual tensors
    int y_rs, res_rs;        // row strides (0 for 1-D tensors)
    int nphase, ksplit, chunks_per_split;
    int act; float slope; float scale; int accumulate;
    int pre_act; float pre_slope;   // fused input LeakyReLU: x -> max(x, x*pre_slope); pre_slope = 1 disables it
    int ntn, ntm;
    int koff_bias;           // bytes: the koff table holds (offset - min offset) * 4, the base pointer is moved back by this
    int glu;                 // WaveNet gate fused into the epilogue: rows are GLU-packed (see glu_store), output has M/2 channels
    int res_nogroup;         // residual channel = m (a tensor shared by all phases) instead of m + y_c0
    unsigned long long *probe;   // tuning build only (-DRVC_KPROBE): per-wave phase timestamps
    int m_fast;              // XCD-aware tile order: >0 = ntm rounded up to 8, m fastest (workgroup b runs on XCD b%8, so all
                             // n-tiles of one weight-row block share one XCD's L2); 0 = n fastest (activation-heavy layers)
    int nbatch;              // igemm2: streams in the launch (grid z = batch * nphase + phase)
    int fold_n;              // > 0: the streams of the launch are folded into the N axis: position n = stream (n / fold_n), local position
                             // (n % fold_n); N = streams * fold_n and the launch has one batch (tiles may straddle streams, nothing is padded per stream)
    int bf3;                 // exploratory (igemm_bf3_kernel): w points at the split-bf16 panels of this layer, the products run as three bf16 MFMAs
    int lin_cs4;             // igemm2 LIN layers (1x1 conv on a 1-D tensor): input channel stride in BYTES, k-th operand row = k * lin_cs4
    // LayerNorm folded into its neighbours (one stream, ContentVec's post-LN layers):
    //  * consumer of a not-yet-normalised tensor y (igemm2 LNB instantiations): the weights carry the LayerNorm scale, the bias its
    //    shift; the kernel sums y and y^2 per column from the operand stream it reads anyway and finishes
    //    out = rstd[n] * (acc - mean[n] * ln_wsum[m]) + bias[m];  the tm == 0 workgroups also publish (mean, rstd) per column
    //  * a later layer whose RESIDUAL is LayerNorm(y): res = (y - mean[n]) * rstd[n] * ln_g[row] + ln_bt[row], from the published stats
    const float *ln_wsum;    // [M] sum_k W'[m][k]
    float *ln_stats_out;     // [N][2]
    const float *ln_stats_in, *ln_g, *ln_bt;
    float ln_eps, ln_inv_rows;
    // conv_tile_kernel (conv_tile.hip.h): work-item table (phase | m-tile << 8 | n-tile << 16, or -1) indexed by blockIdx.x, LDS-offset
    // tables, and the input row geometry (row stride, first / last readable column of a row: the halo)
    const int *items, *ttab;
    int x_ld, x_lo, x_lim, pad2_;
};

__device__ __forceinline__ void epilogue_store(const IgemmP &p, const PhaseD &ph, int b, int m, int n, float acc)
{
    if (m >= p.M || n >= p.N) return;
    if (p.fold_n) { b = n / p.fold_n; n -= b * p.fold_n; }
    int nh = 0, nw = n;
    if (p.y_hm) { nh = n / p.NW; nw = n - nh * p.NW; }
    const int ow = nw * p.y_ws + ph.y_pos, oh = nh * p.y_hm + ph.y_h0;
    if (ow < 0 || ow >= p.OW) return;
    const int ch = m + ph.y_c0;
    float v = acc;
    if (p.bias) v += p.bias[ph.bias_off + m];
    v = apply_act(v, p.act, p.slope);
    if (p.res) v += p.res[(long long)b * p.res_bs + (long long)(p.res_nogroup ? m : ch) * p.res_cs + (long long)oh * p.res_rs + ow];
    v *= p.scale;
    float *yp = p.y + (long long)b * p.y_bs + (long long)ch * p.y_cs + (long long)oh * p.y_rs + ow;
    if (p.accumulate) v += *yp;
    *yp = v;
}

// Fused WaveNet gate: the weight rows of the in-layer are packed so that every 16-row MFMA fragment holds 8 output channels --
// fragment row kq*4 + r is the tanh row of channel f*8 + kq*2 + (r&1) for r < 2 and the sigmoid row of the same channel for
// r >= 2 -- so one lane owns both halves of a channel in its accumulator registers (r, r + 2).
__device__ __forceinline__ void glu_store(const IgemmP &p, const PhaseD &ph, int b, int m1, int n, float a1, float a2)
{
    if (m1 >= p.M || n >= p.N) return;
    if (p.fold_n) { b = n / p.fold_n; n -= b * p.fold_n; }
    const float ta = a1 + p.bias[ph.bias_off + m1], sa = a2 + p.bias[ph.bias_off + m1 + 2];
    const int ch = (m1 >> 4) * 8 + ((m1 & 15) >> 2) * 2 + (m1 & 1) + ph.y_c0;
    p.y[(long long)b * p.y_bs + (long long)ch * p.y_cs + n] = tanhf(ta) * (1.0f / (1.0f + expf(-sa)));
}


// Workgroup barrier that only orders LDS traffic: waits for this wave's LDS operations (lgkmcnt(0)) and joins the barrier, leaving
// global loads in flight (gfx9 s_waitcnt encoding: vmcnt = 63, expcnt = 7, lgkmcnt = 0).
__device__ __forceinline__ void lds_only_barrier()
{
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
}

#ifdef RVC_KPROBE
#define RVC_KP(i) do { if (p.probe && (threadIdx.x & 63) == 0) p.probe[((size_t)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16 + (i)] = wall_clock64(); } while (0)
#else
#define RVC_KP(i)
#endif

// Workgroups reach the 8 XCDs round-robin in dispatch order (block b of a launch on XCD (b + c) % 8, tests/tools/xcd_probe.hip), and every XCD
// has its own L2.  With m-fastest tile order on the raw block index the m-tiles of one activation tile sat on ntm DIFFERENT XCDs, and every
// one of them fetched the tile again (round 4 PMC pass per kernel: the 768 x 3072 projection at 64 streams read 471 MB per launch for 118 MB
// of operands, the first stride-2 stem convolution 4.4 GB for 0.94).  xcd_tile_id gives the workgroups that one XCD receives CONSECUTIVE tile
// ids: an XCD then owns whole activation tiles (each fetched once), and only the weights -- the small operand when streams are folded into N --
// are fetched once per XCD.  Scalar arithmetic, once per workgroup.  (The tiled kernels take m_fast = 1 for this order and m_fast = 2 for the raw
// block index: when the m-tile count is a multiple of 8 AND the weights exceed an L2 -- ContentVec's 3072 x 768 projection, 24 m-tiles, 9.4 MB --
// the raw order keeps every weight-row block on ONE XCD and streams the small activation tensor through all eight: 218 MB per launch against 319.)
__device__ __forceinline__ int xcd_tile_id(int x, int gx, int row_start)
{
    const int off = row_start & 7, c = (x + off) & 7;
    int base = 0;
#pragma unroll
    for (int cc = 0; cc < 8; cc++) {
        const int f = (cc - off) & 7;
        const int cnt = f < gx ? (gx - f + 7) >> 3 : 0;
        base += cc < c ? cnt : 0;
    }
    return base + ((x - ((c - off) & 7)) >> 3);
}

template <int ACT> __device__ __forceinline__ float act_t(float v, float slope)
{
    if (ACT == ACT_RELU) return v > 0.f ? v : 0.f;
    if (ACT == ACT_LRELU) return v > 0.f ? v : v * slope;
    if (ACT == ACT_GELU) return gelu_dev(v);
    if (ACT == ACT_TANH) return tanhf(v);
    if (ACT == ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
    return v;
}
struct Epi2 { float bias, res, yold; int yo; };
__device__ __forceinline__ Epi2 epi2_prefetch(const IgemmP &p, const PhaseD &ph, const float *resb, const float *yb, int m, int n)
{
    Epi2 e = {0.f, 0.f, 0.f, -1};
    if (m >= p.M || n >= p.N) return e;
    const int n_launch = n;
    int bb = 0;
    if (p.fold_n) { bb = n / p.fold_n; n -= bb * p.fold_n; }
    int nh = 0, nw = n;
    if (p.y_hm) { nh = n / p.NW; nw = n - nh * p.NW; }
    const int ow = nw * p.y_ws + ph.y_pos, oh = nh * p.y_hm + ph.y_h0;
    if (ow < 0 || ow >= p.OW) return e;
    const int ch = m + ph.y_c0;
    e.yo = bb * (int)p.y_bs + ch * p.y_cs + oh * p.y_rs + ow;
    if (p.bias) e.bias = p.bias[ph.bias_off + m];
    if (resb) {
        const int rrow = p.res_nogroup ? m : ch;
        e.res = resb[bb * (int)p.res_bs + rrow * p.res_cs + oh * p.res_rs + ow];
        if (p.ln_stats_in)       // the residual is LayerNorm(stored tensor): normalise on the fly
            e.res = (e.res - p.ln_stats_in[2 * n_launch]) * p.ln_stats_in[2 * n_launch + 1] * p.ln_g[rrow] + p.ln_bt[rrow];
    }
    if (p.accumulate) e.yold = yb[e.yo];
    return e;
}
// the epilogue's arithmetic, in ONE place (every path must round the same way: eager/graph and tile choice are bit-identical)
template <int ACT> __device__ __forceinline__ float epi2_value(float acc, float bias, float res, float yold, float slope, float scale)
{
    float v = act_t<ACT>(acc + bias, slope);
    v += res;
    v *= scale;
    v += yold;
    return v;
}
template <int ACT> __device__ __forceinline__ void epi2_finish(const IgemmP &p, float *yb, float acc, const Epi2 &e)
{
    if (e.yo < 0) return;
    yb[e.yo] = epi2_value<ACT>(acc, e.bias, e.res, e.yold, p.slope, p.scale);
}
// Column part of the output address (everything that depends on n only: stream, row, column, validity), computed once per MFMA
// column instead of once per element -- with folded streams it holds an integer division.
struct ColOut { int yo, ro; };          // yo < 0: column not stored
__device__ __forceinline__ ColOut col_locate(const IgemmP &p, const PhaseD &ph, int n)
{
    ColOut c = {-1, 0};
    if (n >= p.N) return c;
    int bb = 0;
    if (p.fold_n) { bb = n / p.fold_n; n -= bb * p.fold_n; }
    int nh = 0, nw = n;
    if (p.y_hm) { nh = n / p.NW; nw = n - nh * p.NW; }
    const int ow = nw * p.y_ws + ph.y_pos, oh = nh * p.y_hm + ph.y_h0;
    if (ow < 0 || ow >= p.OW) return c;
    c.yo = bb * (int)p.y_bs + oh * p.y_rs + ow;
    c.ro = bb * (int)p.res_bs + oh * p.res_rs + ow;
    return c;
}
__device__ __forceinline__ Epi2 epi2_from_col(const IgemmP &p, const PhaseD &ph, const float *resb, const float *yb, const ColOut &c, int m)
{
    Epi2 e = {0.f, 0.f, 0.f, -1};
    if (m >= p.M || c.yo < 0) return e;
    const int ch = m + ph.y_c0;
    e.yo = c.yo + ch * p.y_cs;
    if (p.bias) e.bias = p.bias[ph.bias_off + m];
    if (resb) e.res = resb[c.ro + (p.res_nogroup ? m : ch) * p.res_cs];
    if (p.accumulate) e.yold = yb[e.yo];
    return e;
}
__device__ __forceinline__ Epi2 epi2_plain(float bias, int yo) { Epi2 e = {bias, 0.f, 0.f, yo}; return e; }
__device__ __forceinline__ Epi2 epi2_none() { Epi2 e = {0.f, 0.f, 0.f, -1}; return e; }
// the same with the bias already in hand (batched epilogues: biases are loaded once per row, before any store)
__device__ __forceinline__ Epi2 epi2_aux(const IgemmP &p, const PhaseD &ph, const float *resb, const float *yb, const ColOut &c, int m, float bias)
{
    Epi2 e = {bias, 0.f, 0.f, -1};
    if (m >= p.M || c.yo < 0) return e;
    const int ch = m + ph.y_c0;
    e.yo = c.yo + ch * p.y_cs;
    if (resb) e.res = resb[c.ro + (p.res_nogroup ? m : ch) * p.res_cs];
    if (p.accumulate) e.yold = yb[e.yo];
    return e;
}
// fused WaveNet gate on a located column (see glu_store)
__device__ __forceinline__ void glu_from_col(const IgemmP &p, const PhaseD &ph, float *yb, const ColOut &c, int m1, float a1, float a2)
{
    if (m1 >= p.M || c.yo < 0) return;
    const float ta = a1 + p.bias[ph.bias_off + m1], sa = a2 + p.bias[ph.bias_off + m1 + 2];
    const int ch = (m1 >> 4) * 8 + ((m1 & 15) >> 2) * 2 + (m1 & 1) + ph.y_c0;
    yb[c.yo + ch * p.y_cs] = tanhf(ta) * (1.0f / (1.0f + expf(-sa)));
}

__device__ __forceinline__ void glu_from_col_b(const IgemmP &p, const PhaseD &ph, float *yb, const ColOut &c, int m1, float a1, float a2, float b1, float b2)
{
    if (m1 >= p.M || c.yo < 0) return;
    const float ta = a1 + b1, sa = a2 + b2;
    const int ch = (m1 >> 4) * 8 + ((m1 & 15) >> 2) * 2 + (m1 & 1) + ph.y_c0;
    yb[c.yo + ch * p.y_cs] = tanhf(ta) * (1.0f / (1.0f + expf(-sa)));
}

#define RVC_ACT_DISPATCH(STMT) RVC_ACT_DISPATCH_SEL(p.act, STMT)
#define RVC_ACT_DISPATCH_SEL(SEL, STMT)                                          \
    switch (SEL) {                                                             \
    case ACT_RELU: { constexpr int A_ = ACT_RELU; STMT } break;                  \
    case ACT_LRELU: { constexpr int A_ = ACT_LRELU; STMT } break;                \
    case ACT_GELU: { constexpr int A_ = ACT_GELU; STMT } break;                  \
    case ACT_TANH: { constexpr int A_ = ACT_TANH; STMT } break;                  \
    case ACT_SIGMOID: { constexpr int A_ = ACT_SIGMOID; STMT } break;            \
    default: { constexpr int A_ = ACT_NONE; STMT } break;                        \
    }

// accumulator of one v_mfma_f32_32x32x2_f32 block (igemm32 / igemm32l / conv32s / conv_tile32: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5))
typedef float f32x16 __attribute__((ext_vector_type(16)));

}  // namespace rvc
