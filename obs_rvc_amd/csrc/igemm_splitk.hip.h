// igemm_splitk.hip.h -- igemm_splitk_kernel, the first stage of the two-stage grid-level split-K (instantiated by igemm_tiled_inst.hip, launched by
// launch_igemm_splitk).  A layer whose offset table does not fit in LDS (K > 15360: CREPE's 64-tap layers behind 1024 and 256 channels) is cut along K over
// the grid; every workgroup writes the partial sums of its K slice and splitk_epilogue_kernel (plan_ops.hip.h) adds the slices in order and finishes the
// layer.  This is what is left of the first-generation igemm_kernel<MF, NF, D, KS, PRE>: its <1, 1, 12, 1, PRE> instantiations, cut to what they execute here.
#pragma once
#include "igemm_common.hip.h"

namespace rvc {

// One wave owns one 16 x 16 output tile of 16x16x4 fp32 MFMA fragments; the 4 waves of a workgroup work on 4 consecutive tiles (they share weight rows
// through L1).  The workgroup's slice of the koff table is staged in LDS once; weights and gathered activations are register-prefetched 12 chunks (of
// 16 k) ahead; the koff entries of the next chunk are read from LDS one stage early so the LDS latency is off the critical path.
// Grid: x = tiles / 4, y = (batch * nphase + phase) * ksplit + K slice.  LDS: chunks_per_split * 16 ints.
template <bool PRE>
__global__ __launch_bounds__(256) void igemm_splitk_kernel(IgemmP p)
{
    constexpr int D = 12;
    RVC_KP(0);
    extern __shared__ __attribute__((aligned(16))) int s_koff[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = (int)blockIdx.x * 4 + wave;
    int z = blockIdx.y;
    const int ks = z % p.ksplit; z /= p.ksplit;
    const int phase = z % p.nphase;
    const int b = z / p.nphase;
    const PhaseD ph = p.nphase == 1 ? p.ph0 : p.ph[phase];
    const int nchunks = ph.nchunks;
    const int g0 = ks * p.chunks_per_split;
    int g1 = g0 + p.chunks_per_split;
    g1 = g1 < nchunks ? g1 : nchunks;
    const int nc = g1 - g0;                 // chunks of this workgroup (grid-level split)
    {
        const int4 *src = reinterpret_cast<const int4 *>(p.koff + ph.koff_off + g0 * 16);
        int4 *dst = reinterpret_cast<int4 *>(s_koff);
        for (int i = threadIdx.x; i < nc * 4; i += 256) dst[i] = src[i];
    }
    RVC_KP(8);
    int tn, tm;
    if (p.m_fast) { tm = tile % p.m_fast; tn = tile / p.m_fast; }
    else { tn = tile % p.ntn; tm = tile / p.ntn; }
    const bool live = tm < p.ntm && tn < p.ntn;   // padding of the XCD-aware order / grid tail
    const int li = lane & 15, kq = lane >> 4;
    RVC_KP(9);
    // (the barrier that publishes the koff slice comes after the weight loads of the first D stages have been issued:
    //  they do not depend on it, so their latency overlaps the table's round trip)

    // gathered-activation addressing: wave-uniform base (SGPR pair) + unsigned 32-bit BYTE offset per lane, so each load
    // costs one v_add_u32 (table entries are byte offsets biased by koff_bias to be non-negative)
    const char *xb = reinterpret_cast<const char *>(p.x + (long long)b * p.x_bs + ph.x_off) - p.koff_bias;
    unsigned xo;
    {
        int n = tn * 16 + li;
        n = n < p.N ? n : p.N - 1;
        int nh = 0, nw = n;
        if (p.x_hs) { nh = n / p.NW; nw = n - nh * p.NW; }
        xo = (unsigned)(nh * p.x_hs + nw * p.x_ws) * 4u;
    }
    // weights are pre-packed in MFMA-fragment order [m_tile][chunk][lane][4]: one wave-wide dwordx4 load of a
    // (16 rows x 16 k) fragment is 1 KiB fully contiguous (lane l holds W[mt*16 + (l&15)][c*16 + (l>>4)*4 + 0..3])
    const int mtiles = (p.M + 15) >> 4;
    const int mt = tm < mtiles ? tm : mtiles - 1;
    const float *wrow = p.w + ph.w_off + ((long long)mt * nchunks + g0) * 256 + lane * 4;
    const int4 *kol = reinterpret_cast<const int4 *>(s_koff) + kq;
    const float pre_slope = p.pre_slope;

    // a lone fragment alternates two accumulators (MFMA dependency)
    f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};

    RVC_KP(10);
    f32x4 a_st[D];
    float b_st[D][4];
#define RVC_LOAD_A(S, C) { a_st[S] = *reinterpret_cast<const f32x4 *>(wrow + (C) * 256); }
#define RVC_LOAD_B(S, C)                                                                               \
    {                                                                                                  \
        const int cc_ = (C);                                                                           \
        const int4 ko_ = ko_nx;                                                                        \
        ko_nx = kol[(cc_ + 1 < nc ? cc_ + 1 : cc_) * 4];                                               \
        b_st[S][0] = *reinterpret_cast<const float *>(xb + (xo + (unsigned)ko_.x));                    \
        b_st[S][1] = *reinterpret_cast<const float *>(xb + (xo + (unsigned)ko_.y));                    \
        b_st[S][2] = *reinterpret_cast<const float *>(xb + (xo + (unsigned)ko_.z));                    \
        b_st[S][3] = *reinterpret_cast<const float *>(xb + (xo + (unsigned)ko_.w));                    \
    }
#define RVC_COMPUTE_STAGE(S)                                                                          \
    {                                                                                                  \
        _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                \
            /* fused input LeakyReLU, branch-free so the loads stay in flight (PRE layers only) */     \
            const float bv_ = PRE ? fmaxf(b_st[S][j], b_st[S][j] * pre_slope) : b_st[S][j];            \
            acc[j % 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_st[S][j], bv_, acc[j % 2], 0, 0, 0);   \
        }                                                                                              \
    }
#define RVC_LOAD_STAGE(S, C) { RVC_LOAD_A(S, C) RVC_LOAD_B(S, C) }
    if (live) {
#pragma unroll
        for (int s = 0; s < D; s++)
            if (s < nc) RVC_LOAD_A(s, s)
    }
    RVC_KP(11);
    lds_only_barrier();        // not __syncthreads(): its vmcnt(0) would drain the weight loads just issued
    RVC_KP(1);
    if (!live) return;
    int4 ko_nx = nc > 0 ? kol[0] : make_int4(0, 0, 0, 0);
#pragma unroll
    for (int s = 0; s < D; s++)
        if (s < nc) RVC_LOAD_B(s, s)
    RVC_KP(2);
    int c = 0;
    for (; c + 2 * D <= nc; c += D) {
#pragma unroll
        for (int s = 0; s < D; s++) {
            RVC_COMPUTE_STAGE(s)
            __builtin_amdgcn_sched_barrier(0);
            RVC_LOAD_STAGE(s, c + s + D)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    for (; c < nc; c += D) {
#pragma unroll
        for (int s = 0; s < D; s++) {
            if (c + s < nc) {
                RVC_COMPUTE_STAGE(s)
                if (c + s + D < nc) RVC_LOAD_STAGE(s, c + s + D)
            }
        }
    }
#undef RVC_COMPUTE_STAGE
#undef RVC_LOAD_STAGE
#undef RVC_LOAD_A
#undef RVC_LOAD_B
    acc[0] += acc[1];
    RVC_KP(3);

    // partial sums: part[((b*nphase + phase)*ksplit + ks)][M][N]  (D layout of v_mfma_f32_16x16x4_f32: col = lane & 15, row = (lane >> 4) * 4 + reg)
    float *pp = p.part + ((long long)(b * p.nphase + phase) * p.ksplit + ks) * (long long)p.M * p.N;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int m = tm * 16 + kq * 4 + r, n = tn * 16 + li;
        if (m < p.M && n < p.N) pp[(long long)m * p.N + n] = acc[0][r];
    }
}

}  // namespace rvc
