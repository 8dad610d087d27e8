// model_crepe.hip -- the CREPE f0 method as a plan: frames, six convolution layers on the implicit-GEMM planner with the ReLU -> BatchNorm ->
// max-pool launches between them, the classifier, the decoder; then the pitch tail RMVPE uses (build_pitch_post, model_rmvpe.hip), fed as YIN feeds it.
#include "engine_int.h"
#include "crepe.hip.h"

namespace rvc {

static const int kCrepeCh[6] = {32, 4, 4, 4, 8, 16}, kCrepeK[6] = {512, 64, 64, 64, 64, 64};      // output channels per unit of capacity, kernel sizes; stride 4 then 1
static const int kCrepeLen[7] = {1024, 256, 128, 64, 32, 16, 8};                                 // conv output length of layer l = kCrepeLen[l + 1], pooled to half

ModelCR::ModelCR(const Blob &b)
{
    cap = b.icfg("cap");
    if (cap < 1 || cap > 32) throw std::runtime_error("crepe blob: capacity outside [1, 32]");
    int cin = 1;
    for (int l = 0; l < 6; l++) {
        const int co = kCrepeCh[l] * cap, k = kCrepeK[l];
        const BlobTensor &w = b.t(fmt("cr.conv%d.w", l + 1));
        if (w.nelem != (size_t)co * cin * k || b.t(fmt("cr.conv%d.b", l + 1)).nelem != (size_t)co || b.t(fmt("cr.bn%d.scale", l + 1)).nelem != (size_t)co ||
            b.t(fmt("cr.bn%d.shift", l + 1)).nelem != (size_t)co)
            throw std::runtime_error("crepe blob: layer shape does not match its capacity");
        conv[l] = prep_conv(w.data, b.w(fmt("cr.conv%d.b", l + 1)), co, cin, k, 1);
        scale[l] = dv(b, fmt("cr.bn%d.scale", l + 1));
        shift[l] = dv(b, fmt("cr.bn%d.shift", l + 1));
        weight_bytes += (w.nelem + 3 * (size_t)co) * 4;
        cin = co;
    }
    const int feat = 4 * cin;
    if (b.t("cr.fc.w").nelem != (size_t)CREPE_BINS * feat || b.t("cr.fc.b").nelem != (size_t)CREPE_BINS) throw std::runtime_error("crepe blob: classifier shape");
    fc = prep_conv(b.w("cr.fc.w"), b.w("cr.fc.b"), CREPE_BINS, feat, 1, 1);
    weight_bytes += ((size_t)CREPE_BINS * feat + CREPE_BINS) * 4;
    f0tab = upload_f(crepe_f0_table());
}

ModelCR::~ModelCR()
{
    for (int l = 0; l < 6; l++) { free_conv(conv[l]); wfree(scale[l]); wfree(shift[l]); }
    free_conv(fc);
    wfree(f0tab);
}

// Hz of the 360 bins, rounded once from double: the kernel looks a bin up and calls no exp2f
std::vector<float> crepe_f0_table()
{
    std::vector<float> t(CREPE_BINS);
    for (int i = 0; i < CREPE_BINS; i++) t[i] = (float)(10.0 * std::pow(2.0, (20.0 * i + 1997.3794084376191) / 1200.0));
    return t;
}

size_t crepe_backpointer_bytes(int B, int Tm) { return Tm > CREPE_BP_LDS_FRAMES ? (size_t)B * Tm * CREPE_BINS : 0; }

void launch_crepe_decode(hipStream_t s, int B, const float *prob, int Tm, int decoder, const float *f0tab, unsigned char *bp, float *f0, int *bins, float *pd)
{
    if (B < 1 || Tm < 1 || Tm > 1024 || (decoder != 0 && decoder != 1) || (!bp && crepe_backpointer_bytes(B, Tm))) throw ShapeError("crepe decode: shape");
    CrepeDecP dp{};
    dp.prob = prob; dp.Tm = Tm; dp.decoder = decoder; dp.f0tab = f0tab; dp.bp = bp; dp.f0 = f0; dp.bins = bins; dp.pd = pd;
    hipLaunchKernelGGL(crepe_decode_kernel, dim3(B), dim3(CREPE_DEC_THREADS), 0, s, dp);
}

// layers 2-6: 64 taps, stride 1, zero padding (31, 32).  The operand rows carry a halo of 32 zeros on either side (crepe_bn_pool_kernel writes between them), so
// the asymmetry is only where the tap offsets start: -31.  add_conv1d's table with that one change; the planner sees an ordinary stride-1 convolution
// (plan.hip add_conv1d is the original: the row geometry x_ld / x_lo / x_lim, the N / NW / OW and stride fields and fill_epilogue must track it when it changes)
static void add_crepe_conv(Plan &pl, const ConvW &cw, const T1 &x, const T1 &y)
{
    const int KW = cw.KW, padl = (KW - 1) / 2, padr = KW - 1 - padl;
    if (x.halo < padr || y.T != x.T || cw.K != cw.Kp || cw.groups != 1 || x.C != cw.Cin || y.C != cw.M) throw ShapeError("crepe conv: shape");
    IgemmP p{};
    p.x = x.p; p.w = cw.w; p.y = y.p;
    p.M = cw.M; p.N = y.T; p.K = cw.Kp;
    p.NW = y.T; p.x_hs = 0; p.x_ws = 1; p.y_hm = 0; p.y_ws = 1; p.OW = y.T;
    p.x_bs = x.bs; p.y_bs = y.bs; p.y_cs = y.ld; p.y_rs = 0;
    p.x_ld = x.ld; p.x_lo = -x.halo; p.x_lim = x.T - 1 + x.halo;
    fill_epilogue(p, cw, ConvOpts());
    std::vector<int> koff(cw.Kp, 0);
    for (int ci = 0; ci < cw.Cin; ci++) for (int k = 0; k < KW; k++) koff[ci * KW + k] = ci * x.ld + k - padl;
    queue_igemm(pl, p, x.B, koff, std::vector<PhaseD>(1, PhaseD{}));
}

// raw f0 [B][Tm] of the last f0_extractor_frame samples of each stream of pl.d_in ([B][L]), on RMVPE's frame grid: build_yin's contract
float *build_crepe(rvc_engine *e, Plan &pl, int B, size_t L, size_t frame16k, int method, const char *pre)
{
    const ModelCR *mp = method == RVC_F0_CREPE ? e->cr_full.get() : e->cr_tiny.get();
    if (!mp) throw std::logic_error("f0 method");
    const ModelCR &m = *mp;
    const size_t fr = 5120 * ((frame16k + 800 - 1) / 5120 + 1) - 160;     // rmvpe.rs:256
    if (fr > L) throw PanicError("input shorter than f0_extractor_frame");
    const int Tm = (int)(1 + fr / 160);
    if (Tm % 32 != 0) throw PanicError("mel frame count is not a multiple of 32 (rmvpe.rs:229-233 branch)");
    if (Tm > 1024) throw ShapeError("f0 window too long");
    pl.Tm = Tm;
    Arena &A = pl.arena;
    const int F = B * Tm;          // every frame is a batch entry of the convolutions: B * Tm * len columns
    if ((long long)B * Tm > 65535) throw ShapeError("CREPE: more than 65535 frames in one plan (streams x frames of the f0 window)");          // (a batch entry each; include/rvc_mi355x.h states the limit)
    auto view = [&](const T1 &t, int rows, int cols, int ld) { T1 v = t; v.B = B; v.C = rows; v.T = cols; v.ld = ld; v.halo = 0; v.bs = (long long)Tm * t.bs; return v; };

    T1 x = make_t1(A, F, 1, CREPE_FRAME, 256);          // layer 1 reads 254 samples in front of a frame and 253 behind it (output 255: taps 766 .. 1277)
    {
        CrepeFrameP fp{};
        fp.audio = pl.d_in; fp.audio_bs = (long long)L; fp.n = (int)L; fp.frame = (int)fr; fp.Tm = Tm; fp.out = x.p; fp.out_fs = x.bs;
        const dim3 grid(Tm, B);
        Plan *plp = &pl;
        pl.ops.push_back([=](hipStream_t s) { CrepeFrameP f2 = fp; if (plp->cur_in) f2.audio = plp->cur_in; hipLaunchKernelGGL(crepe_frame_kernel, grid, dim3(256), 0, s, f2); });
    }
    add_tap(pl, (std::string(pre) + ".frames").c_str(), view(x, Tm, CREPE_FRAME, x.ld));
    // one scratch tensor takes every layer's conv + bias (the pool behind it has consumed it before the next layer writes)
    const T1 y0 = make_t1(A, F, kCrepeCh[0] * m.cap, kCrepeLen[1], 0);
    const int feat = 4 * kCrepeCh[5] * m.cap;
    const T1 cls = make_t1(A, B, feat, Tm, 0);
    for (int l = 0; l < 6; l++) {
        const int co = kCrepeCh[l] * m.cap, len = kCrepeLen[l + 1];
        T1 y = y0; y.C = co; y.T = len; y.ld = len; y.bs = (long long)co * len;
        if ((size_t)F * y.bs > (size_t)F * y0.bs) throw std::logic_error("crepe scratch");
        if (l == 0) add_conv1d(pl, m.conv[0], x, y, 4, 254, 1);
        else add_crepe_conv(pl, m.conv[l], x, y);
        CrepePoolP pp{};
        pp.y = y.p; pp.y_ld = y.ld; pp.y_bs = y.bs; pp.C = co; pp.L = len / 2; pp.total = (long long)F * co * (len / 2);
        pp.scale = m.scale[l]; pp.shift = m.shift[l]; pp.Tm = Tm;
        T1 tap;
        if (l < 5) {
            x = make_t1(A, F, co, len / 2, 32);
            pp.out = x.p; pp.o_ld = x.ld; pp.o_bs = x.bs; pp.cls = 0;
            tap = view(x, Tm * co, len / 2, x.ld);
        } else {
            pp.out = cls.p; pp.o_ld = cls.ld; pp.o_bs = cls.bs; pp.cls = 1;
            tap = cls;
        }
        const dim3 grid((unsigned)((pp.total + 255) / 256));
        pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(crepe_bn_pool_kernel, grid, dim3(256), 0, s, pp); });
        add_tap(pl, (pre + fmt(".p%d", l + 1)).c_str(), tap);
    }
    const T1 logit = make_t1(A, B, CREPE_BINS, Tm, 0);
    add_conv1d(pl, m.fc, cls, logit, 1, 0, 1);
    float *prob = A.floats((size_t)B * Tm * CREPE_BINS);
    {
        const long long total = (long long)B * Tm * CREPE_BINS;
        const dim3 grid((unsigned)((total + 255) / 256));
        pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(crepe_sigmoid_kernel, grid, dim3(256), 0, s, logit.p, logit.ld, logit.bs, Tm, total, prob); });
    }
    { T1 t; t.p = prob; t.B = B; t.C = Tm; t.T = CREPE_BINS; t.ld = CREPE_BINS; t.bs = (long long)Tm * CREPE_BINS; add_tap(pl, (std::string(pre) + ".prob").c_str(), t); }
    float *f0 = A.floats((size_t)B * Tm);
    {
        const size_t bpn = crepe_backpointer_bytes(B, Tm);
        unsigned char *bp = bpn ? (unsigned char *)A.alloc(bpn) : nullptr;
        const int decoder = pl.key.crepe_decoder; const float *tab = m.f0tab;
        pl.ops.push_back([=](hipStream_t s) { launch_crepe_decode(s, B, prob, Tm, decoder, tab, bp, f0, nullptr, nullptr); });
    }
    { T1 t; t.p = f0; t.B = B; t.C = 1; t.T = Tm; t.ld = Tm; t.bs = Tm; add_tap(pl, (std::string(pre) + ".f0").c_str(), t); }
    return f0;
}

}  // namespace rvc
