// model_fcpe.hip -- the FCPE f0 method as a plan: RMVPE's mel front end on FCPE's Slaney filterbank, the input stack and the
// pointwise convolutions on the implicit-GEMM planner, the kernels of fcpe.hip.h between them, the classifier, the decoder; then the pitch tail RMVPE uses
// (build_pitch_post, model_rmvpe.hip), fed as YIN and CREPE feed it.
#include "engine_int.h"
#include "fcpe.hip.h"

namespace rvc {

static void want(const Blob &b, const std::string &name, size_t n)
{
    if (b.t(name).nelem != n) throw std::runtime_error("fcpe blob: " + name + " does not match the blob's sizes");
}

ModelFC::ModelFC(const Blob &b)
{
    H = b.icfg("hidden"); I = b.icfg("inner"); layers = b.icfg("layers");
    if (H < 16 || H > 1024 || H % 16 != 0 || I < 16 || I > 4096 || I % 16 != 0 || layers < 1 || layers > 32) throw std::runtime_error("fcpe blob: sizes out of range (hidden, inner: multiples of 16)");
    const size_t h = H, in = I;
    want(b, "fc.in0.w", h * FCPE_MELS * 3); want(b, "fc.in0.b", h); want(b, "fc.gn.g", h); want(b, "fc.gn.b", h);
    want(b, "fc.in1.w", h * h * 3); want(b, "fc.in1.b", h);
    want(b, "fc.norm.g", h); want(b, "fc.norm.b", h); want(b, "fc.out.w", FCPE_BINS * h); want(b, "fc.out.b", FCPE_BINS);
    want(b, "fc.mel_basis", (size_t)FCPE_MELS * 513); want(b, "fc.mel_band", (size_t)FCPE_MELS * 2);
    // the band table is what bounds the front end's reads of the basis rows and of the 513 magnitudes: checked before anything is uploaded
    std::vector<int> bd(FCPE_MELS * 2);
    for (int i = 0; i < FCPE_MELS; i++) {
        const float lo = b.w("fc.mel_band")[2 * i], hi = b.w("fc.mel_band")[2 * i + 1];
        if (!(lo >= 0.f && lo <= hi && hi <= 513.f) || lo != floorf(lo) || hi != floorf(hi)) throw std::runtime_error("fcpe blob: mel band table out of range");
        bd[2 * i] = (int)lo; bd[2 * i + 1] = (int)hi;
    }
    in0 = prep_conv(b.w("fc.in0.w"), b.w("fc.in0.b"), H, FCPE_MELS, 3, 1);
    in1 = prep_conv(b.w("fc.in1.w"), b.w("fc.in1.b"), H, H, 3, 1);
    gn_g = dv(b, "fc.gn.g"); gn_b = dv(b, "fc.gn.b");
    ly.resize(layers);
    for (int l = 0; l < layers; l++) {
        Layer &y = ly[l];
        want(b, fmt("fc.l%d.ln.g", l), h); want(b, fmt("fc.l%d.ln.b", l), h);
        want(b, fmt("fc.l%d.pw1.w", l), 2 * in * h); want(b, fmt("fc.l%d.pw1.b", l), 2 * in);
        want(b, fmt("fc.l%d.dw.w", l), in * FCPE_DW_K); want(b, fmt("fc.l%d.dw.b", l), in);
        want(b, fmt("fc.l%d.pw2.w", l), h * in); want(b, fmt("fc.l%d.pw2.b", l), h);
        y.ln_g = dv(b, fmt("fc.l%d.ln.g", l)); y.ln_b = dv(b, fmt("fc.l%d.ln.b", l));
        y.pw1 = prep_conv(b.w(fmt("fc.l%d.pw1.w", l)), b.w(fmt("fc.l%d.pw1.b", l)), 2 * I, H, 1, 1);
        y.dw_w = dv(b, fmt("fc.l%d.dw.w", l)); y.dw_b = dv(b, fmt("fc.l%d.dw.b", l));
        y.pw2 = prep_conv(b.w(fmt("fc.l%d.pw2.w", l)), b.w(fmt("fc.l%d.pw2.b", l)), H, I, 1, 1);
    }
    norm_g = dv(b, "fc.norm.g"); norm_b = dv(b, "fc.norm.b");
    out = prep_conv(b.w("fc.out.w"), b.w("fc.out.b"), FCPE_BINS, H, 1, 1);
    basis = dv(b, "fc.mel_basis");
    HIPCHK(hipMalloc(&band, bd.size() * sizeof(int)));
    HIPCHK(hipMemcpy(band, bd.data(), bd.size() * sizeof(int), hipMemcpyHostToDevice));
    f0tab = upload_f(fcpe_f0_table());
    weight_bytes = b.bytes();
}

ModelFC::~ModelFC()
{
    free_conv(in0); free_conv(in1); free_conv(out);
    for (Layer &y : ly) { free_conv(y.pw1); free_conv(y.pw2); wfree(y.ln_g); wfree(y.ln_b); wfree(y.dw_w); wfree(y.dw_b); }
    for (float *p : {gn_g, gn_b, norm_g, norm_b, basis, f0tab}) if (p) wfree(p);
    if (band) (void)hipFree(band);
}

// the cent table is linspace(1200 log2(32.70 / 10), 1200 log2(1975.5 / 10), 360); Hz of a bin's centre rounded once from double
static const double kFcpeC0 = 1200.0 * std::log2(32.70 / 10.0), kFcpeC1 = 1200.0 * std::log2(1975.5 / 10.0);
float fcpe_cent_step() { return (float)((kFcpeC1 - kFcpeC0) / (FCPE_BINS - 1)); }
std::vector<float> fcpe_f0_table()
{
    std::vector<float> t(FCPE_BINS);
    const double step = (kFcpeC1 - kFcpeC0) / (FCPE_BINS - 1);
    for (int i = 0; i < FCPE_BINS; i++) t[i] = (float)(10.0 * std::pow(2.0, (kFcpeC0 + step * i) / 1200.0));
    return t;
}

void launch_fcpe_decode(hipStream_t s, int B, int Tm, const float *logit, int l_ld, long long l_bs, const float *prob_in, float *prob, const float *f0tab, double threshold, float *f0, int *bins)
{
    if (B < 1 || B > 65535 || Tm < 1 || Tm > 1024 || (!logit && !prob_in) || (logit && !prob) || !(threshold >= 0.0 && threshold < 1.0)) throw ShapeError("fcpe decode: shape");
    FcpeDecP dp{};
    dp.logit = logit; dp.l_ld = l_ld; dp.l_bs = l_bs; dp.prob_in = prob_in; dp.prob = prob; dp.f0tab = f0tab; dp.cent_step = fcpe_cent_step();
    dp.threshold = threshold; dp.Tm = Tm; dp.f0 = f0; dp.bins = bins;
    hipLaunchKernelGGL(fcpe_decode_kernel, dim3((Tm + 3) / 4, B), dim3(256), 0, s, dp);
}

void launch_fcpe_glu_dw(hipStream_t s, int B, int I, int T, const float *z, int z_ld, long long z_bs, const float *w, const float *bias, float *y, int y_ld, long long y_bs)
{
    if (B < 1 || B > 65535 || I < 1 || T < 1 || z_ld < T || y_ld < T || z_bs < 2LL * I * z_ld || y_bs < (long long)I * y_ld || (T + FCPE_DW_TT - 1) / FCPE_DW_TT > 65535)
        throw ShapeError("fcpe depthwise: shape");
    FcpeDwP q{};
    q.z = z; q.z_ld = z_ld; q.z_bs = z_bs; q.y = y; q.y_ld = y_ld; q.y_bs = y_bs; q.w = w; q.bias = bias; q.I = I; q.T = T;
    hipLaunchKernelGGL(fcpe_glu_dw_silu_kernel, dim3((I + FCPE_DW_CH - 1) / FCPE_DW_CH, (T + FCPE_DW_TT - 1) / FCPE_DW_TT, B), dim3(256), 0, s, q);
}

static void add_fcpe_layernorm(Plan &pl, const T1 &x, const T1 &y, const float *g, const float *b)
{
    if (x.C != y.C || x.T != y.T || x.B != y.B) throw ShapeError("fcpe layernorm: shape");
    FcpeLnP q{};
    q.x = x.p; q.x_ld = x.ld; q.x_bs = x.bs; q.y = y.p; q.y_ld = y.ld; q.y_bs = y.bs; q.g = g; q.b = b; q.C = x.C; q.T = x.T;
    const dim3 grid((x.T + 15) / 16, x.B);
    pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(fcpe_layernorm_kernel, grid, dim3(256), 0, s, q); });
}

// raw f0 [B][Tm] of the last f0_extractor_frame samples of each stream of pl.d_in ([B][L]), on RMVPE's frame grid: build_yin's contract
float *build_fcpe(rvc_engine *e, Plan &pl, int B, size_t L, size_t frame16k)
{
    if (!e->fc) throw std::logic_error("f0 method");
    const ModelFC &m = *e->fc;
    const size_t fr = 5120 * ((frame16k + 800 - 1) / 5120 + 1) - 160;     // rmvpe.rs:256
    if (fr > L) throw PanicError("input shorter than f0_extractor_frame");
    const int Tm = (int)(1 + fr / 160);
    if (Tm % 32 != 0) throw PanicError("mel frame count is not a multiple of 32 (rmvpe.rs:229-233 branch)");
    if (Tm > 1024) throw ShapeError("f0 window too long");
    pl.Tm = Tm;
    Arena &A = pl.arena;
    const int H = m.H, I = m.I;
    // front end: RMVPE's kernel and launch shape on FCPE's tables; its image output (the log-mel with an affine, here the identity) goes to a scratch image
    float *d_mel = A.floats((size_t)B * FCPE_MELS * Tm);
    const T2 img = make_t2(A, B, 1, Tm, FCPE_MELS);
    add_mel_frontend_tables(e, pl, B, pl.d_in, (long long)L, (int)L, (int)fr, Tm, d_mel, img, 1.0f, 0.0f, m.basis, m.band);
    const T1 mel = make_t1(A, B, FCPE_MELS, Tm, 1);
    {
        const long long total = (long long)B * FCPE_MELS * Tm;
        const dim3 grid((unsigned)((total + 255) / 256));
        pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(fcpe_mel_pad_kernel, grid, dim3(256), 0, s, d_mel, Tm, total, mel.p, mel.ld, mel.bs); });
    }
    add_tap(pl, "fc.mel", mel);
    // input stack
    const T1 s0 = make_t1(A, B, H, Tm, 0), s1 = make_t1(A, B, H, Tm, 1);
    add_conv1d(pl, m.in0, mel, s0, 1, 1, 1);
    {
        FcpeGnP q{};
        q.x = s0.p; q.x_ld = s0.ld; q.x_bs = s0.bs; q.y = s1.p; q.y_ld = s1.ld; q.y_bs = s1.bs; q.g = m.gn_g; q.b = m.gn_b; q.Cg = H / 4; q.T = Tm; q.slope = 0.01f;
        const dim3 grid(4, B);
        pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(fcpe_gn_lrelu_kernel, grid, dim3(256), 0, s, q); });
    }
    T1 x = make_t1(A, B, H, Tm, 0), x2 = make_t1(A, B, H, Tm, 0);
    add_conv1d(pl, m.in1, s1, x, 1, 1, 1);
    add_tap(pl, "fc.stack", x);
    // the layers: x <- x + pw2(silu(dw(glu(pw1(LayerNorm(x)))))); the residual add is the last GEMM's epilogue, writing the other of two buffers
    const T1 n = make_t1(A, B, H, Tm, 0), z = make_t1(A, B, 2 * I, Tm, 0), d = make_t1(A, B, I, Tm, 0);
    for (int l = 0; l < m.layers; l++) {
        const ModelFC::Layer &y = m.ly[l];
        add_fcpe_layernorm(pl, x, n, y.ln_g, y.ln_b);
        add_conv1d(pl, y.pw1, n, z, 1, 0, 1);
        {
            const float *w = y.dw_w, *bias = y.dw_b;
            pl.ops.push_back([=](hipStream_t s) { launch_fcpe_glu_dw(s, B, I, Tm, z.p, z.ld, z.bs, w, bias, d.p, d.ld, d.bs); });
        }
        if (l == 0) add_tap(pl, "fc.l0.dw", d);
        { ConvOpts o; o.res = x.p; o.res_cs = x.ld; o.res_bs = x.bs; add_conv1d(pl, y.pw2, d, x2, 1, 0, 1, o); }
        std::swap(x, x2);
        add_tap(pl, fmt("fc.l%d", l).c_str(), x);
    }
    add_fcpe_layernorm(pl, x, n, m.norm_g, m.norm_b);
    const T1 logit = make_t1(A, B, FCPE_BINS, Tm, 0);
    add_conv1d(pl, m.out, n, logit, 1, 0, 1);
    float *prob = A.floats((size_t)B * Tm * FCPE_BINS), *f0 = A.floats((size_t)B * Tm);
    {
        const float *tab = m.f0tab; const double thr = pl.key.fcpe_threshold;
        pl.ops.push_back([=](hipStream_t s) { launch_fcpe_decode(s, B, Tm, logit.p, logit.ld, logit.bs, nullptr, prob, tab, thr, f0, nullptr); });
    }
    { T1 t; t.p = prob; t.B = B; t.C = Tm; t.T = FCPE_BINS; t.ld = FCPE_BINS; t.bs = (long long)Tm * FCPE_BINS; add_tap(pl, "fc.prob", t); }
    { T1 t; t.p = f0; t.B = B; t.C = 1; t.T = Tm; t.ld = Tm; t.bs = Tm; add_tap(pl, "fc.f0", t); }
    return f0;
}

}  // namespace rvc
