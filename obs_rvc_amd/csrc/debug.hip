// debug.hip -- the test and tuning aids of include/rvc_mi355x_debug.h that build a plan of their own or read the last call's plan.  None of this is
// the engine: every aid queues launches with the planner calls the models use (engine_int.h), runs them through one harness (run_ops) and hands the
// tensors back to the caller.  The hooks that read another unit's statics live with those statics (rvc_debug_option, rvc_debug_autotune_*,
// rvc_debug_weight_slabs: plan.hip; rvc_debug_session_sola_ms: session.hip.h; rvc_debug_formant_table: engine.hip).
#include "engine_int.h"
#include "../../include/rvc_mi355x_debug.h"
#include <deque>

namespace {

// the whole allocation of a test aid's tensor: its start and geo = (size, offset of element (0, 0, 0), C, T (2-D: W), ld, bs, cs, H (1-D: 1))
struct DebugGeo {
    float *base = nullptr; long long g[8] = {0, 0, 0, 0, 0, 0, 0, 1};
    bool live() const { return base && g[0] > 0; }
    void upload(const float *h) const { if (live()) HIPCHK(hipMemcpy(base, h, (size_t)g[0] * 4, hipMemcpyHostToDevice)); }
    void download(float *h) const { if (live()) HIPCHK(hipMemcpy(h, base, (size_t)g[0] * 4, hipMemcpyDeviceToHost)); }
};
DebugGeo debug_geo1(const T1 &t)
{
    DebugGeo q; const size_t gd = t1_guard(t.ld);
    q.base = t.p - gd - t.halo; q.g[0] = (long long)t.B * t.bs + 2 * (long long)gd; q.g[1] = (long long)gd + t.halo; q.g[2] = t.C; q.g[3] = t.T; q.g[4] = t.ld; q.g[5] = t.bs; q.g[6] = t.ld;
    return q;
}
DebugGeo debug_geo2(const T2 &t)
{
    DebugGeo q; const size_t gd = t2_guard(t.ld);
    q.base = t.p - gd - t.ld - 1; q.g[0] = (long long)t.B * t.bs + 2 * (long long)gd; q.g[1] = (long long)gd + t.ld + 1; q.g[2] = t.C; q.g[3] = t.W; q.g[4] = t.ld; q.g[5] = t.bs; q.g[6] = t.cs; q.g[7] = t.H;
    return q;
}
DebugGeo debug_geo_flat(float *p, long long n, int C, int T) { DebugGeo q; q.base = p; q.g[0] = n; q.g[1] = 0; q.g[2] = C; q.g[3] = T; q.g[4] = T; q.g[5] = (long long)C * T; q.g[6] = T; return q; }

// a launch that throws while the stream is capturing must not leave it in capture mode: the capture is ended and its partial graph dropped
void end_failed_capture(hipStream_t st) { hipGraph_t g = nullptr; (void)hipStreamEndCapture(st, &g); if (g) (void)hipGraphDestroy(g); (void)hipGetLastError(); }

// the one run of every aid: the plan's ops `reps` times on the engine's stream, eagerly or -- graph -- captured once and the graph replayed `reps` times;
// returns with the stream idle and no error pending
void run_ops(rvc_engine *e, Plan &pl, int reps, bool graph)
{
    HIPCHK(hipDeviceSynchronize());
    if (graph) {
        hipGraph_t g; hipGraphExec_t ge;
        HIPCHK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
        try { for (auto &o : pl.ops.v) o(e->stream); } catch (...) { end_failed_capture(e->stream); throw; }
        HIPCHK(hipStreamEndCapture(e->stream, &g));
        const hipError_t ie = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        HIPCHK(ie);
        hipError_t le = hipSuccess;
        for (int r = 0; r < reps && le == hipSuccess; r++) le = hipGraphLaunch(ge, e->stream);
        const hipError_t se = hipStreamSynchronize(e->stream);
        (void)hipGraphExecDestroy(ge);
        HIPCHK(le); HIPCHK(se);
    } else {
        for (int r = 0; r < reps; r++) for (auto &o : pl.ops.v) o(e->stream);
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    HIPCHK(hipGetLastError());
}

// the device weights of one aid, released on every exit (a throw included).  Declared behind the aid's Plan, so that they go before the plan does.
struct DebugWeights {
    std::deque<ConvW> convs; std::deque<ResBlockW> blocks; std::vector<float *> raw;
    DebugWeights() = default;
    DebugWeights(const DebugWeights &) = delete;
    ConvW &conv(ConvW c) { convs.push_back(std::move(c)); return convs.back(); }
    ResBlockW &block(ResBlockW b) { blocks.push_back(std::move(b)); return blocks.back(); }
    float *dev(float *p) { raw.push_back(p); return p; }
    ~DebugWeights() { for (ConvW &c : convs) free_conv(c); for (ResBlockW &b : blocks) free_res_block(b); for (float *p : raw) wfree(p); }
};

// the deterministic data of the *_check / tuning aids
void fill_weights(std::vector<float> &w) { for (size_t i = 0; i < w.size(); i++) w[i] = (float)((i * 2654435761u) % 1000) / 1000.0f - 0.5f; }
void fill_input(std::vector<float> &x) { for (size_t i = 0; i < x.size(); i++) x[i] = (float)(((i * 40503u) ^ (i >> 3)) % 2001) / 1000.0f - 1.0f; }

}  // namespace

extern "C" {

// timeline of the last call (RVC_STAMPS=1): "name us-since-first-stamp" lines
int rvc_debug_stamps(rvc_engine *e, char *buf, size_t cap)
{
    if (!e || !e->last_plan || !e->last_plan->d_stamps) return 0;
    Plan &pl = *e->last_plan;
    std::vector<unsigned long long> h(pl.stamp_names.size());
    if (hipMemcpy(h.data(), pl.d_stamps, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    unsigned long long t0 = ~0ull; for (auto v : h) t0 = std::min(t0, v);
    std::string out;
    for (size_t i = 0; i < h.size(); i++) { char ln[96]; snprintf(ln, sizeof ln, "%s %.2f\n", pl.stamp_names[i].c_str(), (double)(h[i] - t0) / 100.0); out += ln; }
    if (out.size() + 1 > cap) return -1;
    memcpy(buf, out.c_str(), out.size() + 1);
    return (int)h.size();
}

#ifdef RVC_TUNING
// tuning build only: time one Conv1d(Cin -> M, KW taps, dilation dil, stride 1, "same" padding) over N positions and `streams` streams,
// through whatever kernel the planner (or RVC_FORCE_CFG) picks; returns microseconds per launch
double rvc_debug_conv_bench(rvc_engine *e, int M, int Cin, int KW, int dil, int N, int iters, int pre_act, int streams, int act)
{
    double us = -1.0;
    (void)guarded(e, [&]() {
        std::vector<float> w((size_t)M * Cin * KW), bias(M, 0.1f);
        fill_weights(w);
        const int Bb = streams > 0 ? streams : 1;
        Plan pl; pl.key.B = Bb;
        DebugWeights wts;
        ConvW &cw = wts.conv(prep_conv(w.data(), bias.data(), M, Cin, KW, 1));
        const int pad = (KW - 1) * dil / 2;
        T1 x = make_t1(pl.arena, Bb, Cin, N, (pad + 3) / 4 * 4), y = make_t1(pl.arena, Bb, M, N, 0);
        std::vector<float> hx((size_t)Cin * x.ld, 0.25f);
        for (int b = 0; b < Bb; b++) HIPCHK(hipMemcpy(x.p + (long long)b * x.bs - x.halo, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
        ConvOpts o; if (pre_act) { o.pre_act = ACT_LRELU; o.pre_slope = 0.1f; }
        o.act = act;
        add_conv1d(pl, cw, x, y, 1, pad, dil, o);
        run_ops(e, pl, 3, false);
        hipEvent_t a, b; HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
        HIPCHK(hipEventRecord(a, e->stream));
        for (int i = 0; i < iters; i++) for (auto &op : pl.ops.v) op(e->stream);
        HIPCHK(hipEventRecord(b, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        float ms; HIPCHK(hipEventElapsedTime(&ms, a, b));
        us = ms * 1e3 / iters;
        (void)hipEventDestroy(a); (void)hipEventDestroy(b);
        return RVC_OK;
    });
    return us;
}

// tuning build only (-DRVC_KPROBE): one launch of a Conv1d with per-wave phase stamps (device wall clock, 10 ns ticks):
// out[wave][16]; returns the number of waves (workgroups * waves per workgroup), *event_us = the dispatch's own begin..end time
int rvc_debug_conv_probe(rvc_engine *e, int M, int Cin, int KW, int dil, int N, unsigned long long *out, size_t cap_waves, double *event_us, int *waves_per_wg)
{
    int nw = -1;
    (void)guarded(e, [&]() {
        std::vector<float> w((size_t)M * Cin * KW), bias(M, 0.1f);
        fill_weights(w);
        Plan pl; pl.key.B = 1;
        DebugWeights wts;
        ConvW &cw = wts.conv(prep_conv(w.data(), bias.data(), M, Cin, KW, 1));
        const int pad = (KW - 1) * dil / 2;
        T1 x = make_t1(pl.arena, 1, Cin, N, (pad + 3) / 4 * 4), y = make_t1(pl.arena, 1, M, N, 0);
        std::vector<float> hx((size_t)Cin * x.ld, 0.25f);
        HIPCHK(hipMemcpy(x.p - x.halo, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
        const size_t pbytes = (size_t)1 << 24;
        unsigned long long *d_probe = (unsigned long long *)pl.arena.alloc(pbytes);          // (zeroed by the arena)
        ConvOpts o; if (const char *a = tune_env("RVC_BENCH_ACT")) o.act = atoi(a);
        {
            struct Probing { Probing(unsigned long long *p) { g_kprobe = p; } ~Probing() { g_kprobe = nullptr; } } probing(d_probe);
            add_conv1d(pl, cw, x, y, 1, pad, dil, o);
        }
        run_ops(e, pl, 5, false);
        HIPCHK(hipMemset(d_probe, 0, pbytes));
        pl.profile = true; pl.prof_used = 0;
        run_ops(e, pl, 1, false);
        float t = 0.f; HIPCHK(hipEventElapsedTime(&t, pl.prof[0].a, pl.prof[0].b));
        if (event_us) *event_us = t * 1e3;
        nw = g_last_wgs * g_last_waves;
        if (waves_per_wg) *waves_per_wg = g_last_waves;
        if ((size_t)nw <= cap_waves && (size_t)nw * 128 <= pbytes) HIPCHK(hipMemcpy(out, d_probe, (size_t)nw * 128, hipMemcpyDeviceToHost));
        else nw = -2;
        return RVC_OK;
    });
    return nw;
}
#endif

// test aid for the folded LayerNorm (IgemmP::ln_*): two launches on deterministic data against a double-precision host evaluation --
//   (1) y1 = W1 . LN(x) + b1 through the folded weights on the RAW x, publishing the column statistics;
//   (2) y2 = W2 . z + b2 + LN(x), the residual normalised on the fly from the statistics launch (1) published (needs M2 = K rows).
// Tile shape / K split are whatever the planner (or RVC_FORCE_CFG) picks; the planner forces an in-workgroup K split.  Returns the
// largest |gpu - host| / rms(host) over both outputs and the published (mean, rstd); negative on failure.  `offset` = mean of the
// tensor being normalised (spread ~1.15): large values probe the cancellation in the one-pass statistics.
double rvc_debug_ln_fold_check(rvc_engine *e, int M, int K, int N, float offset)
{
    double worst = -1.0;
    (void)guarded(e, [&]() {
        if (K % 16 != 0) throw ShapeError("K must be a multiple of 16");
        auto rnd = [](size_t i, unsigned salt) { return (float)((((i + 1) * 2654435761u) ^ (salt * 40503u) ^ (i >> 5)) % 2001) / 1000.0f - 1.0f; };
        std::vector<float> w1((size_t)M * K), b1(M), w2((size_t)K * M), b2(K), g(K), beta(K), hx((size_t)K * N), hz((size_t)M * N);
        for (size_t i = 0; i < w1.size(); i++) w1[i] = 0.5f * rnd(i, 1);
        for (size_t i = 0; i < w2.size(); i++) w2[i] = 0.5f * rnd(i, 2);
        for (int m = 0; m < M; m++) b1[m] = 0.1f * rnd(m, 3);
        for (int k = 0; k < K; k++) { b2[k] = 0.1f * rnd(k, 4); g[k] = 1.0f + 0.3f * rnd(k, 5); beta[k] = 0.2f * rnd(k, 6); }
        for (size_t i = 0; i < hx.size(); i++) hx[i] = 2.0f * rnd(i, 7) + offset;        // column mean = offset, spread ~1.15
        for (size_t i = 0; i < hz.size(); i++) hz[i] = rnd(i, 8);
        Plan pl; pl.key.B = 1;
        DebugWeights wts;
        float *wsum = nullptr;
        ConvW &c1 = wts.conv(ModelCV::fold_ln(w1.data(), b1.data(), M, K, g.data(), beta.data(), &wsum));
        wts.dev(wsum);
        ConvW &c2 = wts.conv(prep_conv(w2.data(), b2.data(), K, M, 1, 1));
        float *dg = wts.dev(upload_f(g)), *dbeta = wts.dev(upload_f(beta));
        T1 x = make_t1(pl.arena, 1, K, N, 0), y1 = make_t1(pl.arena, 1, M, N, 0), z = make_t1(pl.arena, 1, M, N, 0), y2 = make_t1(pl.arena, 1, K, N, 0);
        float *st = pl.arena.floats((size_t)2 * N + 16);
        for (int k = 0; k < K; k++) HIPCHK(hipMemcpy(x.p + (long long)k * x.ld, &hx[(size_t)k * N], (size_t)N * 4, hipMemcpyHostToDevice));
        for (int m = 0; m < M; m++) HIPCHK(hipMemcpy(z.p + (long long)m * z.ld, &hz[(size_t)m * N], (size_t)N * 4, hipMemcpyHostToDevice));
        { ConvOpts o; o.ln_wsum = wsum; o.ln_stats_out = st; o.ln_rows = K; add_conv1d(pl, c1, x, y1, 1, 0, 1, o); }
        { ConvOpts o; o.res = x.p; o.res_cs = x.ld; o.res_bs = x.bs; o.ln_stats_in = st; o.ln_g = dg; o.ln_b = dbeta; add_conv1d(pl, c2, z, y2, 1, 0, 1, o); }
        run_ops(e, pl, 1, false);
        // host: LayerNorm over the K rows of every column (two-pass, double), then the two layers
        std::vector<double> ln((size_t)K * N), mean(N), rstd(N);
        for (int n = 0; n < N; n++) {
            double s = 0; for (int k = 0; k < K; k++) s += hx[(size_t)k * N + n];
            const double mu = s / K; double q = 0;
            for (int k = 0; k < K; k++) { const double d = hx[(size_t)k * N + n] - mu; q += d * d; }
            mean[n] = mu; rstd[n] = 1.0 / std::sqrt(q / K + 1e-5);
            for (int k = 0; k < K; k++) ln[(size_t)k * N + n] = (hx[(size_t)k * N + n] - mu) * rstd[n] * g[k] + beta[k];
        }
        double err = 0.0;
        std::vector<float> row(N), hst((size_t)2 * N);
        {
            double ss = 0; std::vector<double> ref((size_t)M * N);
            for (int m = 0; m < M; m++) for (int n = 0; n < N; n++) {
                double a = b1[m]; for (int k = 0; k < K; k++) a += (double)w1[(size_t)m * K + k] * ln[(size_t)k * N + n];
                ref[(size_t)m * N + n] = a; ss += a * a;
            }
            const double rms1 = std::sqrt(ss / ((double)M * N)) + 1e-12;
            for (int m = 0; m < M; m++) {
                HIPCHK(hipMemcpy(row.data(), y1.p + (long long)m * y1.ld, (size_t)N * 4, hipMemcpyDeviceToHost));
                for (int n = 0; n < N; n++) err = std::max(err, std::fabs((double)row[n] - ref[(size_t)m * N + n]) / rms1);
            }
        }
        {
            double ss = 0; std::vector<double> ref((size_t)K * N);
            for (int k = 0; k < K; k++) for (int n = 0; n < N; n++) {
                double a = b2[k]; for (int m = 0; m < M; m++) a += (double)w2[(size_t)k * M + m] * hz[(size_t)m * N + n];
                a += ln[(size_t)k * N + n];
                ref[(size_t)k * N + n] = a; ss += a * a;
            }
            const double rms2 = std::sqrt(ss / ((double)K * N)) + 1e-12;
            for (int k = 0; k < K; k++) {
                HIPCHK(hipMemcpy(row.data(), y2.p + (long long)k * y2.ld, (size_t)N * 4, hipMemcpyDeviceToHost));
                for (int n = 0; n < N; n++) err = std::max(err, std::fabs((double)row[n] - ref[(size_t)k * N + n]) / rms2);
            }
        }
        HIPCHK(hipMemcpy(hst.data(), st, (size_t)2 * N * 4, hipMemcpyDeviceToHost));
        for (int n = 0; n < N; n++) {
            err = std::max(err, std::fabs((double)hst[2 * n] - mean[n]) / (std::fabs(mean[n]) + 1.0));
            err = std::max(err, std::fabs((double)hst[2 * n + 1] - rstd[n]) / rstd[n]);
        }
        worst = err;
        return RVC_OK;
    });
    return worst;
}

// test aid: one Conv1d(Cin -> M, KW taps, dilation dil, "same" padding, bias, optional input LeakyReLU) over N positions and `streams`
// streams on deterministic data, through whatever tile configuration the planner (or RVC_FORCE_CFG) picks, against a double-precision
// host evaluation.  Returns the largest |gpu - host| / (rms(host) + 1e-12); negative on failure.
double rvc_debug_conv_check(rvc_engine *e, int M, int Cin, int KW, int dil, int N, int streams, int pre_act)
{
    double worst = -1.0;
    (void)guarded(e, [&]() {
        std::vector<float> w((size_t)M * Cin * KW), bias(M);
        fill_weights(w);
        for (int m = 0; m < M; m++) bias[m] = 0.01f * (float)(m % 7) - 0.02f;
        Plan pl; pl.key.B = streams;
        DebugWeights wts;
        ConvW &cw = wts.conv(prep_conv(w.data(), bias.data(), M, Cin, KW, 1));
        const int pad = (KW - 1) * dil / 2, halo = (pad + 3) / 4 * 4;
        T1 x = make_t1(pl.arena, streams, Cin, N, halo), y = make_t1(pl.arena, streams, M, N, 0);
        std::vector<float> hx((size_t)streams * Cin * N);
        fill_input(hx);
        for (int b = 0; b < streams; b++)
            for (int c = 0; c < Cin; c++)
                HIPCHK(hipMemcpy(x.p + (long long)b * x.bs + (long long)c * x.ld, &hx[((size_t)b * Cin + c) * N], (size_t)N * 4, hipMemcpyHostToDevice));
        ConvOpts o; if (pre_act) { o.pre_act = ACT_LRELU; o.pre_slope = 0.1f; }
        add_conv1d(pl, cw, x, y, 1, pad, dil, o);
        run_ops(e, pl, 1, false);
        // host evaluation in double, the (stream, output row) pairs dealt to the host's threads (a test aid: the full-size shapes are 1e9 MACs each)
        std::vector<float> hy((size_t)streams * M * N);
        for (int b = 0; b < streams; b++)
            HIPCHK(hipMemcpy2D(&hy[(size_t)b * M * N], (size_t)N * 4, y.p + (long long)b * y.bs, (size_t)y.ld * 4, (size_t)N * 4, M, hipMemcpyDeviceToHost));
        const int nthr = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        std::vector<double> errs(nthr, 0.0), sss(nthr, 0.0);
        std::vector<std::thread> pool;
        for (int t = 0; t < nthr; t++)
            pool.emplace_back([&, t]() {
                std::vector<double> ref((size_t)N);
                for (long long bm = t; bm < (long long)streams * M; bm += nthr) {
                    const int b = (int)(bm / M), m = (int)(bm % M);
                    for (int n = 0; n < N; n++) {
                        double a = bias[m];
                        for (int c = 0; c < Cin; c++)
                            for (int k = 0; k < KW; k++) {
                                const int tt = n + k * dil - pad;
                                if (tt < 0 || tt >= N) continue;
                                double v = hx[((size_t)b * Cin + c) * N + tt];
                                if (pre_act && v < 0) v *= 0.1f;
                                a += (double)w[((size_t)m * Cin + c) * KW + k] * v;
                            }
                        ref[n] = a; sss[t] += a * a;
                    }
                    const float *row = &hy[((size_t)b * M + m) * N];
                    for (int n = 0; n < N; n++) errs[t] = std::max(errs[t], std::fabs((double)row[n] - ref[n]));
                }
            });
        for (auto &th : pool) th.join();
        double err = 0.0, ss = 0.0; const size_t cnt = (size_t)streams * M * N;
        for (int t = 0; t < nthr; t++) { err = std::max(err, errs[t]); ss += sss[t]; }
        worst = err / (std::sqrt(ss / (double)std::max<size_t>(cnt, 1)) + 1e-12);
        return RVC_OK;
    });
    return worst;
}

// test aid: one Conv2d(Cin -> M, 3x3, pad 1, bias, ReLU) [kind 0] or ConvTranspose2d(Cin -> M, 3x3, stride 2, pad 1, output_pad 1, bias, ReLU) [kind 1] on
// `streams` images of H x W (RMVPE's layers, rvc/src/f0/rmvpe.rs:235-238), residual 0 = none, 1 = + a residual tensor, 2 = accumulate into the
// output; deterministic data, whatever kernel the planner (or a hook) picks, against a double-precision host evaluation.
// Returns the largest |gpu - host| / (rms(host) + 1e-12); negative on failure.
double rvc_debug_conv2d_check(rvc_engine *e, int M, int Cin, int H, int W, int streams, int kind, int residual)
{
    double worst = -1.0;
    (void)guarded(e, [&]() {
        if (kind == 1 && residual) throw ShapeError("transposed test layer takes no residual");
        std::vector<float> w((size_t)M * Cin * 9), bias(M);
        fill_weights(w);
        for (int m = 0; m < M; m++) bias[m] = 0.01f * (float)(m % 7) - 0.02f;
        Plan pl; pl.key.B = streams;
        DebugWeights wts;
        // Conv2d: w [M][Cin][3][3]; ConvTranspose2d: w [Cin][M][3][3]
        ConvW &cw = wts.conv(kind == 0 ? prep_conv(w.data(), bias.data(), M, Cin, 9, 1) : prep_convT2d(w.data(), bias.data(), Cin, M));
        const int OH = kind ? 2 * H : H, OW = kind ? 2 * W : W;
        T2 x = make_t2(pl.arena, streams, Cin, H, W), y = make_t2(pl.arena, streams, M, OH, OW), r = make_t2(pl.arena, streams, M, OH, OW);
        std::vector<float> hx((size_t)streams * Cin * H * W), hr((size_t)streams * M * OH * OW);
        fill_input(hx);
        for (size_t i = 0; i < hr.size(); i++) hr[i] = (float)(((i * 9973u) ^ (i >> 2)) % 1001) / 1000.0f - 0.5f;
        for (int b = 0; b < streams; b++)
            for (int c = 0; c < Cin; c++)
                HIPCHK(hipMemcpy2D(x.p + (long long)b * x.bs + (long long)c * x.cs, (size_t)x.ld * 4, &hx[(((size_t)b * Cin + c) * H) * W], (size_t)W * 4, (size_t)W * 4, H, hipMemcpyHostToDevice));
        for (int b = 0; b < streams; b++)
            for (int c = 0; c < M; c++) {
                T2 &dst = residual == 2 ? y : r;
                HIPCHK(hipMemcpy2D(dst.p + (long long)b * dst.bs + (long long)c * dst.cs, (size_t)dst.ld * 4, &hr[(((size_t)b * M + c) * OH) * OW], (size_t)OW * 4, (size_t)OW * 4, OH, hipMemcpyHostToDevice));
            }
        ConvOpts o; o.act = ACT_RELU;
        if (residual == 1) { o.res = r.p; o.res_cs = r.cs; o.res_bs = r.bs; o.res_rs = r.ld; }
        if (residual == 2) o.accumulate = true;
        if (kind == 0) add_conv2d(pl, cw, x, y, o); else add_convT2d(pl, cw, x, y, o);
        run_ops(e, pl, 1, false);
        std::vector<float> hy((size_t)OH * OW);
        std::vector<double> ref((size_t)OH * OW);
        double err = 0.0, ss = 0.0; size_t cnt = 0;
        for (int b = 0; b < streams; b++)
            for (int m = 0; m < M; m++) {
                HIPCHK(hipMemcpy2D(hy.data(), (size_t)OW * 4, y.p + (long long)b * y.bs + (long long)m * y.cs, (size_t)y.ld * 4, (size_t)OW * 4, OH, hipMemcpyDeviceToHost));
                for (int oh = 0; oh < OH; oh++)
                    for (int ow = 0; ow < OW; ow++) {
                        double a = bias[m];
                        for (int c = 0; c < Cin; c++) {
                            const float *xc = &hx[(((size_t)b * Cin + c) * H) * W];
                            for (int kh = 0; kh < 3; kh++)
                                for (int kw = 0; kw < 3; kw++) {
                                    if (kind == 0) {
                                        const int ih = oh + kh - 1, iw = ow + kw - 1;
                                        if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
                                        a += (double)w[(((size_t)m * Cin + c) * 3 + kh) * 3 + kw] * xc[(size_t)ih * W + iw];
                                    } else {
                                        // out[oh] += w[kh] * in[ih] with oh = 2 ih - 1 + kh
                                        const int th = oh + 1 - kh, tw = ow + 1 - kw;
                                        if (th < 0 || tw < 0 || (th & 1) || (tw & 1)) continue;
                                        const int ih = th / 2, iw = tw / 2;
                                        if (ih >= H || iw >= W) continue;
                                        a += (double)w[(((size_t)c * M + m) * 3 + kh) * 3 + kw] * xc[(size_t)ih * W + iw];
                                    }
                                }
                        }
                        a = a > 0 ? a : 0;
                        if (residual) a += hr[(((size_t)b * M + m) * OH + oh) * OW + ow];
                        ref[(size_t)oh * OW + ow] = a; ss += a * a; cnt++;
                    }
                for (size_t i = 0; i < ref.size(); i++) err = std::max(err, std::fabs((double)hy[i] - ref[i]));
            }
        worst = err / (std::sqrt(ss / (double)std::max<size_t>(cnt, 1)) + 1e-12);
        return RVC_OK;
    });
    return worst;
}

// test aid: one convolution layer as the models build it (include/rvc_mi355x_debug.h, tests/test_gpu_layers.py).  The caller owns every float of the
// tensors' allocations: what the layer must not touch is compared bit for bit afterwards.
int rvc_debug_layer(rvc_engine *e, const rvc_debug_layer_spec *s, const float *w, const float *bias, float *x, float *y, float *r, long long *geo)
{
    return (int)guarded(e, [&]() {
        if (!s || !geo || s->streams < 1 || s->form < 0 || s->form > 4 || ((s->form == 2 || s->form == 3) && (s->n < 1 || s->n > 4))) throw ShapeError("layer spec");
        const int B = s->streams, form = s->form, n = form == 3 ? 2 : s->n;
        Plan pl; pl.key.B = B;
        pl.key.bf3 = e->gemm_precision == 1;      // the engine's setting, as a real plan's key has it (engine.hip): rvc_set_gemm_precision(e, 1) lets queue_bf3 take the layer
        DebugWeights wts;
        DebugGeo gx, gy, gr;
        T1 x1, y1, r1; T2 x2, y2, r2;
        const int yrows = form == 2 ? n * s->cout : (form == 3 ? 3 * s->cout + 16 : (s->glu ? s->cout / 2 : s->cout));
        if (form == 4) {
            x2 = make_t2(pl.arena, B, s->cin, s->t_in, s->t_out); gx = debug_geo2(x2);
            if (s->y_ws) {
                y1 = make_t1(pl.arena, B, s->cout * s->t_out, s->t_in, 0); gy = debug_geo1(y1);
                y2.p = y1.p; y2.B = B; y2.C = s->cout; y2.H = s->t_in; y2.W = s->t_out; y2.cs = s->t_out * y1.ld; y2.ld = 1; y2.bs = y1.bs;
            } else { y2 = make_t2(pl.arena, B, s->cout, s->t_in, s->t_out); gy = debug_geo2(y2); }
            if (s->res == 1) { r2 = make_t2(pl.arena, B, s->cout, s->t_in, s->t_out); gr = debug_geo2(r2); }
        } else {
            x1 = make_t1(pl.arena, B, (form == 2 && s->x_grouped) ? n * s->cin : s->cin, s->t_in, s->x_halo); gx = debug_geo1(x1);
            y1 = make_t1(pl.arena, B, yrows, s->t_out, s->y_halo); gy = debug_geo1(y1);
            if (s->res == 1) { r1 = make_t1(pl.arena, B, (form == 2 && s->res_grouped) ? n * s->cout : s->cout, s->t_out, s->r_halo); gr = debug_geo1(r1); }
        }
        if (s->res == 2) { r1 = make_t1(pl.arena, 1, 1, s->t_out, 0); gr = debug_geo1(r1); }
        for (int i = 0; i < 8; i++) { geo[i] = gx.g[i]; geo[8 + i] = gy.g[i]; geo[16 + i] = gr.g[i]; }
        if (!x) return RVC_OK;
        if (!y || !w || ((s->res == 1 || s->res == 2) && !r)) throw ShapeError("layer buffers");
        gx.upload(x); gy.upload(y); gr.upload(r);
        ConvOpts o;
        o.act = s->act; o.slope = s->slope; o.scale = s->scale; o.accumulate = s->accumulate != 0;
        o.pre_act = s->pre_act; o.pre_slope = s->pre_slope; o.no_bias = s->no_bias != 0; o.final_out = s->final_out != 0; o.glu = s->glu != 0;
        if (s->res == 1 && form == 4) { o.res = r2.p; o.res_cs = r2.cs; o.res_bs = r2.bs; o.res_rs = r2.ld; }
        else if (s->res == 1) { o.res = r1.p; o.res_cs = r1.ld; o.res_bs = r1.bs; }
        else if (s->res == 2) { o.res = r1.p; o.res_cs = 0; o.res_bs = 0; }
        else if (s->res == 3 && form == 4) { o.res = y2.p; o.res_cs = y2.cs; o.res_bs = y2.bs; o.res_rs = y2.ld; }
        else if (s->res == 3) { o.res = y1.p; o.res_cs = y1.ld; o.res_bs = y1.bs; }
        else if (s->res == 4 && form != 4) { o.res = x1.p; o.res_cs = x1.ld; o.res_bs = x1.bs; }
        if (s->y_ws) o.y_ws = y1.ld;
        std::deque<ConvW> &cws = wts.convs;
        float *pair = nullptr;
        if (form == 0 && s->glu) {
            std::vector<float> wp, bp;
            if (!bias) throw ShapeError("GLU layer without bias");
            glu_pack_rows(w, bias, s->cout / 2, (size_t)s->cin * s->kw, wp, bp);
            wts.conv(prep_conv(wp.data(), bp.data(), s->cout, s->cin, s->kw, 1));
        } else if (form == 0) wts.conv(prep_conv(w, bias, s->cout, s->cin, s->kw, s->groups));
        else if (form == 1) wts.conv(prep_convT1d(w, bias, s->cin, s->cout, s->kw, s->stride));
        else if (form == 4) wts.conv(prep_conv(w, bias, s->cout, s->cin, 9, 1));
        else {
            size_t ow = 0;
            for (int j = 0; j < n; j++) {
                const int kw = form == 3 ? 1 : s->kws[j];
                wts.conv(prep_conv(w + ow, bias ? bias + (size_t)j * s->cout : nullptr, s->cout, s->cin, kw, 1));
                ow += (size_t)s->cout * s->cin * kw;
            }
            if (form == 2 && n > 1) { std::vector<ConvW *> m; for (ConvW &c : cws) m.push_back(&c); merge_convs(m); }
            if (form == 3) { if (!bias) throw ShapeError("pair launch without bias"); pair = wts.dev(upload_f(bias, (size_t)2 * s->cout)); }
        }
        if (form == 0) add_conv1d(pl, cws[0], x1, y1, s->stride, s->pad, s->dil, o);
        else if (form == 1) add_convT1d(pl, cws[0], x1, y1, s->pad, o);
        else if (form == 2) {
            std::vector<const ConvW *> cp; std::vector<int> pads, dils;
            for (int j = 0; j < n; j++) { cp.push_back(&cws[j]); pads.push_back(s->pads[j]); dils.push_back(s->dils[j]); }
            add_conv1d_multi(pl, cp, x1, s->x_grouped != 0, y1, pads, dils, o, s->res_grouped != 0);
        } else if (form == 3) add_conv1d_two(pl, cws[0], cws[1], pair, x1, y1.rows(16, s->cout), y1.rows(16 + 2 * s->cout, s->cout));
        else add_conv2d(pl, cws[0], x2, y2, o);
        run_ops(e, pl, 1, false);
        gx.download(x); gy.download(y); gr.download(r);
        return RVC_OK;
    });
}

// test aid: one attention / LayerNorm / GRU op as the models build it (include/rvc_mi355x_debug.h, tests/test_gpu_ops.py).  As for rvc_debug_layer, the caller
// owns every float of the tensors' allocations.
int rvc_debug_op(rvc_engine *e, const rvc_debug_op_spec *s, const float *w0, const float *w1, float *x, float *y, int *status, long long *geo)
{
    return (int)guarded(e, [&]() {
        if (!s || !geo || s->streams < 1 || s->op < 0 || s->op > 3 || s->T < 1 || s->reps < 1 || s->x_halo < 0 || s->y_halo < 0) throw ShapeError("op spec");
        if ((s->op <= 1 && (s->E < 1 || s->heads < 1 || s->E % s->heads)) || (s->op == 1 && s->window < 0) || (s->op == 2 && s->C < 1) || (s->op == 3 && s->H < 1))
            throw ShapeError("op spec");
        const int B = s->streams, op = s->op;
        Plan pl; pl.key.B = B;
        DebugWeights wts;
        T1 x1, y1;
        if (op <= 1) { x1 = make_t1(pl.arena, B, 3 * s->E, s->T, s->x_halo); y1 = make_t1(pl.arena, B, s->E, s->T, s->y_halo); }
        else if (op == 2) x1 = make_t1(pl.arena, B, s->C, s->T, s->x_halo);
        else { x1 = make_t1(pl.arena, B, 6 * s->H, s->T, s->x_halo); y1 = make_t1(pl.arena, B, 2 * s->H, s->T, s->y_halo); }
        const DebugGeo gx = debug_geo1(x1), gy = op == 2 ? DebugGeo() : debug_geo1(y1);
        for (int i = 0; i < 8; i++) { geo[i] = gx.g[i]; geo[8 + i] = gy.g[i]; }
        if (!x) return RVC_OK;
        if ((op != 2 && !y) || (op != 0 && (!w0 || !w1)) || (op == 3 && !status)) throw ShapeError("op buffers");
        gx.upload(x); gy.upload(y);
        int *d_status = nullptr;
        if (op == 0) add_attention(pl, x1, y1, s->heads);
        else if (op == 1) {
            const size_t n = (size_t)(2 * s->window + 1) * (s->E / s->heads);
            float *rk = wts.dev(upload_f(w0, n)), *rv = wts.dev(upload_f(w1, n));
            add_relpos_attention(pl, x1, y1, s->heads, rk, rv, s->window);
        } else if (op == 2) {
            float *g = wts.dev(upload_f(w0, (size_t)s->C)), *b = wts.dev(upload_f(w1, (size_t)s->C));
            add_layernorm(pl, x1, g, b);
        } else {
            const int H = s->H;
            const float *whh_dir[2] = {w0, w0 + (size_t)3 * H * H};
            std::vector<float> wt, wr;
            gru_prep_whh(whh_dir, H, wt, wr);
            float *dwt = wts.dev(upload_f(wt)), *dwr = wts.dev(upload_f(wr)), *bhh = wts.dev(upload_f(w1, (size_t)6 * H));
            d_status = (int *)pl.arena.alloc((size_t)B * sizeof(int));
            HIPCHK(hipMemset(d_status, 0, (size_t)B * sizeof(int)));
            add_gru(pl, x1, y1, H, dwr, dwt, bhh, d_status, 1);
        }
        run_ops(e, pl, s->reps, s->graph != 0);
        gx.download(x); gy.download(y);
        if (d_status) HIPCHK(hipMemcpy(status, d_status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

// test aid: the mel front end, ContentVec's first layer, the pitch decode and the NSF source as the models build them (include/rvc_mi355x_debug.h,
// tests/test_gpu_front.py).  As for rvc_debug_layer, the caller owns every float of the tensors' allocations; the streams' states live in a block of the
// aid's own, so the engine's streams are not touched.
int rvc_debug_front(rvc_engine *e, const rvc_debug_front_spec *s, const float *w0, const float *w1, float *const *buf, rvc_debug_stream_state *state, long long *geo)
{
    return (int)guarded(e, [&]() {
        if (!s || !geo || s->streams < 1 || s->streams > 4096 || s->op < 4 || s->op > 7) throw ShapeError("front spec");
        const int B = s->streams, op = s->op;
        Plan pl; pl.key.B = B;
        DebugWeights wts;
        Arena &A = pl.arena;
        DebugGeo g[4];
        T1 x1, y1; T2 img; int Tm = 0, R = 0;
        float *f0 = nullptr, *pitchf = nullptr, *mel = nullptr; int *pitch = nullptr;
        if (op == 4) {
            if (s->n < 1 || s->n > (1 << 24) || s->frame < 1 || s->frame > s->n) throw ShapeError("front spec");
            Tm = 1 + s->frame / 160;
            if (Tm > 1024) throw ShapeError("f0 window too long");
            const long long na = (long long)B * s->n + 64;
            g[0] = debug_geo_flat(A.floats((size_t)na), na, 1, s->n);
            mel = A.floats((size_t)B * 128 * Tm); g[1] = debug_geo_flat(mel, (long long)B * 128 * Tm, 128, Tm);
            img = make_t2(A, B, 1, Tm, 128); g[2] = debug_geo2(img);
        } else if (op == 5) {
            if (s->C < 1 || s->C > 4096 || s->L < 10 || s->L > (1 << 22)) throw ShapeError("front spec");
            const long long na = (long long)B * s->L + 64;
            x1.p = A.floats((size_t)na); x1.B = B; x1.C = 1; x1.T = s->L; x1.ld = s->L; x1.halo = 0; x1.bs = s->L;      // the plan's input buffer (build_plan, build_contentvec)
            g[0] = debug_geo_flat(x1.p, na, 1, s->L);
            y1 = make_t1(A, B, s->C, (s->L - 10) / 5 + 1, 0); g[1] = debug_geo1(y1);
        } else if (op == 6) {
            Tm = s->Tm; R = s->update ? s->R : 0;
            if (Tm < 1 || Tm > 1024 || R < 0 || R > 1024) throw ShapeError("front spec");
            x1 = make_t1(A, B, 360, Tm, 0); g[0] = debug_geo1(x1);
            f0 = A.floats((size_t)B * Tm); g[1] = debug_geo_flat(f0, (long long)B * Tm, 1, Tm);
            if (s->update) {
                pitchf = A.floats((size_t)B * std::max(R, 1)); g[2] = debug_geo_flat(pitchf, (long long)B * R, 1, R);
                pitch = (int *)A.alloc((size_t)B * std::max(R, 1) * sizeof(int)); g[3] = debug_geo_flat((float *)pitch, (long long)B * R, 1, R);
            }
        } else {
            if (s->T < 1 || s->T > 4096 || s->upp < 1 || s->upp > 4096 || s->x_halo < 0 || s->x_halo > 4096) throw ShapeError("front spec");
            pitchf = A.floats((size_t)B * s->T); g[0] = debug_geo_flat(pitchf, (long long)B * s->T, 1, s->T);
            y1 = make_t1(A, B, 1, s->T * s->upp, s->x_halo); g[1] = debug_geo1(y1);
        }
        for (int j = 0; j < 4; j++) for (int i = 0; i < 8; i++) geo[8 * j + i] = g[j].base ? g[j].g[i] : 0;
        if (!buf) return RVC_OK;
        if (!state) throw ShapeError("front buffers");
        for (int j = 0; j < 4; j++) if (g[j].live() && !buf[j]) throw ShapeError("front buffers");
        std::vector<StreamState> hst(B);
        for (int b = 0; b < B; b++) {
            memset(&hst[b], 0, sizeof(StreamState));
            hst[b].ctl.protect = (float)PROTECT_OFF;       // (a zero word would mean full protection, state.hip.h; none of these ops reads it)
            hst[b].ctl.uppower = state[b].uppower; hst[b].stream_id = state[b].stream_id; hst[b].chunk = state[b].chunk; hst[b].status = state[b].status;
            memcpy(hst[b].cache_pitchf, state[b].cache_pitchf, sizeof hst[b].cache_pitchf);
        }
        StreamState *d_st = A.upload(hst);
        CallParams hcp{}; hcp.seed = s->seed;
        CallParams *d_cp = A.upload(std::vector<CallParams>(1, hcp));
        if (op == 4) add_mel_frontend(e, pl, B, g[0].base, s->n, s->n, s->frame, Tm, mel, img, s->bn_scale, s->bn_shift);
        else if (op == 5) {
            if (!w0 || !w1) throw ShapeError("front buffers");
            float *dw = wts.dev(upload_f(w0, (size_t)s->C * 10)), *gn = wts.dev(upload_f(w1, (size_t)2 * s->C));
            add_conv0_front(pl, wts.conv(prep_conv(w0, nullptr, s->C, 1, 10, 1)), dw, gn, gn + s->C, 10, 5, x1, y1);
        } else if (op == 6) add_pitch_post(pl, B, x1, Tm, d_st, d_cp, f0, s->update != 0, s->shift, s->cache_start, s->read_start, R, pitchf, pitch);
        else add_nsf_source(pl, B, pitchf, y1, s->T, s->upp, s->sr, s->lin_w, s->lin_b, d_st, d_cp, s->f0_num, s->f0_den);
        for (int j = 0; j < 4; j++) g[j].upload(buf[j]);
        run_ops(e, pl, 1, s->graph != 0);
        for (int j = 0; j < 4; j++) g[j].download(buf[j]);
        HIPCHK(hipMemcpy(hst.data(), d_st, sizeof(StreamState) * B, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; b++) { state[b].status = hst[b].status; memcpy(state[b].cache_pitchf, hst[b].cache_pitchf, sizeof hst[b].cache_pitchf); }
        return RVC_OK;
    });
}

// test aid: protect_mix_kernel alone (protect.hip.h; tests/test_gpu_protect.py) on the caller's arrays with the caller's leading dimensions, launched as the plan
// launches it.  The streams' states are a block of the aid's own: zero but for the protect word.
int rvc_debug_protect(rvc_engine *e, const rvc_debug_protect_spec *s, float *phone, const float *cv, const float *pitchf, const double *protect)
{
    return (int)guarded(e, [&]() {
        if (!s || !phone || !cv || !pitchf || !protect) throw ShapeError("protect spec");
        const int B = s->streams, C = s->C, R = s->R, T = s->T;
        if (B < 1 || B > 4096 || C < 1 || C > 4096 || R < 1 || R > 4096 || T < 1 || T > (1 << 20) || s->skip_head < 0 || s->ph_ld < R || s->cv_ld < T || s->ph_ld > (1 << 20) ||
            s->cv_ld > (1 << 21) || (long long)s->skip_head + R > 2LL * T + 1)
            throw ShapeError("protect spec");
        for (int b = 0; b < B; b++) if (!(protect[b] >= 0.0 && protect[b] <= PROTECT_OFF)) throw ShapeError("protect: value outside [0, 0.5]");
        Plan pl; pl.key.B = B; pl.key.nprobe = e->index_nprobe;
        Arena &A = pl.arena;
        const size_t n_ph = (size_t)B * C * s->ph_ld, n_cv = (size_t)B * C * s->cv_ld, n_pf = (size_t)B * R;
        float *d_ph = A.floats(n_ph), *d_cv = A.floats(n_cv), *d_pf = A.floats(n_pf);
        std::vector<StreamState> hst(B);
        for (int b = 0; b < B; b++) { memset(&hst[b], 0, sizeof(StreamState)); hst[b].ctl.protect = (float)protect[b]; }
        const StreamState *d_st = A.upload(hst);
        HIPCHK(hipMemcpy(d_ph, phone, n_ph * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_cv, cv, n_cv * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_pf, pitchf, n_pf * 4, hipMemcpyHostToDevice));
        const int ph_ld = s->ph_ld, cv_ld = s->cv_ld, skip_head = s->skip_head;
        pl.ops.push_back([=](hipStream_t st) { launch_protect_mix(st, B, d_st, d_pf, d_cv, cv_ld, (long long)C * cv_ld, C, T, skip_head, R, d_ph, ph_ld, (long long)C * ph_ld); });
        run_ops(e, pl, 1, s->graph != 0);
        HIPCHK(hipMemcpy(phone, d_ph, n_ph * 4, hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

// test aid: CREPE's decoder alone (crepe.hip.h; tests/test_gpu_crepe.py) on the caller's posteriors, through the launch a plan uses (launch_crepe_decode)
int rvc_debug_crepe_decode(rvc_engine *e, const float *prob, int B, int Tm, int decoder, float *f0_out, int *bins_out, float *pd_out)
{
    return (int)guarded(e, [&]() {
        if (!prob || !f0_out || B < 1 || B > 64 || Tm < 2 || Tm > 1024 || (decoder != 0 && decoder != 1)) throw ShapeError("crepe decode: B in [1, 64], Tm in [2, 1024], decoder 0 or 1");
        const size_t n = (size_t)B * Tm;
        DevBuf<float> d_prob, d_f0, d_pd, d_tab; DevBuf<int> d_bins; DevBuf<unsigned char> d_bp;
        d_prob.alloc(n * 360); d_f0.alloc(n); d_pd.alloc(n); d_bins.alloc(n); d_tab.alloc(360);
        if (const size_t bpn = crepe_backpointer_bytes(B, Tm)) d_bp.alloc(bpn);
        const std::vector<float> tab = crepe_f0_table();
        HIPCHK(hipMemcpy(d_tab.get(), tab.data(), 360 * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_prob.get(), prob, n * 360 * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipDeviceSynchronize());
        launch_crepe_decode(e->stream, B, d_prob.get(), Tm, decoder, d_tab.get(), d_bp.get(), d_f0.get(), d_bins.get(), d_pd.get());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipMemcpy(f0_out, d_f0.get(), n * sizeof(float), hipMemcpyDeviceToHost));
        if (bins_out) HIPCHK(hipMemcpy(bins_out, d_bins.get(), n * sizeof(int), hipMemcpyDeviceToHost));
        if (pd_out) HIPCHK(hipMemcpy(pd_out, d_pd.get(), n * sizeof(float), hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

// test aid: FCPE's decoder alone (fcpe.hip.h; tests/test_gpu_fcpe.py) on the caller's posteriors, through the launch a plan uses (launch_fcpe_decode), under the
// engine's threshold
int rvc_debug_fcpe_decode(rvc_engine *e, const float *prob, int B, int Tm, float *f0_out, int *bins_out)
{
    return (int)guarded(e, [&]() {
        if (!prob || !f0_out || B < 1 || B > 64 || Tm < 1 || Tm > 1024) throw ShapeError("fcpe decode: B in [1, 64], Tm in [1, 1024]");
        const size_t n = (size_t)B * Tm;
        DevBuf<float> d_prob, d_f0, d_tab; DevBuf<int> d_bins;
        d_prob.alloc(n * 360); d_f0.alloc(n); d_bins.alloc(n); d_tab.alloc(360);
        const std::vector<float> tab = fcpe_f0_table();
        HIPCHK(hipMemcpy(d_tab.get(), tab.data(), 360 * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_prob.get(), prob, n * 360 * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipDeviceSynchronize());
        launch_fcpe_decode(e->stream, B, Tm, nullptr, 0, 0, d_prob.get(), nullptr, d_tab.get(), e->fcpe_threshold, d_f0.get(), d_bins.get());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipMemcpy(f0_out, d_f0.get(), n * sizeof(float), hipMemcpyDeviceToHost));
        if (bins_out) HIPCHK(hipMemcpy(bins_out, d_bins.get(), n * sizeof(int), hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

// test aid: FCPE's GLU + depthwise + SiLU kernel alone (fcpe.hip.h), through the launch a plan uses (launch_fcpe_glu_dw), on contiguous arrays: z [B][2 I][T],
// w [I][31], bias [I] -> y [B][I][T].  Any T: the plan's lengths are multiples of 32, the kernel's time tile is 64
int rvc_debug_fcpe_dw(rvc_engine *e, const float *z, const float *w, const float *bias, int B, int I, int T, float *y_out)
{
    return (int)guarded(e, [&]() {
        if (!z || !w || !bias || !y_out || B < 1 || B > 64 || I < 1 || I > 4096 || T < 1 || T > 4096) throw ShapeError("fcpe depthwise: B in [1, 64], I, T in [1, 4096]");
        const size_t nz = (size_t)B * 2 * I * T, ny = (size_t)B * I * T;
        DevBuf<float> d_z, d_w, d_b, d_y;
        d_z.alloc(nz); d_w.alloc((size_t)I * 31); d_b.alloc(I); d_y.alloc(ny);
        HIPCHK(hipMemcpy(d_z.get(), z, nz * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_w.get(), w, (size_t)I * 31 * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_b.get(), bias, (size_t)I * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipDeviceSynchronize());
        launch_fcpe_glu_dw(e->stream, B, I, T, d_z.get(), T, 2LL * I * T, d_w.get(), d_b.get(), d_y.get(), T, (long long)I * T);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipMemcpy(y_out, d_y.get(), ny * sizeof(float), hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

// test aid: the hybrid-f0 launch alone (f0_hybrid.hip.h; tests/test_gpu_f0_hybrid.py) on the caller's member rows [n][B][Tm] and, optionally, a salience
// [B][360][Tm] decoded in place of member rm_at, through the launch a plan uses (launch_f0_hybrid)
int rvc_debug_f0_hybrid(rvc_engine *e, const float *rows, int n, int B, int Tm, int mode, const float *sal, int rm_at, float *out, float *rm_f0_out, float *ms_out)
{
    return (int)guarded(e, [&]() {
        if (!rows || !out || n < 1 || n > HYBRID_MEMBERS_MAX || B < 1 || B > e->n_streams || Tm < 1 || Tm > 1024 || (mode != 0 && mode != 1) ||
            (sal ? (rm_at < 0 || rm_at >= n) : rm_at != -1))
            throw ShapeError("f0 hybrid: n in [1, 4], B in [1, streams], Tm in [1, 1024], mode 0 or 1, rm_at in [0, n) with a salience and -1 without");
        const size_t bt = (size_t)B * Tm;
        DevBuf<float> d_rows, d_sal, d_out, d_rm;
        d_rows.alloc((size_t)n * bt); d_out.alloc(bt); d_rm.alloc(bt);
        HIPCHK(hipMemcpy(d_rows.get(), rows, (size_t)n * bt * sizeof(float), hipMemcpyHostToDevice));
        if (sal) { d_sal.alloc(bt * 360); HIPCHK(hipMemcpy(d_sal.get(), sal, bt * 360 * sizeof(float), hipMemcpyHostToDevice)); }
        const float *rp[HYBRID_MEMBERS_MAX] = {};
        for (int i = 0; i < n; i++) rp[i] = d_rows.get() + (size_t)i * bt;
        DevTimer tm;
        HIPCHK(hipDeviceSynchronize());
        tm.start(e->stream);
        launch_f0_hybrid(e->stream, B, Tm, n, mode, rp, rm_at, sal ? d_sal.get() : nullptr, Tm, 360LL * Tm, e->d_state, d_rm.get(), d_out.get());
        tm.stop(e->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(e->stream));
        if (ms_out) *ms_out = tm.ms();
        HIPCHK(hipMemcpy(out, d_out.get(), bt * sizeof(float), hipMemcpyDeviceToHost));
        if (rm_f0_out && sal) HIPCHK(hipMemcpy(rm_f0_out, d_rm.get(), bt * sizeof(float), hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

// test aid: the PM method's kernels alone (pm.hip.h; tests/test_gpu_pm.py), through the launches a plan uses: (a) peak + candidates on the caller's audio, (b) the
// path on the caller's candidate arrays (include/rvc_mi355x_debug.h)
int rvc_debug_pm(rvc_engine *e, const float *audio, int B, int n, int frame, int Tm, int *cand_n, float *cand_f, float *cand_s, float *cand_delta, int *path_out, float *f0_out)
{
    return (int)guarded(e, [&]() {
        if (B < 1 || B > 64 || Tm < 1 || Tm > 1024 || !cand_n || !cand_f || !cand_delta || (!path_out) != (!f0_out)) throw ShapeError("pm: B in [1, 64], Tm in [1, 1024], candidate arrays");
        if (audio && (!cand_s || n < 1 || frame < 1 || frame > n || Tm != 1 + frame / 160)) throw ShapeError("pm: frame in [1, n], Tm = 1 + frame / 160");
        if (!audio && !path_out) throw ShapeError("pm: nothing to do");
        const size_t bt = (size_t)B * Tm, nc = bt * 15;
        DevBuf<float> d_audio, d_rw, d_gpk, d_f, d_s, d_d, d_f0; DevBuf<int> d_n, d_path;
        d_n.alloc(bt); d_f.alloc(nc); d_s.alloc(nc); d_d.alloc(nc); d_path.alloc(bt); d_f0.alloc(bt);
        if (audio) {
            const std::vector<float> rw = pm_rw_table();
            d_audio.alloc((size_t)B * n); d_rw.alloc(rw.size()); d_gpk.alloc((size_t)B * 2);
            HIPCHK(hipMemcpy(d_audio.get(), audio, (size_t)B * n * sizeof(float), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d_rw.get(), rw.data(), rw.size() * sizeof(float), hipMemcpyHostToDevice));
        } else {
            HIPCHK(hipMemcpy(d_n.get(), cand_n, bt * sizeof(int), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d_f.get(), cand_f, nc * sizeof(float), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d_d.get(), cand_delta, nc * sizeof(float), hipMemcpyHostToDevice));
        }
        HIPCHK(hipDeviceSynchronize());
        if (audio) launch_pm_cand(e->stream, B, d_audio.get(), n, n, frame, Tm, d_rw.get(), d_gpk.get(), d_n.get(), d_f.get(), d_s.get(), d_d.get());
        if (path_out) launch_pm_path(e->stream, B, Tm, d_n.get(), d_f.get(), d_d.get(), d_path.get(), d_f0.get());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(e->stream));
        if (audio) {
            HIPCHK(hipMemcpy(cand_n, d_n.get(), bt * sizeof(int), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(cand_f, d_f.get(), nc * sizeof(float), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(cand_s, d_s.get(), nc * sizeof(float), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(cand_delta, d_d.get(), nc * sizeof(float), hipMemcpyDeviceToHost));
        }
        if (path_out) {
            HIPCHK(hipMemcpy(path_out, d_path.get(), bt * sizeof(int), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(f0_out, d_f0.get(), bt * sizeof(float), hipMemcpyDeviceToHost));
        }
        return RVC_OK;
    });
}

// test aid: the kernels of "f0 from outside" alone (f0_override.hip.h; tests/test_gpu_f0_override.py), through the launches the engine uses (include/rvc_mi355x_debug.h)
int rvc_debug_f0_override(rvc_engine *e, int op, const float *rows, int B, int Tm, const float *ov, const int *ov_n, const long long *geo, const double *t, int n_bp, float *out)
{
    return (int)guarded(e, [&]() {
        if (op < 0 || op > 3 || !out || !ov) throw ShapeError("f0 override: op in [0, 3], arrays");
        const long long LIM = 1LL << 24;
        hipStream_t st = e->stream;
        if (op == 2) {
            if (!t || !geo || n_bp < 1 || n_bp > LIM || geo[0] < 1 || geo[0] > LIM) throw ShapeError("f0 override: breakpoints in [1, 2^24], Nf in [1, 2^24]");
            const size_t Nf = (size_t)geo[0];
            DevBuf<double> d_t; DevBuf<float> d_hz, d_g;
            d_t.alloc((size_t)n_bp); d_hz.alloc((size_t)n_bp); d_g.alloc(Nf);
            HIPCHK(hipMemcpy(d_t.get(), t, (size_t)n_bp * sizeof(double), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d_hz.get(), ov, (size_t)n_bp * sizeof(float), hipMemcpyHostToDevice));
            launch_f0_curve_grid(st, d_t.get(), d_hz.get(), n_bp, d_g.get(), (long long)Nf);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipMemcpy(out, d_g.get(), Nf * sizeof(float), hipMemcpyDeviceToHost));
            return RVC_OK;
        }
        if (!rows || B < 1 || B > 64 || Tm < 1 || Tm > F0_OV_ROWS) throw ShapeError("f0 override: B in [1, 64], Tm in [1, 1024]");
        const size_t bt = (size_t)B * Tm;
        DevBuf<float> d_rows, d_out, d_ov; DevBuf<int> d_cnt; DevBuf<F0OvCall> d_call;
        d_rows.alloc(bt);
        HIPCHK(hipMemcpy(d_rows.get(), rows, bt * sizeof(float), hipMemcpyHostToDevice));
        F0OvCall call{};
        if (op == 0) {
            if (!ov_n) throw ShapeError("f0 override: counts");
            for (int b = 0; b < B; b++) if (ov_n[b] < 0 || ov_n[b] > Tm) throw ShapeError("f0 override: a count outside [0, Tm]");
            d_ov.alloc((size_t)B * F0_OV_ROWS); d_cnt.alloc((size_t)B);
            HIPCHK(hipMemcpy(d_ov.get(), ov, (size_t)B * F0_OV_ROWS * sizeof(float), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d_cnt.get(), ov_n, (size_t)B * sizeof(int), hipMemcpyHostToDevice));
        } else {
            if (!geo || geo[0] < 1 || geo[0] > LIM || geo[1] < 0 || geo[1] > LIM || geo[2] < 0 || geo[2] > B || geo[3] < 1 || geo[3] > F0_OV_ROWS || geo[4] < 0 || geo[4] > F0_OV_ROWS)
                throw ShapeError("f0 override: geometry {Nf, w0, nw, H, C}");
            if (op == 3 && geo[4] + geo[3] > Tm) throw ShapeError("f0 override: the hop [C, C + H) lies outside the window");
            const size_t Nf = (size_t)geo[0];
            d_ov.alloc(Nf);
            HIPCHK(hipMemcpy(d_ov.get(), op == 1 ? ov : out, Nf * sizeof(float), hipMemcpyHostToDevice));
            call = F0OvCall{d_ov.get(), (long long)Nf, 1, (int)geo[1], (int)geo[2], (int)geo[3], (int)geo[4], 0};
        }
        if (op == 3) {
            launch_f0_export(st, d_rows.get(), Tm, (int)geo[1], (int)geo[2], (int)geo[3], (int)geo[4], d_ov.get(), geo[0]);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipMemcpy(out, d_ov.get(), (size_t)geo[0] * sizeof(float), hipMemcpyDeviceToHost));
            return RVC_OK;
        }
        d_out.alloc(bt); d_call.alloc(1);
        HIPCHK(hipMemcpy(d_call.get(), &call, sizeof call, hipMemcpyHostToDevice));
        launch_f0_override(st, B, Tm, d_rows.get(), d_out.get(), d_call.get(), d_cnt.get(), d_ov.get(), nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(out, d_out.get(), bt * sizeof(float), hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

// test aid: the caller-side post-processing, the session's ring updates and a converter of several streams (chunk.hip.h, session.hip.h, resample.hip.h;
// tests/test_gpu_post.py) on the caller's arrays with the caller's stream strides, each launch queued as the session queues it (engine_int.h launch_post_* /
// launch_ring_* / launch_resampler).  Every size is checked against the strides on the host before anything is queued.
int rvc_debug_post(rvc_engine *e, const rvc_debug_post_spec *s, float *const *buf, const float *mix_power, int *offsets)
{
    return (int)guarded(e, [&]() {
        if (!s || !buf) throw ShapeError("post spec");
        const int B = s->streams, op = s->op;
        const long long LIM = 1ll << 22;
        auto in = [](long long v, long long lo, long long hi) { return v >= lo && v <= hi; };
        if (op < 0 || op > 4 || !in(B, 1, 64)) throw ShapeError("post spec");
        Plan pl; pl.key.B = B;
        Arena &A = pl.arena;
        A.set_chunk_min((size_t)1 << 20);
        // the buffers of the op: floats per buffer (0 = unused); each is the whole allocation, uploaded before the launches and downloaded after them
        long long size[4] = {0, 0, 0, 0};
        float *d[4] = {nullptr, nullptr, nullptr, nullptr};
        auto alloc_all = [&]() {
            for (int j = 0; j < 4; j++) if (size[j] > 0) {
                if (!buf[j]) throw ShapeError("post buffers");
                d[j] = A.floats((size_t)size[j]);
                HIPCHK(hipMemcpy(d[j], buf[j], (size_t)size[j] * 4, hipMemcpyHostToDevice));
            }
        };
        struct Conv { rvc_resampler *r = nullptr; ~Conv() { rvc_resampler_destroy(r); } } conv;
        int *d_off = nullptr; double *d_trk = nullptr; size_t n_trk = 0;
        if (op == 0) {
            const int n = s->n, frame = s->frame, hop = s->hop;
            if (!in(n, 1, LIM) || !in(frame, 1, 1 << 16) || !in(hop, 1, 1 << 16) || !mix_power) throw ShapeError("post spec: envelope sizes");
            const int nf = (n + 2 * (frame / 2) - frame) / hop + 1;
            if (!in(s->in_bs, n, LIM) || !in(s->out_bs, n, LIM) || !in(s->r_bs, 2LL * nf, LIM)) throw ShapeError("post spec: a stride is smaller than its row");
            size[0] = B * s->in_bs; size[1] = B * s->out_bs;
            alloc_all();
            if (!buf[2]) throw ShapeError("post buffers");
            // the tracks are f64 on the device: the caller's floats go up widened and come back rounded (the padding is exact either way)
            n_trk = (size_t)(B * s->r_bs);
            std::vector<double> trk(buf[2], buf[2] + n_trk);
            d_trk = A.upload(trk);
            const float *d_mp = A.upload(std::vector<float>(mix_power, mix_power + B));
            float *x = d[0], *y = d[1]; double *r = d_trk;
            const long long in_bs = s->in_bs, out_bs = s->out_bs, r_bs = s->r_bs;
            pl.ops.push_back([=](hipStream_t st) { launch_post_rms(st, B, x, n, frame, hop, nf, r, in_bs, r_bs); });
            pl.ops.push_back([=](hipStream_t st) { launch_post_rms(st, B, y, n, frame, hop, nf, r + nf, out_bs, r_bs); });
            pl.ops.push_back([=](hipStream_t st) { launch_post_mix(st, B, y, n, r, nf, r + nf, nf, 0.f, out_bs, r_bs, d_mp); });
        } else if (op == 1) {
            const int n = s->sola_len, search = s->search, frame = s->frame;
            if (!in(search, 0, 1023)) throw ShapeError("post spec: sola search range too long");
            if (!in(n, 1, 1 << 16) || !in(frame, 1, LIM) || !offsets) throw ShapeError("post spec: sola sizes");
            if (!in(s->out_bs, (long long)search + frame + n, LIM) || !in(s->sola_bs, n, LIM) || !in(s->frame_bs, frame, LIM) || !in(s->cor_bs, search + 1, LIM))
                throw ShapeError("post spec: a stride is smaller than its row");
            size[0] = B * s->out_bs; size[1] = B * s->sola_bs; size[2] = B * s->frame_bs; size[3] = B * s->cor_bs;
            alloc_all();
            d_off = (int *)A.alloc((size_t)B * 4);
            float *o = d[0], *sb = d[1], *fr = d[2], *cor = d[3];
            const long long out_bs = s->out_bs, sola_bs = s->sola_bs, frame_bs = s->frame_bs, cor_bs = s->cor_bs;
            pl.ops.push_back([=](hipStream_t st) { launch_post_sola_corr(st, B, o, sb, n, search, cor, out_bs, sola_bs, cor_bs); });
            pl.ops.push_back([=](hipStream_t st) { launch_post_sola(st, B, o, sb, n, search, frame, fr, d_off, cor, out_bs, sola_bs, frame_bs, cor_bs, nullptr, 0, nullptr, 0LL); });
        } else if (op == 2 || op == 3) {
            const int n = s->n, f = s->f, skip = s->skip, cb = s->copy_begin;
            if (!in(n, 1, LIM) || !in(f, 1, n)) throw ShapeError("post spec: ring sizes");
            size[0] = size[1] = (long long)B * n;
            if (op == 2) {
                size[2] = (long long)B * f;
                alloc_all();
                const float *ri = d[0], *ch = d[2]; float *ro = d[1];
                pl.ops.push_back([=](hipStream_t st) { launch_ring_shift_append(st, B, ri, ro, n, f, ch); });
            } else {
                // samples in front of copy_begin come from in[i + f]; [copy_begin, n) from res[skip ..]
                if (!in(skip, 0, LIM) || !in(cb, 0, n - f)) throw ShapeError("post spec: ring sizes");
                if (!in(s->x_bs, (long long)skip + n - cb, LIM)) throw ShapeError("post spec: a stride is smaller than its row");
                size[2] = B * s->x_bs;
                alloc_all();
                const float *ri = d[0], *res = d[2]; float *ro = d[1];
                const long long res_bs = s->x_bs;
                pl.ops.push_back([=](hipStream_t st) { launch_ring16_update(st, B, ri, ro, n, f, res, skip, cb, res_bs); });
            }
        } else {
            const int chunks = s->chunks;
            if (!in(s->rate_in, 1, 1 << 20) || !in(s->rate_out, 1, 1 << 20) || !in(s->chunk, 1, 1 << 16) || !in(chunks, 1, 16)) throw ShapeError("post spec: converter sizes");
            int fi = 0, fo = 0;
            const rvc_status rc = resampler_create_streams(e, (size_t)s->rate_in, (size_t)s->rate_out, (size_t)s->chunk, B, &conv.r, &fi, &fo);
            if (rc != RVC_OK) return rc;
            if (!in(s->x_bs, fi, LIM) || !in(s->out_bs, fo, LIM)) throw ShapeError("post spec: a stride is smaller than its row");
            size[0] = (long long)chunks * B * s->x_bs; size[1] = (long long)chunks * B * s->out_bs;
            alloc_all();
            rvc_resampler *r = conv.r;
            const long long x_bs = s->x_bs, out_bs = s->out_bs;
            for (int c = 0; c < chunks; c++) {
                const float *x = d[0] + (long long)c * B * x_bs; float *y = d[1] + (long long)c * B * out_bs;
                pl.ops.push_back([=](hipStream_t) { launch_resampler(r, x, y, x_bs, out_bs); });
            }
        }
        run_ops(e, pl, 1, s->graph != 0);
        for (int j = 0; j < 4; j++) if (size[j] > 0) HIPCHK(hipMemcpy(buf[j], d[j], (size_t)size[j] * 4, hipMemcpyDeviceToHost));
        if (d_trk) {
            std::vector<double> trk(n_trk);
            HIPCHK(hipMemcpy(trk.data(), d_trk, n_trk * 8, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n_trk; i++) buf[2][i] = (float)trk[i];
        }
        if (d_off) HIPCHK(hipMemcpy(offsets, d_off, (size_t)B * 4, hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

// test aid: one ConvBlockRes of RMVPE as build_rmvpe queues it -- rm_block_kernel when the block is eligible, else the implicit-GEMM launches, with the poolings
// folded into the block or queued as launches of their own by the model's own dry runs (include/rvc_mi355x_debug.h, tests/test_gpu_rmblock.py).  As for
// rvc_debug_layer, the caller owns every float of the tensors' allocations.
int rvc_debug_rm_block(rvc_engine *e, const rvc_debug_rm_block_spec *s, const float *w1, const float *b1, const float *w2, const float *b2, const float *wsc,
                       const float *bsc, float *x, float *y, float *p, long long *geo)
{
    return (int)guarded(e, [&]() {
        if (!s || !geo || s->streams < 1 || s->streams > 64 || s->cin < 1 || s->cin > 1024 || s->cout < 1 || s->cout > 1024 || s->H < 1 || s->H > 1024 || s->W < 1 ||
            s->W > 1024 || s->reps < 1 || (s->pool_out && (s->H < 2 || s->W < 2)))
            throw ShapeError("rm block spec");
        const int B = s->streams, ci = s->cin, co = s->cout, H = s->H, W = s->W;
        Plan pl; pl.key.B = B; pl.rm_fuse = s->rm_fuse != 0;
        DebugWeights wts;
        Arena &A = pl.arena;
        const T2 src = s->pool_in ? make_t2(A, B, ci, 2 * H, 2 * W) : make_t2(A, B, ci, H, W);
        const T2 ybuf = make_t2(A, B, s->y_in_cat ? 2 * co : co, H, W), out = s->y_in_cat ? ybuf.chans(co, co) : ybuf;
        T2 pooled;
        if (s->pool_out) pooled = make_t2(A, B, co, H / 2, W / 2);
        const DebugGeo gx = debug_geo2(src), gy = debug_geo2(ybuf), gp = s->pool_out ? debug_geo2(pooled) : DebugGeo();
        for (int i = 0; i < 8; i++) { geo[i] = gx.g[i]; geo[8 + i] = gy.g[i]; geo[16 + i] = gp.base ? gp.g[i] : 0; }
        if (!x) return RVC_OK;
        if (!y || !w1 || !b1 || !w2 || !b2 || (s->pool_out && !p) || (wsc && !bsc) || (!wsc && ci != co)) throw ShapeError("rm block buffers");
        const ResBlockW &w = wts.block(make_res_block(w1, b1, w2, b2, wsc, bsc, ci, co));
        const ResBlockW *next = s->next ? &wts.block(make_res_block(w1, b1, w2, b2, wsc, bsc, ci, co)) : nullptr;
        // the poolings, decided as build_rmvpe decides them: a dry run of the fused block with the pooled input / the pooled second output
        const int hook = test_opt_int("RVC_RM_FUSE", 1);
        T2 xin = src; const T2 *pool_src = nullptr;
        if (s->pool_in) {
            xin = make_t2(A, B, ci, H, W);          // (the block pools while it stages: only the geometry of this tensor is used)
            if (hook != 3 && add_rm_block_fused(pl, w, xin, out, nullptr, &src, true)) pool_src = &src;
            else add_avgpool2(pl, src, xin);
        }
        const bool by_block = s->pool_out && hook != 3 && add_rm_block_fused(pl, w, xin, out, nullptr, pool_src, true, &pooled);
        add_res_block(pl, w, xin, out, next, pool_src, by_block ? &pooled : nullptr);
        if (s->pool_out && !by_block) add_avgpool2(pl, out, pooled);
        gx.upload(x); gy.upload(y); gp.upload(p);
        run_ops(e, pl, s->reps, s->graph != 0);
        gx.download(x); gy.download(y); gp.download(p);
        return RVC_OK;
    });
}

// test aid: the retrieval section of an infer plan alone (retrieval.hip build_retrieval; tests/test_gpu_knn.py) on the caller's arrays with the caller's leading
// dimensions.  The streams' states are a block of the aid's own (the one-launch form raises ST_KNN_TIMEOUT there), the engine's index rate is the spec's for
// the duration of the call.
int rvc_debug_retrieval(rvc_engine *e, const rvc_debug_retrieval_spec *s, float *cv, float *phone, int *idx, float *dist, int *overflow)
{
    return (int)guarded(e, [&]() {
        if (!s || !cv || !phone || !idx || !dist || !overflow) throw ShapeError("retrieval spec");
        const int B = s->streams, C = s->C, T = s->T, R = s->R;
        if (B < 1 || B > 4096 || C < 1 || C > 4096 || R < 1 || R > 4096 || T < 1 || T > (1 << 20) || s->skip_head < 0 || s->ph_ld < R || s->cv_ld < T || s->ph_ld > (1 << 20) ||
            s->cv_ld > (1 << 21) || (long long)s->skip_head + R > 2LL * T + 1 || s->reps < 1 || s->reps > 64 || s->path < 0 || s->path > 1 || !(s->rate >= 0.f && s->rate <= 1.f))
            throw ShapeError("retrieval spec");
        if (!e->index.rows) throw ShapeError("no index loaded");
        if (e->index.dim != (size_t)C) throw ShapeError("index dimension does not match the feature dimension");
        Plan pl; pl.key.B = B; pl.key.nprobe = e->index_nprobe; pl.key.knn_k = e->index_k;
        Arena &A = pl.arena;
        const size_t n_ph = (size_t)B * C * s->ph_ld, n_cv = (size_t)B * C * s->cv_ld, n_hit = (size_t)B * R * pl.key.knn_k;
        T1 cvo, ph;
        cvo.p = A.floats(n_cv); cvo.B = B; cvo.C = C; cvo.T = T; cvo.ld = s->cv_ld; cvo.halo = 0; cvo.bs = (long long)C * s->cv_ld;
        ph.p = A.floats(n_ph); ph.B = B; ph.C = C; ph.T = R; ph.ld = s->ph_ld; ph.halo = 0; ph.bs = (long long)C * s->ph_ld;
        pl.cv_out = cvo;
        std::vector<StreamState> hst(B);
        for (int b = 0; b < B; b++) { memset(&hst[b], 0, sizeof(StreamState)); hst[b].ctl.protect = (float)PROTECT_OFF; }
        StreamState *d_st = A.upload(hst);
        // the plan is built against the aid's states and rate; the engine gets its own back on every exit
        struct Swap {
            rvc_engine *e; StreamState *st; int n; float rate;
            Swap(rvc_engine *e_, StreamState *s_, int B_, float r_) : e(e_), st(e_->d_state), n(e_->n_streams), rate(e_->index_rate) { e->d_state = s_; e->n_streams = B_; e->index_rate = r_; }
            ~Swap() { e->d_state = st; e->n_streams = n; e->index_rate = rate; }
        } swap_guard(e, d_st, B, s->rate);
        build_retrieval(e, pl, B, T, C, (uint32_t)s->skip_head, (uint32_t)R, ph);
        if (s->path == 1) {
            if (pl.key.nprobe > 0) throw ShapeError("the IVF retrieval has no exhaustive list");
            if (pl.knn_fallback.empty()) throw ShapeError("this plan has no fallback list");
            pl.ops = OpList();
            for (Op &o : pl.knn_fallback) pl.ops.push_back(o);
            snprintf(g_last_kernel, sizeof g_last_kernel, "knn_fallback");
        }
        HIPCHK(hipMemcpy(cvo.p, cv, n_cv * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ph.p, phone, n_ph * 4, hipMemcpyHostToDevice));
        run_ops(e, pl, s->reps, s->graph != 0);
        HIPCHK(hipMemcpy(cv, cvo.p, n_cv * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(phone, ph.p, n_ph * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(idx, pl.d_knn_idx, n_hit * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dist, pl.d_knn_dist, n_hit * sizeof(float), hipMemcpyDeviceToHost));
        memset(overflow, 0, (size_t)B * sizeof(int));
        if (pl.d_knn_overflow && s->path == 0) HIPCHK(hipMemcpy(overflow, pl.d_knn_overflow, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hst.data(), d_st, sizeof(StreamState) * B, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; b++) if (hst[b].status != 0) throw std::runtime_error("retrieval raised a stream's status word");
        if (pl.knn_ticket && s->path == 0) {
            std::vector<unsigned> tk(pl.knn_ticket_bytes / sizeof(unsigned));
            HIPCHK(hipMemcpy(tk.data(), pl.knn_ticket, pl.knn_ticket_bytes, hipMemcpyDeviceToHost));
            for (unsigned v : tk) if (v != 0) throw std::runtime_error("the one-launch retrieval left its ticket words non-zero");
        }
        return RVC_OK;
    });
}

// test aid: which copies of the index exist (a fallback list built while the transposed copy is absent walks the row-major matrix)
int rvc_debug_index_layouts(rvc_engine *e) { return e ? (e->index.rowsF ? 1 : 0) | (e->index.rowsT ? 2 : 0) | (e->index.ivf.cent ? 4 : 0) : 0; }

// test aids of the run-time speaker selection (model_synth.hip, speaker.hip.h; tests/test_gpu_speaker.py): the live folded biases, read only, and the
// duration of the last fold queued under rvc_set_profile
int rvc_debug_speaker_biases(rvc_engine *e, int composed, float *out, size_t cap, size_t *n)
{
    return (int)guarded(e, [&]() {
        if (!e->sy) return RVC_MODEL_NOT_LOADED;
        std::vector<float> v;
        e->sy->speaker_biases(composed != 0, v);
        if (n) *n = v.size();
        if (!out || cap < v.size()) return RVC_SHAPE;
        memcpy(out, v.data(), v.size() * sizeof(float));
        return RVC_OK;
    });
}
float rvc_debug_speaker_fold_ms(rvc_engine *e)
{
    float ms = -1.f;
    (void)guarded(e, [&]() {
        if (!e->sy || !e->sy->spk_prof_valid) return RVC_OK;
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipEventElapsedTime(&ms, e->sy->spk_prof[0], e->sy->spk_prof[1]));
        return RVC_OK;
    });
    return ms;
}

// test aid: one assign step and one update step of the k-means training (retrieval.hip kmeans_assign_step / kmeans_update_step; tests/test_gpu_kmeans.py)
int rvc_debug_kmeans_step(rvc_engine *e, const float *centroids_in, size_t nlist, const int32_t *prev_assign_or_null, int32_t *assign_out, float *dist_out,
                          float *centroids_out, double *objective_out, long long *moved_out)
{
    return (int)guarded(e, [&]() {
        if (!centroids_in || !assign_out || !dist_out || !centroids_out || !objective_out || !moved_out) throw ShapeError("k-means step: null argument");
        if (!e->index.rows) throw ShapeError("no index loaded");
        const size_t n = e->index.n, dim = e->index.dim;
        if (nlist < 1 || nlist > n || nlist > 65536) throw ShapeError("k-means step: nlist must be in [1, min(n, 65536)]");
        HIPCHK(hipDeviceSynchronize());
        KmeansWork w;
        w.alloc(n, dim, nlist);
        HIPCHK(hipMemcpy(w.cent.get(), centroids_in, nlist * dim * sizeof(float), hipMemcpyHostToDevice));
        if (prev_assign_or_null) HIPCHK(hipMemcpy(w.assign[1].get(), prev_assign_or_null, n * sizeof(int), hipMemcpyHostToDevice));
        kmeans_assign_step(e, w, prev_assign_or_null ? w.assign[1].get() : nullptr, 0, objective_out, moved_out);
        HIPCHK(hipMemcpy(assign_out, w.assign[0].get(), n * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dist_out, w.dist.get(), n * sizeof(float), hipMemcpyDeviceToHost));
        kmeans_update_step(e, w, 0);
        HIPCHK(hipMemcpy(centroids_out, w.cent.get(), nlist * dim * sizeof(float), hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

// test aid: one append of the index builder (retrieval.hip index_build_reserve / index_build_append; tests/test_gpu_index_build.py) on a store of its own
int rvc_debug_index_append(rvc_engine *e, const float *cv, int C, int T, int ld, size_t cursor, size_t capacity, const float *head_rows, float *store_out,
                           size_t cap_rows, size_t *rows_out, size_t *dropped_out)
{
    return (int)guarded(e, [&]() {
        if (!cv || !store_out || !rows_out || !dropped_out || (cursor && !head_rows)) throw ShapeError("index append: null argument");
        if (C < 1 || T < 1 || ld < T || capacity < 1 || cursor > capacity) throw ShapeError("index append: needs C >= 1, 1 <= T <= ld, cursor <= capacity, capacity >= 1");
        if (cap_rows < cursor + (size_t)T) throw ShapeError("index append: store_out holds fewer than cursor + T rows");
        HIPCHK(hipDeviceSynchronize());
        IndexBuild b;
        b.alloc((size_t)C, capacity);
        DevBuf<float> d_cv; d_cv.alloc((size_t)C * ld);
        HIPCHK(hipMemcpy(d_cv.get(), cv, (size_t)C * ld * sizeof(float), hipMemcpyHostToDevice));
        if (cursor) HIPCHK(hipMemcpy(b.store.get(), head_rows, cursor * C * sizeof(float), hipMemcpyHostToDevice));
        const int cnt0[2] = {(int)cursor, 0};
        HIPCHK(hipMemcpy(b.d_cnt.get(), cnt0, sizeof cnt0, hipMemcpyHostToDevice));
        index_build_reserve(e, b, cursor, cursor + (size_t)T);
        index_build_append(e, b, d_cv.get(), C, T, ld);
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipGetLastError());
        int cnt[2] = {0, 0};
        HIPCHK(hipMemcpy(cnt, b.d_cnt.get(), sizeof cnt, hipMemcpyDeviceToHost));
        if (cnt[0] < (int)cursor || (size_t)cnt[0] > cursor + (size_t)T) throw std::runtime_error("index append: the device-side row count is out of range");
        HIPCHK(hipMemcpy(store_out, b.store.get(), (size_t)cnt[0] * C * sizeof(float), hipMemcpyDeviceToHost));
        *rows_out = (size_t)cnt[0]; *dropped_out = (size_t)cnt[1];
        return RVC_OK;
    });
}

// the kernel family of the most recently queued implicit-GEMM launch (the first word of its description), the variant of the last op or the form of the
// last ConvBlockRes: tests assert which path they exercised
const char *rvc_debug_last_kernel(void)
{
    static thread_local std::string buf;
    buf = g_last_kernel;
    return buf.c_str();
}

// the whole description of this thread's most recently queued implicit-GEMM launch (what rvc_debug_profile_dump prints per launch): tests read the fields
// after the family, e.g. "split=2" for the two-stage grid-level split-K
const char *rvc_debug_last_desc(void)
{
    static thread_local std::string buf;
    buf = g_last_desc;
    return buf.c_str();
}

// test aid: launches (ops) of the last call's plan
int rvc_debug_last_plan(rvc_engine *e, int *n_ops)
{
    if (!e || !e->last_plan) return 0;
    int n = 0;
    for (size_t i = 0; i < e->last_plan->ops.v.size(); i++) if (e->last_plan->ops.kind[i] == 0) n++;
    if (n_ops) *n_ops = n;
    return 1;
}

// tuning aid: one line per profiled launch of the last call: "<us> <gflop> <description>"
int rvc_debug_profile_dump(rvc_engine *e, char *buf, size_t cap)
{
    if (!e || !e->last_plan) return 0;
    Plan &pl = *e->last_plan;
    if (hipDeviceSynchronize() != hipSuccess) return 0;
    std::string out;
    for (size_t i = 0; i < pl.prof_used; i++) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, pl.prof[i].a, pl.prof[i].b) != hipSuccess) continue;
        char ln[320];
        snprintf(ln, sizeof ln, "%.2f %.4f %s\n", t * 1e3, pl.prof[i].flops * 1e-9, pl.prof[i].desc >= 0 ? pl.descs[pl.prof[i].desc].c_str() : (pl.prof[i].name ? pl.prof[i].name : "?"));
        out += ln;
    }
    if (out.size() + 1 > cap) return -1;
    memcpy(buf, out.c_str(), out.size() + 1);
    return (int)pl.prof_used;
}

}  // extern "C"
