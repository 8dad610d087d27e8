// convert.hip.h -- conversion of whole recordings (DESIGN.md sections 19 and 29; upstream's "model inference" tab, vc_single and vc_multi), included by
// convert_many.hip.h (engine.hip's unit).
//
// The recordings of a call are cut into windows of ONE geometry (convert_geometry.h), so one plan serves the whole call; the windows are laid end to end
// (convert_many_geometry.h: global window g = P_f + w) and run S at a time through infer_common on the engine's S streams, so a batch may hold the windows of
// several files and only the last batch of the CALL is padded.  They are stitched by the plugin's SOLA step in its LINEAR crossfade, one offset chain per file,
// on the device (stitch.hip.h).  In front of it the optional 48 Hz high-pass (highpass.hip.h) and the silence gate (silence.hip.h).  Per batch: one gather
// launch, one infer call with its one synchronisation, two stitch launches; the signals, S window inputs, S window outputs, the tails and the outputs stay in
// HBM.  convert_windows_run is the one driver: rvc_convert* is its call of one file (convert_run), rvc_convert_many (convert_many.hip.h) its call of many.
// f0_analyze.hip.h / f0_analyze_many.hip.h: the same windows through the pitch-only plan, order statistics of f0 rows, and the two auto-transposes.
#pragma once
#include "convert_geometry.h"
#include "stitch.hip.h"
#include "resample_whole.hip.h"
#include "change_rms.hip.h"
#include "f0_analyze_many.hip.h"

namespace rvc {

// the statuses of a call that runs the models, as rvc_infer's: before any argument is looked at
static rvc_status convert_loaded(rvc_engine *e)
{
    if (!e->sy) return RVC_MODEL_NOT_LOADED;
    if (!e->cv) return RVC_CONTENTVEC_NOT_LOADED;
    if (!e->f0_method && e->sy->has_f0) return RVC_F0_NOT_LOADED;
    return RVC_OK;
}

// the shape checks of a conversion of n samples at 16 kHz; fills the geometry
static void convert_shape(rvc_engine *e, size_t n, size_t k, size_t context, size_t crossfade, ConvertGeometry *g)
{
    if (n == 0) throw ShapeError("convert: empty recording");
    if (e->sy->sr <= 0 || e->sy->sr % 100 != 0) throw ShapeError("convert: the synthesizer's sample rate is not a multiple of 100");
    if (const char *why = convert_geometry(n, (size_t)e->sy->sr, k, context, crossfade, g)) throw ShapeError(why);
    if (g->windows > (size_t)1 << 30 || g->out_samples > (size_t)1 << 40) throw ShapeError("convert: recording too long");
}

// statuses and arguments of rvc_convert / rvc_convert_device, in the order the header documents; fills the geometry and *out_len
static rvc_status convert_check(rvc_engine *e, const void *pcm, size_t n, size_t k, size_t context, size_t crossfade, const void *out, size_t cap, size_t *out_len, ConvertGeometry *g)
{
    const rvc_status rc = convert_loaded(e);
    if (rc != RVC_OK) return rc;
    convert_shape(e, n, k, context, crossfade, g);
    if (out_len) *out_len = g->out_samples;
    if (cap < g->out_samples) { e->err = "convert: output buffer too small"; return RVC_SHAPE; }
    if (!pcm || !out) throw ShapeError("convert: null buffer");
    return RVC_OK;
}

// what a caller takes of the driver's optional parts
struct ConvertCall {
    const char *who;                      // the entry point's name in the refusals
    rvc_engine::ConvertInfo *info;        // the info block the call reports to: e->conv or e->many
    bool single;                          // one recording (rvc_convert*): the f0 curve, the engine-wide auto-transpose and the f0 export to e->conv_f0 apply;
                                          // else (rvc_convert_many) the per-file factors do
    DevBuf<float> *keep_filtered;         // (rvc_convert_file) the high-passed signal is handed to the caller instead of being freed; or null
};

// The conversion proper, device to device: d_sig = the signal arena of the call, tabs its tables, d_out the output arena.  Begins with what rvc_reset_state does
// (pitch caches and chunk counters zeroed), so that a window's result depends on the recording alone; every per-stream setting, the index, the f0 method and
// graph replay apply as to any infer call.  The callers hold the guards that take the call's settings (curve gather, auto_mul, many_mul) off the engine again
static rvc_status convert_windows_run(rvc_engine *e, const float *d_sig, const ConvertManyGeometry &m, const ManyTables &tabs, int32_t pitch_shift, bool highpass, float *d_out,
                                      const ConvertCall &call)
{
    hipStream_t st = e->stream;
    const ConvertGeometry &g = m.g;
    const size_t F = m.files(), S = (size_t)e->n_streams, W = m.windows_total();
    size_t batches = m.batches(S);
    const size_t sola_len = g.X * g.zc, search = g.Q * g.zc, frame = g.H * g.zc, ylen = g.return_length * g.zc;
    const bool gated = silence_gate_on(e);
    e->conv.valid = false; e->conv_f0_valid = false; call.info->valid = false;
    HIPCHK(hipDeviceSynchronize());
    reset_state(e);          // (pending f0 overrides of the streams go with it: a conversion uses the curve alone)
    // one recording, f0 from outside: the curve's grid is built once; each batch's plan gathers from it, and the conditioned rows of each
    // window's hop [Cg, Cg + H) go back onto the grid for rvc_convert_f0 (analyze_cg: Cg and its centring check)
    const bool single_f0 = call.single && e->sy->has_f0;
    const int Cg = single_f0 ? analyze_cg(g, call.who) : 0;
    const bool curve = single_f0 && e->curve_n > 0;
    DevBuf<float> f0grid;
    bool export_ok = single_f0;
    if (single_f0) f0grid.alloc(g.Nf);
    if (curve) {
        e->curve_grid.alloc(g.Nf);
        launch_f0_curve_grid(st, e->curve_t.get(), e->curve_hz.get(), (int)e->curve_n, e->curve_grid.get(), (long long)g.Nf);
        e->conv_curve = true;
    }
    DevTimer t_total, t_hp;
    t_total.start(st);
    DevBuf<float> filtered;
    const float *sig = d_sig;
    if (highpass) {
        filtered.alloc(m.sig_total());
        t_hp.start(st);
        many_highpass(e, d_sig, m, filtered.get());
        t_hp.stop(st);
        sig = filtered.get();
    }
    // the silence gate (silence.hip.h): with a threshold set, the signals the model will see are measured first, every file on its own, the
    // active windows of all files are compacted in global window order and only they run; a skipped window enters the stitch as zeros.  Off (the default):
    // nothing is queued here and the loop below is the ungated one
    SilenceWork work;
    const SilenceWork *gate = gated ? &work : nullptr;
    if (gated) {
        many_gate(st, sig, m, e->sil_db, e->sil_hang, ylen, &work);
        batches = work.batches(S);
        if (single_f0) HIPCHK(hipMemsetAsync(f0grid.get(), 0, g.Nf * sizeof(float), st));      // (the rows of skipped windows are 0)
    }
    // the pitch of the call, from the f0 of the signals the model will see -- the call's own windows through the pitch-only plan (the gate's active ones when it
    // is on).  One recording with a target set: the curve merged in, 12 log2(target / median) semitones become one more factor of every
    // stream's multiplier until the call returns.  Many recordings with a per-file setting (section 31): file_mul[f] = (float)2^(t_f / 12), 0 = none, and every
    // stream takes the factor of the file whose window it holds, batch by batch; under the gate that is the file of the window win_of names.  Off (the
    // default): nothing is queued here
    const bool per_file = !call.single && e->sy->has_f0 && (!e->many_semitones.empty() || e->many_at_target > 0.0);
    std::vector<float> file_mul; std::vector<int> win_of;
    if (single_f0 && e->at_target > 0.0) {
        float mul = 0.f;
        const rvc_status rc = auto_transpose_run(e, sig, m, tabs, curve ? e->curve_grid.get() : nullptr, &mul, gate);
        if (rc != RVC_OK) { (void)hipStreamSynchronize(st); return rc; }
        e->auto_mul = mul;
    }
    if (per_file) {
        const rvc_status rc = many_pitch_run(e, sig, m, tabs, gate, &file_mul);
        if (rc != RVC_OK) { (void)hipStreamSynchronize(st); return rc; }
        if (gated && work.A) { win_of.resize(work.A); HIPCHK(hipMemcpy(win_of.data(), work.win_of.get(), work.A * sizeof(int), hipMemcpyDeviceToHost)); }
    }
    DevBuf<float> win, y, tails; DevBuf<int> offs;
    win.alloc(S * g.n + 64); y.alloc(S * ylen + 64); tails.alloc((W + 1) * sola_len); offs.alloc(W);
    HIPCHK(hipMemsetAsync(win.get(), 0, (S * g.n + 64) * sizeof(float), st));
    HIPCHK(hipMemsetAsync(tails.get(), 0, sola_len * sizeof(float), st));       // row 0: every file's stitch starts from silence
    std::vector<DevEvent> ev(3 * batches);
    for (size_t b = 0; b < batches; b++) {
        // (gated: g0 is the batch's first PLACE and nw its active windows, of the A in all)
        const size_t g0 = b * S; const int nw = (int)std::min(S, (gated ? work.A : W) - g0);
        ev[3 * b].record(st);
        launch_gather_windows(st, sig, tabs, win.get(), S, gate, g0, nw, g);
        if (curve) e->conv_call = F0OvCall{e->curve_grid.get(), (long long)g.Nf, 1, (int)g0, nw, (int)g.H, Cg, 0, gated ? work.win_of.get() : nullptr};
        if (per_file) {
            e->many_mul.assign(S, 0.f);
            for (int s = 0; s < nw; s++) e->many_mul[s] = file_mul[many_file_of(m.P.data(), (int)F, gated ? win_of[g0 + s] : (int)(g0 + s))];
        }
        size_t got = 0;
        const rvc_status rc = infer_common(e, win.get(), true, g.n, g.sf, pitch_shift, (uint32_t)g.skip_head, (uint32_t)g.return_length, y.get(), true, ylen, &got, true);
        if (rc != RVC_OK) { (void)hipStreamSynchronize(st); return rc; }
        if (got != ylen) throw ShapeError(std::string(call.who) + ": the synthesizer does not produce sample_rate / 100 samples per frame");
        ev[3 * b + 1].record(st);
        if (gated) work.stitch(st, y.get(), (long long)ylen, g0, nw, tabs, (int)sola_len, (int)search, (int)frame, tails.get(), offs.get(), d_out);
        else {
            int f_first = 0, f_last = 0;
            m.batch_files(b, S, &f_first, &f_last);
            launch_stitch_many(st, y.get(), (long long)ylen, (int)g0, nw, f_first, f_last, tabs, (int)sola_len, (int)search, (int)frame, tails.get(), offs.get(), d_out);
        }
        ev[3 * b + 2].record(st);
        // the batch's conditioned f0 rows onto the grid, behind the timed sections: in ms[3] (total), in neither ms[1] (model) nor ms[2] (stitch).  The plan's rows
        // stay until the next batch's pitch tail, which this stream orders behind the launch
        if (export_ok) {
            const Plan *pl = e->last_plan;      // (streams in several formant buckets ran through several plans: no export then)
            if (pl && !pl->key.bucket && pl->d_f0 && pl->key.B == (int)S && (size_t)Cg + g.H <= (size_t)pl->Tm)
                launch_f0_export_many(st, pl->d_f0, pl->Tm, tabs, S, gate, g0, nw, (int)g.H, Cg, f0grid.get());
            else export_ok = false;
        }
    }
    // a gated call without an active window: no batch ran; the stitch walks its W windows of zeros (offsets and output as rvc_sola_stitch's on zeros)
    DevTimer t_zero;
    if (gated && batches == 0) {
        t_zero.start(st);
        work.stitch(st, y.get(), (long long)ylen, 0, 0, tabs, (int)sola_len, (int)search, (int)frame, tails.get(), offs.get(), d_out);
        t_zero.stop(st);
    }
    t_total.stop(st);
    rvc_engine::ConvertInfo &info = *call.info;
    info.offsets.assign(W, 0);
    HIPCHK(hipMemcpyAsync(info.offsets.data(), offs.get(), W * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (export_ok) { e->conv_f0.assign(g.Nf, 0.f); HIPCHK(hipMemcpyAsync(e->conv_f0.data(), f0grid.get(), g.Nf * sizeof(float), hipMemcpyDeviceToHost, st)); }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    double ms_model = 0, ms_stitch = 0;
    for (size_t b = 0; b < batches; b++) {
        float a = 0.f, c = 0.f;
        HIPCHK(hipEventElapsedTime(&a, ev[3 * b].get(), ev[3 * b + 1].get())); HIPCHK(hipEventElapsedTime(&c, ev[3 * b + 1].get(), ev[3 * b + 2].get()));
        ms_model += a; ms_stitch += c;
    }
    if (gated && batches == 0) ms_stitch = (double)t_zero.ms();
    if (gated) silence_gate_report(e, work);
    info.windows = W; info.batches = batches;
    info.ms[0] = highpass ? (double)t_hp.ms() : 0.0; info.ms[1] = ms_model; info.ms[2] = ms_stitch; info.ms[3] = (double)t_total.ms();
    info.valid = true; e->conv_f0_valid = export_ok;
    if (call.keep_filtered) *call.keep_filtered = std::move(filtered);
    return RVC_OK;
}

// one recording as the call of one file.  keep_filtered (rvc_convert_file): see ConvertCall
static rvc_status convert_run(rvc_engine *e, const float *d_pcm, size_t n, const ConvertGeometry &g, int32_t pitch_shift, bool highpass, float *d_out,
                              DevBuf<float> *keep_filtered = nullptr)
{
    const ConvertManyGeometry m = convert_many_single(g, n);
    ManyDeviceTables tabs;
    tabs.upload(m);
    struct CurveGuard { rvc_engine *e; ~CurveGuard() { e->conv_curve = false; e->ov_dirty = true; } } curve_guard{e};
    struct AutoGuard { rvc_engine *e; ~AutoGuard() { e->auto_mul = 0.f; } } auto_guard{e};
    return convert_windows_run(e, d_pcm, m, tabs.t, pitch_shift, highpass, d_out, ConvertCall{"convert", &e->conv, true, keep_filtered});
}

// peak[0] = max |x[i]| as the bits of a non-negative float (peak starts as 0; unsigned order = float order there): exact, max is order-free
static __global__ __launch_bounds__(256) void absmax_kernel(const float *x, long long n, unsigned *peak)
{
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(peak, __float_as_uint(m));
}

// what rvc_convert_file / rvc_convert_file_device check, in the order the header documents, and the sizes of every stage
struct FileGeometry {
    bool res_in = false, res_out = false;
    ResampleGeometry rin, rout;      // rate_in -> 16 000; model rate -> rate_out
    ConvertGeometry cg;
    RmsGeometry r1, r2;
    size_t n16 = 0, rate_out = 0, n_out = 0;
};
static rvc_status convert_file_check(rvc_engine *e, const void *pcm, size_t n, size_t rate_in, size_t k, size_t context, size_t crossfade, double rms_mix_rate, size_t rate_out,
                                     const void *out, size_t cap, size_t *out_len, FileGeometry *f)
{
    const rvc_status rc = convert_loaded(e);
    if (rc != RVC_OK) return rc;
    if (const char *why = resample_geometry(rate_in, 16000, n, &f->rin)) throw ShapeError(why);
    f->res_in = rate_in != 16000;
    f->n16 = f->rin.n_out;
    convert_shape(e, f->n16, k, context, crossfade, &f->cg);
    const size_t sr = (size_t)e->sy->sr;
    change_rms_check(f->n16, 16000, f->cg.out_samples, sr, rms_mix_rate, &f->r1, &f->r2);
    f->rate_out = rate_out ? rate_out : sr;
    f->res_out = f->rate_out != sr;
    if (const char *why = resample_geometry(sr, f->rate_out, f->cg.out_samples, &f->rout)) throw ShapeError(why);
    f->n_out = f->rout.n_out;
    if (out_len) *out_len = f->n_out;
    if (cap < f->n_out) { e->err = "convert_file: output buffer too small"; return RVC_SHAPE; }
    if (!pcm || !out) throw ShapeError("convert_file: null buffer");
    return RVC_OK;
}

// the chain, device to device: resample to 16 kHz, convert_run, change_rms against the signal the model saw, resample to rate_out, peak
static rvc_status convert_file_run(rvc_engine *e, const float *d_pcm, size_t n, const FileGeometry &f, int32_t pitch_shift, bool highpass, double rms_mix_rate, float *d_out)
{
    hipStream_t st = e->stream;
    e->file.valid = false;
    DevTimer t_total, t_in, t_env, t_out;
    DevBuf<float> sig16, filtered, model_out; DevBuf<double> tracks; DevBuf<unsigned> peak;
    peak.alloc(1);
    t_total.start(st);
    const float *x16 = d_pcm;
    if (f.res_in) {
        sig16.alloc(f.n16);
        t_in.start(st);
        launch_resample_whole(e, d_pcm, n, f.rin, sig16.get());
        t_in.stop(st);
        x16 = sig16.get();
    }
    float *y = d_out;      // the model's output: in place when nothing is resampled behind it
    if (f.res_out) { model_out.alloc(f.cg.out_samples); y = model_out.get(); }
    const rvc_status rc = convert_run(e, x16, f.n16, f.cg, pitch_shift, highpass, y, &filtered);
    if (rc != RVC_OK) return rc;
    const bool env = rms_mix_rate != 1.0;
    if (env) {
        t_env.start(st);
        launch_change_rms(e, highpass ? filtered.get() : x16, f.n16, f.r1, y, f.cg.out_samples, f.r2, rms_mix_rate, tracks);
        t_env.stop(st);
    }
    if (f.res_out) {
        t_out.start(st);
        launch_resample_whole(e, y, f.cg.out_samples, f.rout, d_out);
        t_out.stop(st);
    }
    HIPCHK(hipMemsetAsync(peak.get(), 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)std::min<size_t>((f.n_out + 255) / 256, 2048)), dim3(256), 0, st, (const float *)d_out, (long long)f.n_out, peak.get());
    t_total.stop(st);
    unsigned bits = 0;
    HIPCHK(hipMemcpyAsync(&bits, peak.get(), sizeof bits, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    float pk; memcpy(&pk, &bits, sizeof pk);
    e->file.ms[0] = f.res_in ? (double)t_in.ms() : 0.0;
    for (int i = 0; i < 3; i++) e->file.ms[1 + i] = e->conv.ms[i];
    e->file.ms[4] = env ? (double)t_env.ms() : 0.0;
    e->file.ms[5] = f.res_out ? (double)t_out.ms() : 0.0;
    e->file.ms[6] = (double)t_total.ms();
    e->file.rate_out = f.rate_out; e->file.peak = pk;
    e->file.valid = true;
    return RVC_OK;
}

// the stitch alone on host buffers, behind the entry points' checks: windows [W][window_len] laid end to end, file f holding globals [P[f], P[f + 1]) and
// every file's tail starting as zeros -> out [W][frame], offsets [W] (may be null)
static void sola_stitch_run(rvc_engine *e, const float *windows, const std::vector<int> &P, size_t window_len, size_t sola_len, size_t search, size_t frame, float *out,
                            int32_t *offsets)
{
    const size_t F = P.size() - 1, W = (size_t)P.back();
    std::vector<long long> zero(F + 1, 0), out_off(F), out_n(F);
    for (size_t f = 0; f < F; f++) { out_off[f] = (long long)((size_t)P[f] * frame); out_n[f] = (long long)((size_t)(P[f + 1] - P[f]) * frame); }
    hipStream_t st = e->stream;
    DevBuf<float> d_y, d_tails, d_out; DevBuf<int> d_off;
    d_y.alloc(W * window_len); d_tails.alloc((W + 1) * sola_len); d_out.alloc(W * frame); d_off.alloc(W);
    ManyDeviceTables tabs;
    tabs.upload(P, zero, zero, out_off, out_n, zero);
    HIPCHK(hipMemcpyAsync(d_y.get(), windows, W * window_len * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_tails.get(), 0, sola_len * sizeof(float), st));
    const size_t step = 4096;      // windows per pair of launches (the assembly's grid.y; at most as many files, the chain's grid.x)
    for (size_t g0 = 0; g0 < W; g0 += step) {
        const size_t nw = std::min(step, W - g0);
        const int f_first = many_file_of(P.data(), (int)F, (int)g0), f_last = many_file_of(P.data(), (int)F, (int)(g0 + nw - 1));
        launch_stitch_many(st, d_y.get() + g0 * window_len, (long long)window_len, (int)g0, (int)nw, f_first, f_last, tabs.t, (int)sola_len, (int)search, (int)frame, d_tails.get(),
                           d_off.get(), d_out.get());
    }
    std::vector<int32_t> off(W);
    HIPCHK(hipMemcpyAsync(out, d_out.get(), W * frame * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(off.data(), d_off.get(), W * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (offsets) for (size_t i = 0; i < W; i++) offsets[i] = off[i];
}

}  // namespace rvc

extern "C" {

// host only, pure: out = {windows, n, sample_frame_16k_size, skip_head, return_length, hop, zc, output samples}
rvc_status rvc_convert_geometry(size_t n16k, size_t sample_rate, size_t k, size_t context, size_t crossfade, size_t out[8])
{
    if (!out) return RVC_SHAPE;
    ConvertGeometry g;
    if (convert_geometry(n16k, sample_rate, k, context, crossfade, &g)) return RVC_SHAPE;
    const size_t v[8] = {g.windows, g.n, g.sf, g.skip_head, g.return_length, g.H, g.zc, g.out_samples};
    for (int i = 0; i < 8; i++) out[i] = v[i];
    return RVC_OK;
}

rvc_status rvc_convert_device(rvc_engine *e, const void *d_pcm16k, size_t n, size_t k, size_t context, size_t crossfade, int32_t pitch_shift, int highpass, void *d_out,
                              size_t cap, size_t *out_len)
{
    return guarded(e, [&]() {
        ConvertGeometry g;
        const rvc_status rc = convert_check(e, d_pcm16k, n, k, context, crossfade, d_out, cap, out_len, &g);
        if (rc != RVC_OK) return rc;
        return convert_run(e, (const float *)d_pcm16k, n, g, pitch_shift, highpass != 0, (float *)d_out);
    });
}

rvc_status rvc_convert(rvc_engine *e, const float *pcm16k, size_t n, size_t k, size_t context, size_t crossfade, int32_t pitch_shift, int highpass, float *out, size_t cap,
                       size_t *out_len)
{
    return guarded(e, [&]() {
        ConvertGeometry g;
        rvc_status rc = convert_check(e, pcm16k, n, k, context, crossfade, out, cap, out_len, &g);
        if (rc != RVC_OK) return rc;
        DevBuf<float> d_in, d_out;
        d_in.alloc(n); d_out.alloc(g.out_samples);
        HIPCHK(hipMemcpyAsync(d_in.get(), pcm16k, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
        rc = convert_run(e, d_in.get(), n, g, pitch_shift, highpass != 0, d_out.get());
        if (rc != RVC_OK) { (void)hipStreamSynchronize(e->stream); return rc; }
        HIPCHK(hipMemcpy(out, d_out.get(), g.out_samples * sizeof(float), hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

// a recording at any rate -> the voice at rate_out (0 = the model's), with the volume envelope of the input; PCM in, PCM out, one upload and one download
rvc_status rvc_convert_file_device(rvc_engine *e, const void *d_pcm, size_t n, size_t rate_in, size_t k, size_t context, size_t crossfade, int32_t pitch_shift, int highpass,
                                   double rms_mix_rate, size_t rate_out, void *d_out, size_t cap, size_t *out_len)
{
    return guarded(e, [&]() {
        FileGeometry f;
        const rvc_status rc = convert_file_check(e, d_pcm, n, rate_in, k, context, crossfade, rms_mix_rate, rate_out, d_out, cap, out_len, &f);
        if (rc != RVC_OK) return rc;
        return convert_file_run(e, (const float *)d_pcm, n, f, pitch_shift, highpass != 0, rms_mix_rate, (float *)d_out);
    });
}

rvc_status rvc_convert_file(rvc_engine *e, const float *pcm, size_t n, size_t rate_in, size_t k, size_t context, size_t crossfade, int32_t pitch_shift, int highpass,
                            double rms_mix_rate, size_t rate_out, float *out, size_t cap, size_t *out_len)
{
    return guarded(e, [&]() {
        FileGeometry f;
        rvc_status rc = convert_file_check(e, pcm, n, rate_in, k, context, crossfade, rms_mix_rate, rate_out, out, cap, out_len, &f);
        if (rc != RVC_OK) return rc;
        DevBuf<float> d_in, d_out;
        d_in.alloc(n); d_out.alloc(f.n_out);
        HIPCHK(hipMemcpyAsync(d_in.get(), pcm, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
        rc = convert_file_run(e, d_in.get(), n, f, pitch_shift, highpass != 0, rms_mix_rate, d_out.get());
        if (rc != RVC_OK) { (void)hipStreamSynchronize(e->stream); return rc; }
        HIPCHK(hipMemcpy(out, d_out.get(), f.n_out * sizeof(float), hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

// of the last completed rvc_convert_file: device ms = {resample in, high-pass, gather + model, stitch, envelope, resample out, total}, the output rate, max |out|
rvc_status rvc_convert_file_info(rvc_engine *e, double ms[7], size_t *rate_out, float *peak)
{
    return guarded(e, [&]() {
        if (!e->file.valid) throw ShapeError("convert_file_info: no convert_file has completed on this engine");
        if (ms) for (int i = 0; i < 7; i++) ms[i] = e->file.ms[i];
        if (rate_out) *rate_out = e->file.rate_out;
        if (peak) *peak = e->file.peak;
        return RVC_OK;
    });
}

// of the last completed convert: windows, batches, the SOLA offset of every window (up to cap_offsets of them), device milliseconds
// {high-pass, gather + model, stitch, total}; any pointer may be NULL
rvc_status rvc_convert_info(rvc_engine *e, size_t *windows, size_t *batches, int32_t *offsets, size_t cap_offsets, double ms[4])
{
    return guarded(e, [&]() {
        if (!e->conv.valid) throw ShapeError("convert_info: no convert has completed on this engine");
        if (windows) *windows = e->conv.windows;
        if (batches) *batches = e->conv.batches;
        if (offsets) for (size_t i = 0; i < std::min(cap_offsets, e->conv.offsets.size()); i++) offsets[i] = e->conv.offsets[i];
        if (ms) for (int i = 0; i < 4; i++) ms[i] = e->conv.ms[i];
        return RVC_OK;
    });
}

// the chained LINEAR rvc_sola_step over windows [n_windows][window_len], the tail starting as zeros: out [n_windows][frame], offsets [n_windows] (may be NULL).
// The one-file call of what rvc_sola_stitch_many does (sola_stitch_run above)
rvc_status rvc_sola_stitch(rvc_engine *e, const float *windows, size_t n_windows, size_t window_len, size_t sola_len, size_t search, size_t frame, float *out, int32_t *offsets)
{
    return guarded(e, [&]() {
        if (!windows || !out) throw ShapeError("sola_stitch: null buffer");
        if (n_windows < 1 || n_windows > (size_t)1 << 24) throw ShapeError("sola_stitch: window count out of range");
        if (search > 1023) throw ShapeError("sola_stitch: search range longer than 1023 samples");
        if (sola_len < 1 || frame < sola_len) throw ShapeError("sola_stitch: the frame must be at least as long as the crossfade (a window's tail is then its own samples)");
        if (window_len > (size_t)1 << 28 || window_len < search + frame + sola_len) throw ShapeError("sola_stitch: a window holds fewer than search + frame + sola_len samples");
        sola_stitch_run(e, windows, {0, (int)n_windows}, window_len, sola_len, search, frame, out, offsets);
        return RVC_OK;
    });
}

// the silence gate of the file converter (silence.hip.h): engine-wide, at or below -60 dB = off (the default), hang in [0, 1000] frames; anything else, NaN
// included, is refused and changes nothing
rvc_status rvc_set_convert_silence(rvc_engine *e, double threshold_db, int hang_frames)
{
    return guarded(e, [&]() {
        if (threshold_db != threshold_db) throw ShapeError("convert silence: the threshold is not a number");
        if (hang_frames < 0 || hang_frames > SILENCE_MAX_HANG) throw ShapeError("convert silence: the hang is in [0, 1000] frames");
        e->sil_db = threshold_db; e->sil_hang = hang_frames;
        return RVC_OK;
    });
}

rvc_status rvc_convert_silence(rvc_engine *e, double *threshold_db, int *hang_frames)
{
    return guarded(e, [&]() {
        if (threshold_db) *threshold_db = e->sil_db;
        if (hang_frames) *hang_frames = e->sil_hang;
        return RVC_OK;
    });
}

// of the last completed conversion or analysis that ran with the gate: windows run and skipped, loud and kept frames, device ms of the gate's own kernels
rvc_status rvc_convert_silence_info(rvc_engine *e, size_t *windows_run, size_t *windows_skipped, size_t *frames_loud, size_t *frames_kept, double *ms_analysis)
{
    return guarded(e, [&]() {
        if (!e->sil_info.valid) throw ShapeError("convert_silence_info: no call has run with the silence gate on this engine");
        if (windows_run) *windows_run = e->sil_info.run;
        if (windows_skipped) *windows_skipped = e->sil_info.skipped;
        if (frames_loud) *frames_loud = e->sil_info.loud;
        if (frames_kept) *frames_kept = e->sil_info.kept;
        if (ms_analysis) *ms_analysis = e->sil_info.ms;
        return RVC_OK;
    });
}

// the gate's analysis alone, on host buffers and with its own threshold (applied as given: -60 is a threshold here, not "off") and hang; no model is needed.
// frame_loud / frame_kept [Nf] (cap_frames), window_active / window_place [W] (cap_windows); any of them may be NULL, a given one with a short cap is RVC_SHAPE
rvc_status rvc_silence_map(rvc_engine *e, const float *pcm16k, size_t n, double threshold_db, int hang_frames, size_t k, size_t context, size_t crossfade, size_t sample_rate,
                           uint8_t *frame_loud, uint8_t *frame_kept, size_t cap_frames, uint8_t *window_active, int32_t *window_place, size_t cap_windows)
{
    return guarded(e, [&]() {
        if (n == 0 || !pcm16k) throw ShapeError("silence_map: empty recording");
        if (threshold_db != threshold_db) throw ShapeError("silence_map: the threshold is not a number");
        if (hang_frames < 0 || hang_frames > SILENCE_MAX_HANG) throw ShapeError("silence_map: the hang is in [0, 1000] frames");
        ConvertGeometry g;
        if (const char *why = convert_geometry(n, sample_rate, k, context, crossfade, &g)) throw ShapeError(why);
        if (g.windows > (size_t)1 << 30) throw ShapeError("silence_map: recording too long");
        if ((frame_loud || frame_kept) && cap_frames < g.Nf) throw ShapeError("silence_map: frame buffer too small");
        if ((window_active || window_place) && cap_windows < g.windows) throw ShapeError("silence_map: window buffer too small");
        hipStream_t st = e->stream;
        DevBuf<float> d_in;
        d_in.alloc(n);
        HIPCHK(hipMemcpyAsync(d_in.get(), pcm16k, n * sizeof(float), hipMemcpyHostToDevice, st));
        SilenceWork w;
        many_gate(st, d_in.get(), convert_many_single(g, n), threshold_db, hang_frames, 0, &w);
        std::vector<int> act;
        if (frame_loud) HIPCHK(hipMemcpyAsync(frame_loud, w.loud.get(), g.Nf, hipMemcpyDeviceToHost, st));
        if (frame_kept) HIPCHK(hipMemcpyAsync(frame_kept, w.kept.get(), g.Nf, hipMemcpyDeviceToHost, st));
        if (window_place) HIPCHK(hipMemcpyAsync(window_place, w.place.get(), g.windows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (window_active) { act.resize(g.windows); HIPCHK(hipMemcpyAsync(act.data(), w.active.get(), g.windows * sizeof(int), hipMemcpyDeviceToHost, st)); }
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        if (window_active) for (size_t i = 0; i < g.windows; i++) window_active[i] = (uint8_t)(act[i] != 0);
        silence_gate_report(e, w);
        return RVC_OK;
    });
}

// the converter's 48 Hz zero-phase high-pass on its own: out[n]
rvc_status rvc_highpass(rvc_engine *e, const float *pcm16k, size_t n, float *out)
{
    return guarded(e, [&]() {
        if (!pcm16k || !out || n < 1) throw ShapeError("highpass: empty signal");
        DevBuf<float> d_x, d_y;
        d_x.alloc(n); d_y.alloc(n);
        HIPCHK(hipMemcpyAsync(d_x.get(), pcm16k, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
        launch_highpass(e, d_x.get(), n, d_y.get());
        HIPCHK(hipMemcpyAsync(out, d_y.get(), n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipGetLastError());
        return RVC_OK;
    });
}

}  // extern "C"
