// convert.hip.h -- conversion of a whole recording (upstream's "model inference" tab, vc_single), included by engine.hip.
//
// The recording is cut into windows of ONE geometry (convert_geometry.h), so one plan serves the whole file; the windows run S at a time through
// infer_common on the engine's S streams (window w = i S + s on stream s in batch i) and are stitched by the plugin's SOLA step in its LINEAR crossfade,
// chained over the windows on the device (stitch.hip.h).  In front of it the optional 48 Hz high-pass (highpass.hip.h).  Per batch: one gather launch,
// one infer call with its one synchronisation, two stitch launches; the signal, S window inputs, S window outputs, the tails and the output stay in HBM.
// f0_analyze.hip.h (included below): the same windows through the pitch-only plan -- rvc_analyze_f0 --, order statistics of f0 rows, and auto-transpose.
#pragma once
#include "convert_geometry.h"
#include "highpass.hip.h"
#include "stitch.hip.h"
#include "resample_whole.hip.h"
#include "change_rms.hip.h"
#include "silence.hip.h"

namespace rvc {
// (what f0_analyze.hip.h uses of this file, defined below)
static void launch_highpass(rvc_engine *e, const float *d_x, size_t n, float *d_y);
static void launch_window_gather(hipStream_t st, const float *sig, long long N, float *dst, int n, int S, long long w0, int nw, int H, int C);
// the silence gate of a call on one recording (silence.hip.h): the analysis of sig and the tables of a call of one file
struct SilenceGate { SilenceWork work; ManyDeviceTables tabs; };
static void silence_gate_run(rvc_engine *e, const float *sig, size_t n, const ConvertGeometry &g, size_t zero_len, SilenceGate *gate);
static void silence_gate_report(rvc_engine *e, const SilenceWork &w);
static inline bool silence_gate_on(const rvc_engine *e) { return e->sil_db > SILENCE_OFF_DB; }
}
#include "f0_analyze.hip.h"

namespace rvc {

// the plan's batch input [S][n]: stream s gets window w0 + s of the signal, samples [160 (w H - C), + n), zero outside [0, N); streams at or beyond nw
// (the padding of a short last batch) get zeros
static __global__ void window_gather_kernel(const float *sig, long long N, float *dst, int n, long long w0, int nw, int H, int C)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (i >= n) return;
    float v = 0.f;
    if (s < nw) {
        const long long src = 160LL * ((w0 + s) * (long long)H - C) + i;
        if (src >= 0 && src < N) v = sig[src];
    }
    dst[(long long)s * n + i] = v;
}

static void launch_window_gather(hipStream_t st, const float *sig, long long N, float *dst, int n, int S, long long w0, int nw, int H, int C)
{
    hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)S), dim3(256), 0, st, sig, N, dst, n, w0, nw, H, C);
}

static void launch_highpass(rvc_engine *e, const float *d_x, size_t n, float *d_y)
{
    if (!e->hp_taps) {
        const std::vector<float> h = highpass_taps();
        e->hp_taps.alloc(h.size());
        HIPCHK(hipMemcpy(e->hp_taps.get(), h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (n > ((size_t)1 << 40)) throw ShapeError("highpass: signal too long");
    hipLaunchKernelGGL(highpass_fir_kernel, dim3((unsigned)((n + HP_TILE - 1) / HP_TILE)), dim3(HP_THREADS), 0, e->stream, d_x, (long long)n, (const float *)e->hp_taps.get(), d_y);
}

// the gate's analysis of one recording with the engine's setting, queued on the engine's stream; returns behind the call's one read (synchronised)
static void silence_gate_run(rvc_engine *e, const float *sig, size_t n, const ConvertGeometry &g, size_t zero_len, SilenceGate *gate)
{
    gate->work.begin(e->stream, g.Nf, g.windows, e->sil_db, e->sil_hang, zero_len);
    silence_single_tables(&gate->tabs, n, g);
    gate->work.queue_file(e->stream, sig, n, g.Nf, 0, g.windows, 0, g);
    gate->work.finish(e->stream);
}
static void silence_gate_report(rvc_engine *e, const SilenceWork &w)
{
    e->sil_info.run = w.A; e->sil_info.skipped = w.W - w.A; e->sil_info.loud = w.n_loud; e->sil_info.kept = w.n_kept; e->sil_info.ms = w.ms;
    e->sil_info.valid = true;
}

// the two stitch launches for windows [w0, w0 + nw) whose outputs lie in y [nw][y_bs]
static void launch_stitch(hipStream_t st, const float *y, long long y_bs, int w0, int nw, int sola_len, int search, int frame, float *tails, int *offsets, float *out, long long n_out)
{
    hipLaunchKernelGGL(stitch_chain_kernel, dim3(1), dim3(STITCH_CHAIN_THREADS), 0, st, y, y_bs, w0, nw, sola_len, search, frame, tails, offsets);
    hipLaunchKernelGGL(stitch_assemble_kernel, dim3((unsigned)((frame + STITCH_TILE - 1) / STITCH_TILE), (unsigned)nw), dim3(256), 0, st, y, y_bs, w0, sola_len, frame,
                       (const float *)tails, (const int *)offsets, out, n_out);
}

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

// the conversion proper, device to device.  Begins with what rvc_reset_state does (pitch caches and chunk counters zeroed), so that a window's result depends
// on the recording alone; every per-stream setting, the index, the f0 method and graph replay apply as to any infer call.  keep_filtered (rvc_convert_file): the
// high-passed signal is handed to the caller instead of being freed
static rvc_status convert_run(rvc_engine *e, const float *d_pcm, size_t n, const ConvertGeometry &g, int32_t pitch_shift, bool highpass, float *d_out,
                              DevBuf<float> *keep_filtered = nullptr)
{
    hipStream_t st = e->stream;
    const size_t S = (size_t)e->n_streams, W = g.windows;
    size_t batches = (W + S - 1) / S;
    const size_t sola_len = g.X * g.zc, search = g.Q * g.zc, frame = g.H * g.zc, ylen = g.return_length * g.zc;
    const bool gated = silence_gate_on(e);
    e->conv.valid = false; e->conv_f0_valid = false;
    HIPCHK(hipDeviceSynchronize());
    reset_state(e);          // (pending f0 overrides of the streams go with it: a conversion uses the curve alone)
    // f0 from outside.  The f0 front end takes the last fr samples of a window and reflect-pads them by 512, so f0 row t of window w is
    // centred on sample 160 (w H - C) + (n - fr) + 160 t of the recording: grid row w H - Cg + t with Cg = C - (n - fr) / 160.  (fr = n for every geometry
    // convert_geometry makes; the check stays.)  The curve's grid is built once; each batch's plan gathers from it, and the conditioned rows of each window's
    // hop [Cg, Cg + H) go back onto the grid for rvc_convert_f0
    const bool has_f0 = e->sy->has_f0;
    const size_t fr = 5120 * ((g.sf + 799) / 5120 + 1) - 160;
    if (has_f0 && (fr > g.n || (g.n - fr) % 160 != 0 || (g.n - fr) / 160 > g.C)) throw ShapeError("convert: the f0 rows of a window are not centred on the recording's 10 ms grid");
    const int Cg = (int)(g.C - (g.n - fr) / 160);
    const bool curve = has_f0 && e->curve_n > 0;
    struct CurveGuard { rvc_engine *e; ~CurveGuard() { e->conv_curve = false; e->ov_dirty = true; } } curve_guard{e};
    DevBuf<float> f0grid;
    bool export_ok = has_f0;
    if (has_f0) f0grid.alloc(g.Nf);
    if (curve) {
        e->curve_grid.alloc(g.Nf);
        launch_f0_curve_grid(st, e->curve_t.get(), e->curve_hz.get(), (int)e->curve_n, e->curve_grid.get(), (long long)g.Nf);
        e->conv_curve = true;
    }
    DevTimer t_total, t_hp;
    t_total.start(st);
    DevBuf<float> filtered;
    const float *sig = d_pcm;
    if (highpass) {
        filtered.alloc(n);
        t_hp.start(st);
        launch_highpass(e, d_pcm, n, filtered.get());
        t_hp.stop(st);
        sig = filtered.get();
    }
    // the silence gate (silence.hip.h): with a threshold set, the signal the model will see is measured first, the active windows are
    // compacted and only they run; a skipped window enters the stitch as zeros.  Off (the default): nothing is queued here and the loop below is the ungated one
    SilenceGate gate;
    if (gated) {
        silence_gate_run(e, sig, n, g, ylen, &gate);
        batches = gate.work.batches(S);
        if (has_f0) HIPCHK(hipMemsetAsync(f0grid.get(), 0, g.Nf * sizeof(float), st));      // (the rows of skipped windows are 0)
    }
    // auto-transpose (f0_analyze.hip.h): with a target set, the f0 of the signal the model will see is analysed first -- the call's own
    // windows through the pitch-only plan (the gate's active ones when it is on) --, the curve merged in, and 12 log2(target / median) semitones become one more
    // factor of every stream's multiplier until the call returns, on whatever path.  Off (the default): nothing is queued here
    struct AutoGuard { rvc_engine *e; ~AutoGuard() { e->auto_mul = 0.f; } } auto_guard{e};
    if (has_f0 && e->at_target > 0.0) {
        float mul = 0.f;
        const rvc_status rc = auto_transpose_run(e, sig, n, g, curve ? e->curve_grid.get() : nullptr, &mul, gated ? &gate : nullptr);
        if (rc != RVC_OK) return rc;
        e->auto_mul = mul;
    }
    DevBuf<float> win, y, tails; DevBuf<int> offs;
    win.alloc(S * g.n + 64); y.alloc(S * ylen + 64); tails.alloc((W + 1) * sola_len); offs.alloc(W);
    HIPCHK(hipMemsetAsync(win.get(), 0, (S * g.n + 64) * sizeof(float), st));
    HIPCHK(hipMemsetAsync(tails.get(), 0, sola_len * sizeof(float), st));       // tails[0]: the stitch starts from silence
    std::vector<DevEvent> ev(3 * batches);
    for (size_t b = 0; b < batches; b++) {
        // (gated: w0 is the batch's first PLACE and nw its active windows, of the A in all)
        const size_t w0 = b * S; const int nw = (int)std::min(S, (gated ? gate.work.A : W) - w0);
        ev[3 * b].record(st);
        if (gated) gate.work.gather(st, sig, gate.tabs.t, win.get(), S, w0, g);
        else hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)((g.n + 255) / 256), (unsigned)S), dim3(256), 0, st, sig, (long long)n, win.get(), (int)g.n, (long long)w0, nw,
                           (int)g.H, (int)g.C);
        size_t got = 0;
        if (curve) e->conv_call = F0OvCall{e->curve_grid.get(), (long long)g.Nf, 1, (int)w0, nw, (int)g.H, Cg, 0, gated ? gate.work.win_of.get() : nullptr};
        const rvc_status rc = infer_common(e, win.get(), true, g.n, g.sf, pitch_shift, (uint32_t)g.skip_head, (uint32_t)g.return_length, y.get(), true, ylen, &got, true);
        if (rc != RVC_OK) return rc;
        if (got != ylen) throw ShapeError("convert: the synthesizer does not produce sample_rate / 100 samples per frame");
        ev[3 * b + 1].record(st);
        if (gated) gate.work.stitch(st, y.get(), (long long)ylen, w0, nw, gate.tabs.t, (int)sola_len, (int)search, (int)frame, tails.get(), offs.get(), d_out);
        else launch_stitch(st, y.get(), (long long)ylen, (int)w0, nw, (int)sola_len, (int)search, (int)frame, tails.get(), offs.get(), d_out, (long long)g.out_samples);
        ev[3 * b + 2].record(st);
        // the batch's conditioned f0 rows onto the grid, behind the timed sections: in ms[3] (total), in neither ms[1] (model) nor ms[2] (stitch).  The plan's rows
        // stay until the next batch's pitch tail, which this stream orders behind the launch
        if (export_ok) {
            const Plan *pl = e->last_plan;      // (streams in several formant buckets ran through several plans: no export then)
            if (pl && !pl->key.bucket && pl->d_f0 && pl->key.B == (int)S && (size_t)Cg + g.H <= (size_t)pl->Tm) {
                if (gated) gate.work.export_f0(st, pl->d_f0, pl->Tm, S, w0, (int)g.H, Cg, f0grid.get(), (long long)g.Nf);
                else launch_f0_export(st, pl->d_f0, pl->Tm, (int)w0, nw, (int)g.H, Cg, f0grid.get(), (long long)g.Nf);
            } else export_ok = false;
        }
    }
    // a gated call without an active window: no batch ran; the stitch walks its W windows of zeros (offsets and output as rvc_sola_stitch's on zeros)
    DevTimer t_zero;
    if (gated && batches == 0) {
        t_zero.start(st);
        gate.work.stitch(st, y.get(), (long long)ylen, 0, 0, gate.tabs.t, (int)sola_len, (int)search, (int)frame, tails.get(), offs.get(), d_out);
        t_zero.stop(st);
    }
    t_total.stop(st);
    e->conv.offsets.assign(W, 0);
    HIPCHK(hipMemcpyAsync(e->conv.offsets.data(), offs.get(), W * sizeof(int32_t), hipMemcpyDeviceToHost, st));
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
    if (gated) silence_gate_report(e, gate.work);
    e->conv.windows = W; e->conv.batches = batches;
    e->conv.ms[0] = highpass ? (double)t_hp.ms() : 0.0; e->conv.ms[1] = ms_model; e->conv.ms[2] = ms_stitch; e->conv.ms[3] = (double)t_total.ms();
    e->conv.valid = true; e->conv_f0_valid = export_ok;
    if (keep_filtered) *keep_filtered = std::move(filtered);
    return RVC_OK;
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

// the chained LINEAR rvc_sola_step over windows [n_windows][window_len], the tail starting as zeros: out [n_windows][frame], offsets [n_windows] (may be NULL)
rvc_status rvc_sola_stitch(rvc_engine *e, const float *windows, size_t n_windows, size_t window_len, size_t sola_len, size_t search, size_t frame, float *out, int32_t *offsets)
{
    return guarded(e, [&]() {
        if (!windows || !out) throw ShapeError("sola_stitch: null buffer");
        if (n_windows < 1 || n_windows > (size_t)1 << 24) throw ShapeError("sola_stitch: window count out of range");
        if (search > 1023) throw ShapeError("sola_stitch: search range longer than 1023 samples");
        if (sola_len < 1 || frame < sola_len) throw ShapeError("sola_stitch: the frame must be at least as long as the crossfade (a window's tail is then its own samples)");
        if (window_len > (size_t)1 << 28 || window_len < search + frame + sola_len) throw ShapeError("sola_stitch: a window holds fewer than search + frame + sola_len samples");
        hipStream_t st = e->stream;
        DevBuf<float> d_y, d_tails, d_out; DevBuf<int> d_off;
        d_y.alloc(n_windows * window_len); d_tails.alloc((n_windows + 1) * sola_len); d_out.alloc(n_windows * frame); d_off.alloc(n_windows);
        HIPCHK(hipMemcpyAsync(d_y.get(), windows, n_windows * window_len * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(d_tails.get(), 0, sola_len * sizeof(float), st));
        const size_t step = 4096;      // windows per pair of launches (the assembly's grid.y)
        for (size_t w0 = 0; w0 < n_windows; w0 += step)
            launch_stitch(st, d_y.get() + w0 * window_len, (long long)window_len, (int)w0, (int)std::min(step, n_windows - w0), (int)sola_len, (int)search, (int)frame,
                          d_tails.get(), d_off.get(), d_out.get(), (long long)(n_windows * frame));
        std::vector<int32_t> off(n_windows);
        HIPCHK(hipMemcpyAsync(out, d_out.get(), n_windows * frame * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(off.data(), d_off.get(), n_windows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        if (offsets) for (size_t i = 0; i < n_windows; i++) offsets[i] = off[i];
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
        w.begin(st, g.Nf, g.windows, threshold_db, hang_frames, 0);
        w.queue_file(st, d_in.get(), n, g.Nf, 0, g.windows, 0, g);
        w.finish(st);
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
