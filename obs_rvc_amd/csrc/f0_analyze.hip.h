// f0_analyze.hip.h -- the f0 of recordings without the synthesizer, exact order statistics of f0 rows, and auto-transpose (the
// forks' "proposed pitch"), included by f0_analyze_many.hip.h (engine.hip's unit).
//
// An analysis cuts its recordings into the converter's windows (convert_many_geometry.h; windows.hip.h gathers them), runs them S = rvc_set_streams at a time
// through the pitch-only plan (PlanKey::mode 2, B = S) of that geometry under a NEUTRAL control block -- multiplier 1, every pitch control off, whatever the
// streams' settings say -- and exports the hop rows of every window onto the 10 ms grids (launch_f0_export_many).  A row is what rvc_pitch returns for that
// window with pitch_shift = 0 and neutral controls.  analyze_many_run is the one loop: rvc_analyze_f0 is its call of one file, rvc_analyze_f0_many
// (f0_analyze_many.hip.h) its call of many.  rvc_f0_stats / rvc_f0_stats_stream select quantiles of the voiced rows (f0_select.hip.h).  rvc_set_auto_transpose
// makes rvc_convert* / rvc_convert_file* run the analysis in front of their first batch, take the lower median and transpose by 12 log2(target / median)
// semitones for the duration of the call (convert.hip.h calls auto_transpose_run).
// A stream's pitch cache holds CONDITIONED f0 -- behind pitch_shift, the semitone transpose and the pitch controls: a host that wants the raw median of a live
// stream from rvc_f0_stats_stream reads it while its transpose is 0.
#pragma once
#include "windows.hip.h"
#include "f0_select.hip.h"

namespace rvc {

// the window geometry of an analysis; sample_rate only scales the output side of the converter's geometry, which an analysis does not have: a model-free call
// uses 16 000
static void analyze_shape(size_t n, size_t sample_rate, size_t k, size_t context, size_t crossfade, ConvertGeometry *g)
{
    if (n == 0) throw ShapeError("analyze_f0: empty recording");
    if (const char *why = convert_geometry(n, sample_rate, k, context, crossfade, g)) throw ShapeError(why);
    if (g->windows > (size_t)1 << 30) throw ShapeError("analyze_f0: recording too long");
}

// row offset of a window's f0 rows against the recording's 10 ms grid.  The f0 front end takes the last fr samples of a window and reflect-pads them by 512, so
// f0 row t of window w is centred on sample 160 (w H - C) + (n - fr) + 160 t of the recording: grid row w H - Cg + t with Cg = C - (n - fr) / 160.  (fr = n for
// every geometry convert_geometry makes; the check stays.)  who: the caller's name in the refusal
static int analyze_cg(const ConvertGeometry &g, const char *who = "analyze_f0")
{
    const size_t fr = 5120 * ((g.sf + 799) / 5120 + 1) - 160;
    if (fr > g.n || (g.n - fr) % 160 != 0 || (g.n - fr) / 160 > g.C) throw ShapeError(std::string(who) + ": the f0 rows of a window are not centred on the recording's 10 ms grid");
    return (int)(g.C - (g.n - fr) / 160);
}

// The analysis proper, device to device: sig = the signal arena of the call, tabs its tables, grid the grid arena (file f's Nf_f rows at tabs.goff[f]).  Begins
// with what rvc_reset_state does and leaves the state that way (a pitch-only plan writes neither the cache nor the chunk counter); returns synchronised, the
// streams' status words checked.  gate (the silence gate's analysis of sig): only its active windows run, compacted; the caller has
// zeroed the grid, which keeps 0 in the rows of skipped windows.  who: the entry point's name in the refusal
static rvc_status analyze_many_run(rvc_engine *e, const float *sig, const ConvertManyGeometry &m, const ManyTables &tabs, float *grid, const SilenceWork *gate, const char *who)
{
    hipStream_t st = e->stream;
    const ConvertGeometry &g = m.g;
    const size_t S = (size_t)e->n_streams, N = gate ? gate->A : m.windows_total(), batches = (N + S - 1) / S;
    const int Cg = analyze_cg(g);
    HIPCHK(hipDeviceSynchronize());
    reset_state(e);
    if (N == 0) { HIPCHK(hipStreamSynchronize(st)); return RVC_OK; }      // (a gated call without an active window: no plan is built, the zeroed grid is the result)
    Plan *pl = get_plan(e, plan_key(e, 2, g.n, g.sf, 0, 0));
    if (pl->key.B != (int)S || !pl->d_f0 || (size_t)Cg + g.H > (size_t)pl->Tm) throw ShapeError(std::string(who) + ": a window's hop lies outside its f0 rows");
    pl->cur_in = nullptr; pl->cur_out = nullptr;
    push_call_params(e, 0, nullptr, nullptr, true);
    for (size_t b = 0; b < batches; b++) {
        const size_t g0 = b * S; const int nw = (int)std::min(S, N - g0);      // (gated: g0 is the batch's first place)
        launch_gather_windows(st, sig, tabs, pl->d_in, S, gate, g0, nw, g);
        run_plan(e, *pl);
        launch_f0_export_many(st, pl->d_f0, pl->Tm, tabs, S, gate, g0, nw, (int)g.H, Cg, grid);
    }
    queue_status(e);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return final_status(e);
}

static void check_quantiles(const double *quantile, size_t nq, const float *out_hz)
{
    if (nq < 1 || nq > (size_t)F0_SEL_MAXQ) throw ShapeError("f0_stats: 1 to 8 quantiles");
    if (!quantile || !out_hz) throw ShapeError("f0_stats: null buffer");
    for (size_t i = 0; i < nq; i++) if (!(quantile[i] >= 0.0 && quantile[i] <= 1.0)) throw ShapeError("f0_stats: a quantile is outside [0, 1]");
}

// the select over n rows on the device, queued on the engine's stream; read_select copies the nq values and v back behind it (the call's one copy)
static void queue_select(rvc_engine *e, const float *d_rows, size_t n, const double *quantile, size_t nq)
{
    if (!e->sel_ws) e->sel_ws.alloc(F0_SEL_WS_WORDS);
    launch_f0_select(e->stream, d_rows, n, quantile, (int)nq, e->sel_ws.get());
}
static void read_select(rvc_engine *e, size_t nq, float *out_hz, size_t *voiced)
{
    uint32_t res[F0_SEL_MAXQ + 1];
    HIPCHK(hipMemcpyAsync(res, e->sel_ws.get() + F0_SEL_OUT_AT, sizeof res, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    for (size_t i = 0; i < nq; i++) memcpy(&out_hz[i], &res[i], sizeof(float));
    if (voiced) *voiced = res[F0_SEL_MAXQ];
}

// the arguments of rvc_set_auto_transpose and rvc_set_convert_many_auto_transpose
static void auto_transpose_check(double target_hz, int step, double limit)
{
    if (!(target_hz >= 0.0 && target_hz <= 20000.0)) throw ShapeError("auto transpose: the target is 0 (off) or in (0, 20000] Hz");
    if (step != 0 && step != 1 && step != 12) throw ShapeError("auto transpose: the step is 0 (exact), 1 (semitones) or 12 (octaves)");
    if (!(limit >= 0.0 && limit <= 24.0)) throw ShapeError("auto transpose: the limit is in [0, 24] semitones");
}

// a = 12 log2(target / m) in double, rounded to the step (ties to even), clamped to [-limit, limit]; no voiced row: 0
static double auto_transpose_semitones(double target, double median, size_t voiced, int step, double limit)
{
    if (voiced == 0 || !(median > 0.0)) return 0.0;
    double a = 12.0 * std::log2(target / median);
    if (step > 0) a = (double)step * std::nearbyint(a / (double)step);      // (the default rounding mode: to nearest, ties to even)
    return std::min(std::max(a, -limit), limit);
}

// In front of the first batch of a conversion of ONE recording (m: its call of one file; a target is set and the model has pitch guidance): the analysis of the
// signal the model will see, the curve merged in when one is in force (curve_grid: its grid, or null), the lower median, the transpose.  -> the factor every
// stream's multiplier takes for the rest of the call, 0 = none.  Ends with the engine in the reset state the conversion starts from
static rvc_status auto_transpose_run(rvc_engine *e, const float *sig, const ConvertManyGeometry &m, const ManyTables &tabs, const float *curve_grid, float *mul, const SilenceWork *gate)
{
    hipStream_t st = e->stream;
    const size_t Nf = m.g.Nf;
    *mul = 0.f;
    e->at_info.valid = false;
    DevBuf<float> grid;
    grid.alloc(Nf);
    DevTimer t_an, t_sel;
    HIPCHK(hipMemsetAsync(grid.get(), 0, Nf * sizeof(float), st));
    t_an.start(st);
    const rvc_status rc = analyze_many_run(e, sig, m, tabs, grid.get(), gate, "analyze_f0");
    if (rc != RVC_OK) return rc;
    t_an.stop(st);
    t_sel.start(st);
    if (curve_grid) hipLaunchKernelGGL(f0_merge_kernel, dim3((unsigned)((Nf + 255) / 256)), dim3(256), 0, st, grid.get(), curve_grid, (long long)Nf);
    const double half = 0.5;
    queue_select(e, grid.get(), Nf, &half, 1);
    t_sel.stop(st);
    float median = 0.f; size_t voiced = 0;
    read_select(e, 1, &median, &voiced);
    const double a = auto_transpose_semitones(e->at_target, (double)median, voiced, e->at_step, e->at_limit);
    if (a != 0.0) *mul = (float)std::pow(2.0, a / 12.0);
    e->at_info.median = median; e->at_info.voiced = voiced; e->at_info.semitones = a;
    e->at_info.ms[0] = (double)t_an.ms(); e->at_info.ms[1] = (double)t_sel.ms();
    e->at_info.valid = true;
    reset_state(e);      // (the analysis left the neutral control block on the device and may have raised status words: the conversion starts from the reset state)
    return RVC_OK;
}

}  // namespace rvc

extern "C" {

rvc_status rvc_analyze_f0_device(rvc_engine *e, const void *d_pcm16k, size_t n, size_t k, size_t context, size_t crossfade, int highpass, void *d_hz, size_t cap,
                                 size_t *n_frames)
{
    return guarded(e, [&]() {
        if (!e->f0_method) return RVC_F0_NOT_LOADED;
        ConvertGeometry g;
        analyze_shape(n, 16000, k, context, crossfade, &g);
        if (n_frames) *n_frames = g.Nf;
        if (cap < g.Nf) { e->err = "analyze_f0: output buffer too small"; return RVC_SHAPE; }
        if (!d_pcm16k || !d_hz) throw ShapeError("analyze_f0: null buffer");
        const ConvertManyGeometry m = convert_many_single(g, n);      // the call of one file
        ManyDeviceTables tabs;
        tabs.upload(m);
        DevBuf<float> filtered;
        const float *sig = (const float *)d_pcm16k;
        if (highpass) {
            filtered.alloc(n);
            launch_highpass(e, sig, n, filtered.get());
            sig = filtered.get();
        }
        const bool gated = silence_gate_on(e);
        SilenceWork gate;
        if (gated) {
            many_gate(e->stream, sig, m, e->sil_db, e->sil_hang, 0, &gate);
            HIPCHK(hipMemsetAsync(d_hz, 0, g.Nf * sizeof(float), e->stream));
        }
        const rvc_status rc = analyze_many_run(e, sig, m, tabs.t, (float *)d_hz, gated ? &gate : nullptr, "analyze_f0");
        if (rc == RVC_OK && gated) silence_gate_report(e, gate);
        return rc;
    });
}

rvc_status rvc_analyze_f0(rvc_engine *e, const float *pcm16k, size_t n, size_t k, size_t context, size_t crossfade, int highpass, float *hz, size_t cap, size_t *n_frames)
{
    return guarded(e, [&]() {
        if (!e->f0_method) return RVC_F0_NOT_LOADED;
        ConvertGeometry g;
        analyze_shape(n, 16000, k, context, crossfade, &g);
        if (n_frames) *n_frames = g.Nf;
        if (cap < g.Nf) { e->err = "analyze_f0: output buffer too small"; return RVC_SHAPE; }
        if (!pcm16k || !hz) throw ShapeError("analyze_f0: null buffer");
        DevBuf<float> d_in, d_out;
        d_in.alloc(n); d_out.alloc(g.Nf);
        HIPCHK(hipMemcpyAsync(d_in.get(), pcm16k, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
        const rvc_status rc = rvc_analyze_f0_device(e, d_in.get(), n, k, context, crossfade, highpass, d_out.get(), g.Nf, nullptr);
        if (rc != RVC_OK) { (void)hipStreamSynchronize(e->stream); return rc; }
        HIPCHK(hipMemcpy(hz, d_out.get(), g.Nf * sizeof(float), hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

rvc_status rvc_f0_stats(rvc_engine *e, const float *hz, size_t n, const double *quantile, size_t nq, float *out_hz, size_t *voiced)
{
    return guarded(e, [&]() {
        if (n < 1 || n > (size_t)1 << 30) throw ShapeError("f0_stats: 1 to 2^30 rows");
        check_quantiles(quantile, nq, out_hz);
        if (!hz) throw ShapeError("f0_stats: null buffer");
        DevBuf<float> d_rows;
        d_rows.alloc(n);
        HIPCHK(hipMemcpyAsync(d_rows.get(), hz, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
        queue_select(e, d_rows.get(), n, quantile, nq);
        read_select(e, nq, out_hz, voiced);
        return RVC_OK;
    });
}

rvc_status rvc_f0_stats_stream(rvc_engine *e, int stream, const double *quantile, size_t nq, float *out_hz, size_t *voiced)
{
    return guarded(e, [&]() {
        if (stream < 0 || stream >= e->n_streams) throw ShapeError("f0_stats: stream out of range");
        check_quantiles(quantile, nq, out_hz);
        static_assert(offsetof(StreamState, cache_pitchf) == 0 && sizeof(StreamState) % 16 == 0, "a stream's pitch cache is 16-byte aligned");
        queue_select(e, e->d_state[stream].cache_pitchf, 1024, quantile, nq);
        read_select(e, nq, out_hz, voiced);
        return RVC_OK;
    });
}

rvc_status rvc_set_auto_transpose(rvc_engine *e, double target_hz, int step, double limit)
{
    return guarded(e, [&]() {
        auto_transpose_check(target_hz, step, limit);
        e->at_target = target_hz; e->at_step = step; e->at_limit = limit;
        return RVC_OK;
    });
}

rvc_status rvc_auto_transpose(rvc_engine *e, double *target_hz, int *step, double *limit)
{
    return guarded(e, [&]() {
        if (target_hz) *target_hz = e->at_target;
        if (step) *step = e->at_step;
        if (limit) *limit = e->at_limit;
        return RVC_OK;
    });
}

rvc_status rvc_auto_transpose_info(rvc_engine *e, float *median_hz, size_t *voiced, double *semitones, double ms[2])
{
    return guarded(e, [&]() {
        if (!e->at_info.valid) throw ShapeError("auto_transpose_info: no conversion has run the analysis on this engine");
        if (median_hz) *median_hz = e->at_info.median;
        if (voiced) *voiced = e->at_info.voiced;
        if (semitones) *semitones = e->at_info.semitones;
        if (ms) { ms[0] = e->at_info.ms[0]; ms[1] = e->at_info.ms[1]; }
        return RVC_OK;
    });
}

}  // extern "C"
