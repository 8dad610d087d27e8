// f0_analyze_many.hip.h -- the f0 of many recordings in one call, their order statistics in one launch, and the per-file pitch pass of rvc_convert_many
// (Applio's batch mode proposes a pitch per file), included by convert.hip.h (engine.hip's unit).
//
// rvc_analyze_f0_many is rvc_analyze_f0 of every file, on the loop rvc_analyze_f0 runs (f0_analyze.hip.h analyze_many_run) and packed as rvc_convert_many
// packs its windows: global window order, S = rvc_set_streams per batch through ONE pitch-only plan (PlanKey::mode 2, B = S) under the neutral control block,
// only the last batch padded.  The rows go to a grid arena: file f's Nf_f rows at goff[f], the prefix sums of Nf_f (convert_many_geometry.h grid_off /
// many_grid_row; the sixth of the call's device tables), zeroed once so that the rows of windows the silence gate skips are 0.
// rvc_f0_stats_many is rvc_f0_stats of every file's rows in one launch (f0_select_many.hip.h).  many_pitch_run strings the two together in front of
// rvc_convert_many's first batch: analysis, lower median per file, the medians and counts down in one copy, the transpose of every file on the host in double.
#pragma once
#include "f0_analyze.hip.h"
#include "f0_select_many.hip.h"

namespace rvc {

// In front of rvc_convert_many's first batch (a per-file setting is on and the model has pitch guidance): the analysis of the signals the model will see, the lower
// median m_f of every file, t_f = semitones[f] + a_f with a_f = auto_transpose_semitones(target, m_f, v_f, ..) (0 with the target off or no voiced row).
// -> mul [F]: the factor (float)2^(t_f / 12) the streams that hold a window of file f take, 0 = none.  Ends with the engine in the reset state the conversion starts from
static rvc_status many_pitch_run(rvc_engine *e, const float *sig, const ConvertManyGeometry &m, const ManyTables &tabs, const SilenceWork *gate, std::vector<float> *mul)
{
    hipStream_t st = e->stream;
    const size_t F = m.files();
    e->many_pitch.valid = false;
    const size_t rows = (size_t)m.grid_off().back();
    DevBuf<float> grid; DevBuf<uint32_t> res;
    grid.alloc(rows); res.alloc(F * F0_SEL_MANY_STRIDE);
    HIPCHK(hipMemsetAsync(grid.get(), 0, rows * sizeof(float), st));
    DevTimer t_an, t_sel;
    t_an.start(st);
    const rvc_status rc = analyze_many_run(e, sig, m, tabs, grid.get(), gate, "analyze_f0_many");
    if (rc != RVC_OK) return rc;
    t_an.stop(st);
    t_sel.start(st);
    const double half = 0.5;
    launch_f0_select_many(st, grid.get(), tabs.goff, F, &half, 1, res.get());
    t_sel.stop(st);
    std::vector<uint32_t> h(F * F0_SEL_MANY_STRIDE);
    HIPCHK(hipMemcpyAsync(h.data(), res.get(), h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    rvc_engine::ManyPitchInfo &pi = e->many_pitch;
    pi.median.assign(F, 0.f); pi.voiced.assign(F, 0); pi.a.assign(F, 0.0); pi.t.assign(F, 0.0);
    mul->assign(F, 0.f);
    for (size_t f = 0; f < F; f++) {
        memcpy(&pi.median[f], &h[f * F0_SEL_MANY_STRIDE], sizeof(float));
        pi.voiced[f] = h[f * F0_SEL_MANY_STRIDE + F0_SEL_MAXQ];
        if (e->many_at_target > 0.0) pi.a[f] = auto_transpose_semitones(e->many_at_target, (double)pi.median[f], pi.voiced[f], e->many_at_step, e->many_at_limit);
        pi.t[f] = (e->many_semitones.empty() ? 0.0 : e->many_semitones[f]) + pi.a[f];
        if (pi.t[f] != 0.0) (*mul)[f] = (float)std::pow(2.0, pi.t[f] / 12.0);
    }
    pi.ms[0] = (double)t_an.ms(); pi.ms[1] = (double)t_sel.ms();
    pi.valid = true;
    reset_state(e);      // (as auto_transpose_run: the analysis left the neutral control block on the device)
    return RVC_OK;
}

}  // namespace rvc

extern "C" {

rvc_status rvc_analyze_f0_many(rvc_engine *e, const float *const *pcm16k, const size_t *n, size_t n_files, size_t k, size_t context, size_t crossfade, int highpass,
                               float *const *hz, const size_t *cap, size_t *n_frames)
{
    return guarded(e, [&]() {
        if (!e->f0_method) return RVC_F0_NOT_LOADED;
        ConvertManyGeometry m;
        if (const char *why = convert_many_geometry(n, n_files, 16000, k, context, crossfade, &m)) throw ShapeError(why);
        (void)analyze_cg(m.g);
        const size_t F = m.files();
        const std::vector<long long> goff = m.grid_off();
        if (n_frames) for (size_t f = 0; f < F; f++) n_frames[f] = (size_t)(goff[f + 1] - goff[f]);
        for (size_t f = 0; f < F; f++)
            if (!cap || cap[f] < (size_t)(goff[f + 1] - goff[f])) { e->err = "analyze_f0_many: output buffer " + std::to_string(f) + " too small"; return RVC_SHAPE; }
        if (!pcm16k || !hz) throw ShapeError("analyze_f0_many: null buffer");
        for (size_t f = 0; f < F; f++) if (!pcm16k[f] || !hz[f]) throw ShapeError("analyze_f0_many: null buffer");
        hipStream_t st = e->stream;
        DevBuf<float> arena, filtered, grid;
        ManyDeviceTables tabs;
        many_upload(pcm16k, m, &arena, &tabs);
        const float *sig = arena.get();
        if (highpass) {
            filtered.alloc(m.sig_total());
            many_highpass(e, arena.get(), m, filtered.get());
            sig = filtered.get();
        }
        const bool gated = silence_gate_on(e);
        SilenceWork gate;
        if (gated) many_gate(st, sig, m, e->sil_db, e->sil_hang, 0, &gate);
        grid.alloc((size_t)goff.back());
        HIPCHK(hipMemsetAsync(grid.get(), 0, (size_t)goff.back() * sizeof(float), st));
        const rvc_status rc = analyze_many_run(e, sig, m, tabs.t, grid.get(), gated ? &gate : nullptr, "analyze_f0_many");
        if (rc != RVC_OK) { (void)hipStreamSynchronize(st); return rc; }
        for (size_t f = 0; f < F; f++)
            HIPCHK(hipMemcpyAsync(hz[f], grid.get() + goff[f], (size_t)(goff[f + 1] - goff[f]) * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        if (gated) silence_gate_report(e, gate);
        reset_state(e);
        return RVC_OK;
    });
}

rvc_status rvc_f0_stats_many(rvc_engine *e, const float *hz, const size_t *rows_per_file, size_t n_files, const double *quantile, size_t nq, float *out_hz, size_t *voiced)
{
    return guarded(e, [&]() {
        if (n_files < 1 || n_files > CONVERT_MANY_MAX_FILES) throw ShapeError("f0_stats_many: the number of files is outside [1, 65536]");
        if (!rows_per_file) throw ShapeError("f0_stats_many: null buffer");
        std::vector<long long> off(n_files + 1, 0);
        for (size_t f = 0; f < n_files; f++) {
            if (rows_per_file[f] < 1 || rows_per_file[f] > (size_t)1 << 30) throw ShapeError("f0_stats_many: a file has 1 to 2^30 rows");
            off[f + 1] = off[f] + (long long)rows_per_file[f];
            if (off[f + 1] > 1LL << 30) throw ShapeError("f0_stats_many: more than 2^30 rows in all");
        }
        check_quantiles(quantile, nq, out_hz);
        if (!hz) throw ShapeError("f0_stats_many: null buffer");
        hipStream_t st = e->stream;
        DevBuf<float> d_rows; DevBuf<long long> d_off; DevBuf<uint32_t> d_res;
        d_rows.alloc((size_t)off.back()); d_off.alloc(n_files + 1); d_res.alloc(n_files * F0_SEL_MANY_STRIDE);
        HIPCHK(hipMemcpyAsync(d_rows.get(), hz, (size_t)off.back() * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpy(d_off.get(), off.data(), (n_files + 1) * sizeof(long long), hipMemcpyHostToDevice));
        launch_f0_select_many(st, d_rows.get(), d_off.get(), n_files, quantile, (int)nq, d_res.get());
        std::vector<uint32_t> h(n_files * F0_SEL_MANY_STRIDE);
        HIPCHK(hipMemcpyAsync(h.data(), d_res.get(), h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        for (size_t f = 0; f < n_files; f++) {
            for (size_t i = 0; i < nq; i++) memcpy(&out_hz[f * nq + i], &h[f * F0_SEL_MANY_STRIDE + i], sizeof(float));
            if (voiced) voiced[f] = h[f * F0_SEL_MANY_STRIDE + F0_SEL_MAXQ];
        }
        return RVC_OK;
    });
}

}  // extern "C"
