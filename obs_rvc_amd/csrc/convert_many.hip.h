// convert_many.hip.h -- conversion of many recordings in one call (upstream's "model inference" tab, vc_multi), included by engine.hip:
// the entry points of the packed call.  The driver they share with rvc_convert is convert.hip.h's convert_windows_run, the kernels are windows.hip.h's gather
// and stitch.hip.h's pair; here are the call's own checks, the upload of the signals into one HBM arena with its tables and the download of the outputs per
// file, and the per-file pitch settings (section 31).
#pragma once
#include "convert.hip.h"

namespace rvc {

// statuses and arguments of rvc_convert_many, in the order the header documents; fills the packing and out_len[]
static rvc_status convert_many_check(rvc_engine *e, const float *const *pcm, const size_t *n, size_t n_files, size_t k, size_t context, size_t crossfade, float *const *out,
                                     const size_t *cap, size_t *out_len, ConvertManyGeometry *m)
{
    const rvc_status rc = convert_loaded(e);
    if (rc != RVC_OK) return rc;
    if (e->sy->sr <= 0 || e->sy->sr % 100 != 0) throw ShapeError("convert_many: the synthesizer's sample rate is not a multiple of 100");
    if (const char *why = convert_many_geometry(n, n_files, (size_t)e->sy->sr, k, context, crossfade, m)) throw ShapeError(why);
    if (e->sy->has_f0 && e->at_target > 0.0) throw ShapeError("convert_many: auto-transpose is in force; it takes one multiplier per recording (rvc_set_auto_transpose(e, 0, ..) or rvc_convert per file)");
    if (e->sy->has_f0 && e->curve_n > 0) throw ShapeError("convert_many: an f0 curve is set; a curve belongs to one recording (rvc_set_f0_curve(e, NULL, NULL, 0) or rvc_convert)");
    if (e->sy->has_f0 && !e->many_semitones.empty() && e->many_semitones.size() != n_files)
        throw ShapeError("convert_many: the per-file pitch list (rvc_set_convert_many_pitch) has " + std::to_string(e->many_semitones.size()) + " entries, the call " +
                         std::to_string(n_files) + " recordings");
    if (out_len) for (size_t f = 0; f < n_files; f++) out_len[f] = m->out_samples[f];
    for (size_t f = 0; f < n_files; f++)
        if (!cap || cap[f] < m->out_samples[f]) { e->err = "convert_many: output buffer " + std::to_string(f) + " too small"; return RVC_SHAPE; }
    if (!pcm || !out) throw ShapeError("convert_many: null buffer");
    for (size_t f = 0; f < n_files; f++) if (!pcm[f] || !out[f]) throw ShapeError("convert_many: null buffer");
    return RVC_OK;
}

// the call: every signal into one arena in one copy, the shared driver, the outputs down once per file.  No curve, no engine-wide auto-transpose, no f0 export
// (refused or out of scope); a per-file pitch (rvc_set_convert_many_pitch / _auto_transpose) gives every stream the factor of the file
// whose window it holds, and the guard takes the factors off the engine on every way out
static rvc_status convert_many_run(rvc_engine *e, const float *const *pcm, const ConvertManyGeometry &m, int32_t pitch_shift, bool highpass, float *const *out)
{
    hipStream_t st = e->stream;
    DevBuf<float> arena, d_out;
    ManyDeviceTables tabs;
    many_upload(pcm, m, &arena, &tabs);
    d_out.alloc(m.out_total());
    struct ManyMulGuard { rvc_engine *e; ~ManyMulGuard() { e->many_mul.clear(); } } mul_guard{e};
    const rvc_status rc = convert_windows_run(e, arena.get(), m, tabs.t, pitch_shift, highpass, d_out.get(), ConvertCall{"convert_many", &e->many, false, nullptr});
    if (rc != RVC_OK) return rc;
    for (size_t f = 0; f < m.files(); f++) HIPCHK(hipMemcpyAsync(out[f], d_out.get() + m.out_off[f], m.out_samples[f] * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return RVC_OK;
}

}  // namespace rvc

extern "C" {

// host only, pure: windows [F], out_samples [F] (either may be NULL), totals = {Wtot, sum of out_samples} (may be NULL)
rvc_status rvc_convert_many_geometry(const size_t *n16k, size_t n_files, size_t sample_rate, size_t k, size_t context, size_t crossfade, size_t *windows, size_t *out_samples,
                                     size_t totals[2])
{
    try {
        ConvertManyGeometry m;
        if (convert_many_geometry(n16k, n_files, sample_rate, k, context, crossfade, &m)) return RVC_SHAPE;
        for (size_t f = 0; f < n_files; f++) { if (windows) windows[f] = m.windows[f]; if (out_samples) out_samples[f] = m.out_samples[f]; }
        if (totals) { totals[0] = m.windows_total(); totals[1] = m.out_total(); }
        return RVC_OK;
    } catch (...) {
        return RVC_BACKEND;
    }
}

rvc_status rvc_convert_many(rvc_engine *e, const float *const *pcm16k, const size_t *n, size_t n_files, size_t k, size_t context, size_t crossfade, int32_t pitch_shift,
                            int highpass, float *const *out, const size_t *cap, size_t *out_len)
{
    return guarded(e, [&]() {
        ConvertManyGeometry m;
        const rvc_status rc = convert_many_check(e, pcm16k, n, n_files, k, context, crossfade, out, cap, out_len, &m);
        if (rc != RVC_OK) return rc;
        return convert_many_run(e, pcm16k, m, pitch_shift, highpass != 0, out);
    });
}

// of the last completed rvc_convert_many: the windows of all files, the batches, the SOLA offset of every window in global window order (the first
// cap_offsets of them), device ms = {high-pass, gather + model, stitch, total}; any pointer may be NULL
rvc_status rvc_convert_many_info(rvc_engine *e, size_t *windows_total, size_t *batches, int32_t *offsets, size_t cap_offsets, double ms[4])
{
    return guarded(e, [&]() {
        if (!e->many.valid) throw ShapeError("convert_many_info: no convert_many has completed on this engine");
        if (windows_total) *windows_total = e->many.windows;
        if (batches) *batches = e->many.batches;
        if (offsets) for (size_t i = 0; i < std::min(cap_offsets, e->many.offsets.size()); i++) offsets[i] = e->many.offsets[i];
        if (ms) for (int i = 0; i < 4; i++) ms[i] = e->many.ms[i];
        return RVC_OK;
    });
}

// the per-file pitch of rvc_convert_many: engine-wide, kept over model loads, read by rvc_convert_many alone.  A refused call changes nothing
rvc_status rvc_set_convert_many_pitch(rvc_engine *e, const double *semitones, size_t n_files)
{
    return guarded(e, [&]() {
        if (!semitones || n_files == 0) { e->many_semitones.clear(); return RVC_OK; }
        if (n_files > CONVERT_MANY_MAX_FILES) throw ShapeError("convert_many pitch: more than 65536 entries");
        for (size_t f = 0; f < n_files; f++)
            if (!(semitones[f] >= -24.0 && semitones[f] <= 24.0)) throw ShapeError("convert_many pitch: entry " + std::to_string(f) + " is outside [-24, 24] semitones");
        e->many_semitones.assign(semitones, semitones + n_files);
        return RVC_OK;
    });
}

rvc_status rvc_set_convert_many_auto_transpose(rvc_engine *e, double target_hz, int step, double limit)
{
    return guarded(e, [&]() {
        auto_transpose_check(target_hz, step, limit);
        e->many_at_target = target_hz; e->many_at_step = step; e->many_at_limit = limit;
        return RVC_OK;
    });
}

rvc_status rvc_convert_many_auto_transpose(rvc_engine *e, double *target_hz, int *step, double *limit)
{
    return guarded(e, [&]() {
        if (target_hz) *target_hz = e->many_at_target;
        if (step) *step = e->many_at_step;
        if (limit) *limit = e->many_at_limit;
        return RVC_OK;
    });
}

// of the last rvc_convert_many that ran the per-file pitch pass, per file (the first cap_files of them): the lower median, the voiced rows, a_f, t_f; device
// ms = {analysis, select}; any pointer may be NULL
rvc_status rvc_convert_many_pitch_info(rvc_engine *e, float *median_hz, size_t *voiced, double *auto_semitones, double *total_semitones, size_t cap_files, double ms[2])
{
    return guarded(e, [&]() {
        const rvc_engine::ManyPitchInfo &pi = e->many_pitch;
        if (!pi.valid) throw ShapeError("convert_many_pitch_info: no convert_many has run the per-file pitch pass on this engine");
        for (size_t f = 0; f < std::min(cap_files, pi.median.size()); f++) {
            if (median_hz) median_hz[f] = pi.median[f];
            if (voiced) voiced[f] = pi.voiced[f];
            if (auto_semitones) auto_semitones[f] = pi.a[f];
            if (total_semitones) total_semitones[f] = pi.t[f];
        }
        if (ms) { ms[0] = pi.ms[0]; ms[1] = pi.ms[1]; }
        return RVC_OK;
    });
}

// the per-file chained LINEAR rvc_sola_step over windows [Wtot][window_len] laid end to end, file f holding windows_per_file[f] >= 1 of them and every file's
// tail starting as zeros: out [Wtot][frame], offsets [Wtot] (may be NULL)
rvc_status rvc_sola_stitch_many(rvc_engine *e, const float *windows, const size_t *windows_per_file, size_t n_files, size_t window_len, size_t sola_len, size_t search, size_t frame,
                                float *out, int32_t *offsets)
{
    return guarded(e, [&]() {
        if (!windows || !out || !windows_per_file) throw ShapeError("sola_stitch_many: null buffer");
        if (n_files < 1 || n_files > CONVERT_MANY_MAX_FILES) throw ShapeError("sola_stitch_many: the number of files is outside [1, 65536]");
        if (search > 1023) throw ShapeError("sola_stitch_many: search range longer than 1023 samples");
        if (sola_len < 1 || frame < sola_len) throw ShapeError("sola_stitch_many: the frame must be at least as long as the crossfade (a window's tail is then its own samples)");
        if (window_len > (size_t)1 << 28 || window_len < search + frame + sola_len) throw ShapeError("sola_stitch_many: a window holds fewer than search + frame + sola_len samples");
        std::vector<int> P(n_files + 1, 0);
        size_t W = 0;
        for (size_t f = 0; f < n_files; f++) {
            if (windows_per_file[f] < 1 || windows_per_file[f] > (size_t)1 << 24) throw ShapeError("sola_stitch_many: a file's window count is out of range");
            W += windows_per_file[f];
            if (W > (size_t)1 << 24) throw ShapeError("sola_stitch_many: window count out of range");
            P[f + 1] = (int)W;
        }
        sola_stitch_run(e, windows, P, window_len, sola_len, search, frame, out, offsets);
        return RVC_OK;
    });
}

}  // extern "C"
