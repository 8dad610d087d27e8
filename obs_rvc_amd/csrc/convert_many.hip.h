// convert_many.hip.h -- conversion of many recordings in one call (upstream's "model inference" tab, vc_multi), included by engine.hip
// behind convert.hip.h.
//
// The F recordings share one window geometry; their windows are laid end to end (convert_many_geometry.h: global window g = P_f + w) and run S at a time
// through infer_common, so a batch holds the windows of several files and only the last batch of the CALL is padded.  The signals lie in one HBM arena
// with an offset table, the outputs in another; per batch one gather launch, one infer call with its one synchronisation, two stitch launches, as in
// convert_run.  The stitch keeps one offset chain per FILE: the chains of the files of a batch run side by side, one workgroup each.
//   tabs     the device tables of a call, all indexed by file: P [F + 1] window prefix sums, sig_off / sig_n the file's place in the signal arena,
//            out_off / out_n its place in the output arena
//   tails    [Wtot + 1][sola_len]   row 0 stays zero: what the FIRST window of every file is correlated and blended with; row g + 1 = the tail global
//            window g leaves, which window g + 1 reads if it belongs to the same file
//   offsets  [Wtot], in global window order
#pragma once
#include "convert_many_geometry.h"
#include "stitch.hip.h"
#include "highpass.hip.h"
#include "silence.hip.h"

namespace rvc {

// (ManyTables, the device tables of a call, and ManyDeviceTables, their upload: silence.hip.h, whose gated kernels read the same tables)

// the plan's batch input [S][n]: stream s gets global window g0 + s = window w of file f, samples [160 (w H - C), + n) of THAT file, zero outside [0, N_f)
// -- a sample of the neighbour file in the arena is never read; streams at or beyond nw (the padding of the call's last batch) get zeros
static __global__ __launch_bounds__(256) void window_gather_many_kernel(const float *sig, ManyTables tabs, float *dst, int n, int g0, int nw, int H, int C)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (i >= n) return;
    float v = 0.f;
    if (s < nw) {
        const int g = g0 + s, f = many_file_of(tabs.P, tabs.n_files, g), w = g - tabs.P[f];
        const long long src = 160LL * ((long long)w * H - C) + i;
        if (src >= 0 && src < tabs.sig_n[f]) v = sig[tabs.sig_off[f] + src];
    }
    dst[(long long)s * n + i] = v;
}

// Offset chains: workgroup b walks the windows file f_first + b has among globals [g0, g0 + nw), in order, as stitch_chain_kernel walks a file's; y [nw][y_bs]
// holds the batch's model outputs (global g at y + (g - g0) y_bs).  A file's first window meets the zero tail (row 0), a window that continues a file from
// the batch before meets the row that batch left behind.  Workgroups touch disjoint rows of tails and offsets.  search <= 1023 (the LDS array).
static __global__ __launch_bounds__(STITCH_CHAIN_THREADS) void stitch_chain_many_kernel(const float *y, long long y_bs, int g0, int nw, int f_first, ManyTables tabs, int sola_len,
                                                                                        int search, int frame, float *tails, int *offsets)
{
    __shared__ float cor[1024];
    __shared__ int s_off;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int f = f_first + blockIdx.x;
    if (f >= tabs.n_files) return;
    const int p0 = tabs.P[f], lo = max(p0, g0), hi = min(tabs.P[f + 1], g0 + nw);
    for (int g = lo; g < hi; g++) {
        const float *yw = y + (long long)(g - g0) * y_bs;
        const float *prev = g == p0 ? tails : tails + (long long)g * sola_len;
        float *next = tails + (long long)(g + 1) * sola_len;
        for (int l = wave; l <= search; l += STITCH_CHAIN_THREADS / 64) {
            const float c = sola_corr_lag(yw + l, prev, sola_len, lane);
            if (lane == 0) cor[l] = c;
        }
        __syncthreads();
        if (t == 0) { const int best = sola_argmax_last(cor, search); s_off = best; offsets[g] = best; }
        __syncthreads();
        const float *o = yw + s_off;
        for (int i = t; i < sola_len; i += STITCH_CHAIN_THREADS) next[i] = o[frame + i];
        // the file's next window reads `next` (global memory written by this workgroup) and overwrites cor / s_off
        __threadfence_block();
        __syncthreads();
    }
}

// Assembly: grid (tiles of a frame, nw).  Global window g = g0 + blockIdx.y = window w of file f: its `frame` samples from its offset on, the first sola_len
// of them blended with the tail in front of it by the sin^2 fade, written to out[out_off[f] + w frame ..); samples at or beyond out_n[f] (the file's last,
// partial hop) are not written, so nothing lands in the next file's region
static __global__ __launch_bounds__(256) void stitch_assemble_many_kernel(const float *y, long long y_bs, int g0, ManyTables tabs, int sola_len, int frame, const float *tails,
                                                                          const int *offsets, float *out)
{
    const int j = blockIdx.y, g = g0 + j, f = many_file_of(tabs.P, tabs.n_files, g), w = g - tabs.P[f];
    const float *o = y + (long long)j * y_bs + offsets[g];
    const float *prev = w == 0 ? tails : tails + (long long)g * sola_len;
    const long long base = (long long)w * frame, n_out = tabs.out_n[f];
    float *dst = out + tabs.out_off[f];
    const int i0 = blockIdx.x * STITCH_TILE;
    for (int i = i0 + threadIdx.x; i < i0 + STITCH_TILE && i < frame; i += 256) {
        if (base + i >= n_out) break;
        dst[base + i] = i < sola_len ? sola_fade(o[i], prev[i], i, sola_len) : o[i];
    }
}

// the two stitch launches for globals [g0, g0 + nw), which lie in files [f_first, f_last]
static void launch_stitch_many(hipStream_t st, const float *y, long long y_bs, int g0, int nw, int f_first, int f_last, const ManyTables &tabs, int sola_len, int search, int frame,
                               float *tails, int *offsets, float *out)
{
    hipLaunchKernelGGL(stitch_chain_many_kernel, dim3((unsigned)(f_last - f_first + 1)), dim3(STITCH_CHAIN_THREADS), 0, st, y, y_bs, g0, nw, f_first, tabs, sola_len, search, frame,
                       tails, offsets);
    hipLaunchKernelGGL(stitch_assemble_many_kernel, dim3((unsigned)((frame + STITCH_TILE - 1) / STITCH_TILE), (unsigned)nw), dim3(256), 0, st, y, y_bs, g0, tabs, sola_len, frame,
                       (const float *)tails, (const int *)offsets, out);
}

}  // namespace rvc
#include "f0_analyze_many.hip.h"
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

// the conversion proper.  Begins with what rvc_reset_state does, as convert_run; no curve, no engine-wide auto-transpose, no f0 export (refused or out of scope).
// A per-file pitch (rvc_set_convert_many_pitch / _auto_transpose) runs many_pitch_run in front of the first batch and gives every stream
// the factor of the file whose window it holds, batch by batch; with both off nothing is queued for it
static rvc_status convert_many_run(rvc_engine *e, const float *const *pcm, const ConvertManyGeometry &m, int32_t pitch_shift, bool highpass, float *const *out)
{
    hipStream_t st = e->stream;
    const ConvertGeometry &g = m.g;
    const size_t F = m.files(), S = (size_t)e->n_streams, W = m.windows_total();
    size_t batches = m.batches(S);
    const bool gated = silence_gate_on(e);
    const size_t sola_len = g.X * g.zc, search = g.Q * g.zc, frame = g.H * g.zc, ylen = g.return_length * g.zc;
    e->conv.valid = false; e->conv_f0_valid = false; e->many.valid = false;
    HIPCHK(hipDeviceSynchronize());
    reset_state(e);
    // 1. every signal into one arena, one copy
    std::vector<float> stage(m.sig_total());
    for (size_t f = 0; f < F; f++) memcpy(stage.data() + m.sig_off[f], pcm[f], m.n[f] * sizeof(float));
    DevBuf<float> arena, filtered, d_out;
    arena.alloc(m.sig_total()); d_out.alloc(m.out_total());
    HIPCHK(hipMemcpyAsync(arena.get(), stage.data(), stage.size() * sizeof(float), hipMemcpyHostToDevice, st));
    ManyDeviceTables tabs;
    {
        std::vector<long long> sig_n(F), out_n(F);
        for (size_t f = 0; f < F; f++) { sig_n[f] = (long long)m.n[f]; out_n[f] = (long long)m.out_samples[f]; }
        tabs.upload(m.P, m.sig_off, sig_n, m.out_off, out_n);
    }
    DevTimer t_total, t_hp;
    t_total.start(st);
    const float *sig = arena.get();
    if (highpass) {      // each file on its own: rvc_highpass's bits, the zero extension per file
        filtered.alloc(m.sig_total());
        t_hp.start(st);
        for (size_t f = 0; f < F; f++) launch_highpass(e, arena.get() + m.sig_off[f], m.n[f], filtered.get() + m.sig_off[f]);
        t_hp.stop(st);
        sig = filtered.get();
    }
    // the silence gate (silence.hip.h): every file measured on its own, the active windows of all files compacted in global window order
    SilenceWork gate;
    if (gated) {
        many_gate(e, sig, m, ylen, &gate);
        batches = gate.batches(S);
    }
    // the per-file pitch: file_mul[f] = (float)2^(t_f / 12), 0 = none; under the gate the file of a stream is the file of the window win_of names
    struct ManyMulGuard { rvc_engine *e; ~ManyMulGuard() { e->many_mul.clear(); } } mul_guard{e};
    const bool per_file = e->sy->has_f0 && (!e->many_semitones.empty() || e->many_at_target > 0.0);
    std::vector<float> file_mul; std::vector<int> win_of;
    if (per_file) {
        const rvc_status rc = many_pitch_run(e, sig, m, tabs.t, gated ? &gate : nullptr, &file_mul);
        if (rc != RVC_OK) { (void)hipStreamSynchronize(st); return rc; }
        if (gated && gate.A) { win_of.resize(gate.A); HIPCHK(hipMemcpy(win_of.data(), gate.win_of.get(), gate.A * sizeof(int), hipMemcpyDeviceToHost)); }
    }
    DevBuf<float> win, y, tails; DevBuf<int> offs;
    win.alloc(S * g.n + 64); y.alloc(S * ylen + 64); tails.alloc((W + 1) * sola_len); offs.alloc(W);
    HIPCHK(hipMemsetAsync(win.get(), 0, (S * g.n + 64) * sizeof(float), st));
    HIPCHK(hipMemsetAsync(tails.get(), 0, sola_len * sizeof(float), st));       // row 0: every file's stitch starts from silence
    std::vector<DevEvent> ev(3 * batches);
    for (size_t b = 0; b < batches; b++) {
        // (gated: g0 is the batch's first PLACE and nw its active windows, of the A in all)
        const size_t g0 = b * S; const int nw = (int)std::min(S, (gated ? gate.A : W) - g0);
        int f_first = 0, f_last = 0;
        if (!gated) m.batch_files(b, S, &f_first, &f_last);
        ev[3 * b].record(st);
        if (gated) gate.gather(st, sig, tabs.t, win.get(), S, g0, g);
        else hipLaunchKernelGGL(window_gather_many_kernel, dim3((unsigned)((g.n + 255) / 256), (unsigned)S), dim3(256), 0, st, sig, tabs.t, win.get(), (int)g.n, (int)g0, nw, (int)g.H,
                           (int)g.C);
        if (per_file) {
            e->many_mul.assign(S, 0.f);
            for (int s = 0; s < nw; s++) e->many_mul[s] = file_mul[many_file_of(m.P.data(), (int)F, gated ? win_of[g0 + s] : (int)(g0 + s))];
        }
        size_t got = 0;
        const rvc_status rc = infer_common(e, win.get(), true, g.n, g.sf, pitch_shift, (uint32_t)g.skip_head, (uint32_t)g.return_length, y.get(), true, ylen, &got, true);
        if (rc != RVC_OK) { (void)hipStreamSynchronize(st); return rc; }
        if (got != ylen) throw ShapeError("convert_many: the synthesizer does not produce sample_rate / 100 samples per frame");
        ev[3 * b + 1].record(st);
        if (gated) gate.stitch(st, y.get(), (long long)ylen, g0, nw, tabs.t, (int)sola_len, (int)search, (int)frame, tails.get(), offs.get(), d_out.get());
        else launch_stitch_many(st, y.get(), (long long)ylen, (int)g0, nw, f_first, f_last, tabs.t, (int)sola_len, (int)search, (int)frame, tails.get(), offs.get(), d_out.get());
        ev[3 * b + 2].record(st);
    }
    DevTimer t_zero;      // a gated call without an active window: no batch ran; the stitch walks zeros, as in convert_run
    if (gated && batches == 0) {
        t_zero.start(st);
        gate.stitch(st, y.get(), (long long)ylen, 0, 0, tabs.t, (int)sola_len, (int)search, (int)frame, tails.get(), offs.get(), d_out.get());
        t_zero.stop(st);
    }
    t_total.stop(st);
    // 5. the outputs come down once, per file
    e->many.offsets.assign(W, 0);
    HIPCHK(hipMemcpyAsync(e->many.offsets.data(), offs.get(), W * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    for (size_t f = 0; f < F; f++) HIPCHK(hipMemcpyAsync(out[f], d_out.get() + m.out_off[f], m.out_samples[f] * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    double ms_model = 0, ms_stitch = 0;
    for (size_t b = 0; b < batches; b++) {
        float a = 0.f, c = 0.f;
        HIPCHK(hipEventElapsedTime(&a, ev[3 * b].get(), ev[3 * b + 1].get())); HIPCHK(hipEventElapsedTime(&c, ev[3 * b + 1].get(), ev[3 * b + 2].get()));
        ms_model += a; ms_stitch += c;
    }
    if (gated && batches == 0) ms_stitch = (double)t_zero.ms();
    if (gated) silence_gate_report(e, gate);
    e->many.windows = W; e->many.batches = batches;
    e->many.ms[0] = highpass ? (double)t_hp.ms() : 0.0; e->many.ms[1] = ms_model; e->many.ms[2] = ms_stitch; e->many.ms[3] = (double)t_total.ms();
    e->many.valid = true;
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
    return guarded(e, [&]() {      // (rvc_set_auto_transpose's checks)
        if (!(target_hz >= 0.0 && target_hz <= 20000.0)) throw ShapeError("auto transpose: the target is 0 (off) or in (0, 20000] Hz");
        if (step != 0 && step != 1 && step != 12) throw ShapeError("auto transpose: the step is 0 (exact), 1 (semitones) or 12 (octaves)");
        if (!(limit >= 0.0 && limit <= 24.0)) throw ShapeError("auto transpose: the limit is in [0, 24] semitones");
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
        std::vector<long long> zero(n_files, 0), out_off(n_files), out_n(n_files);
        size_t W = 0;
        for (size_t f = 0; f < n_files; f++) {
            if (windows_per_file[f] < 1 || windows_per_file[f] > (size_t)1 << 24) throw ShapeError("sola_stitch_many: a file's window count is out of range");
            out_off[f] = (long long)(W * frame); out_n[f] = (long long)(windows_per_file[f] * frame);
            W += windows_per_file[f];
            if (W > (size_t)1 << 24) throw ShapeError("sola_stitch_many: window count out of range");
            P[f + 1] = (int)W;
        }
        hipStream_t st = e->stream;
        DevBuf<float> d_y, d_tails, d_out; DevBuf<int> d_off;
        d_y.alloc(W * window_len); d_tails.alloc((W + 1) * sola_len); d_out.alloc(W * frame); d_off.alloc(W);
        ManyDeviceTables tabs;
        tabs.upload(P, zero, zero, out_off, out_n);
        HIPCHK(hipMemcpyAsync(d_y.get(), windows, W * window_len * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(d_tails.get(), 0, sola_len * sizeof(float), st));
        const size_t step = 4096;      // windows per pair of launches (the assembly's grid.y; at most as many files, the chain's grid.x)
        for (size_t g0 = 0; g0 < W; g0 += step) {
            const size_t nw = std::min(step, W - g0);
            const int f_first = many_file_of(P.data(), (int)n_files, (int)g0), f_last = many_file_of(P.data(), (int)n_files, (int)(g0 + nw - 1));
            launch_stitch_many(st, d_y.get() + g0 * window_len, (long long)window_len, (int)g0, (int)nw, f_first, f_last, tabs.t, (int)sola_len, (int)search, (int)frame, d_tails.get(),
                               d_off.get(), d_out.get());
        }
        std::vector<int32_t> off(W);
        HIPCHK(hipMemcpyAsync(out, d_out.get(), W * frame * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(off.data(), d_off.get(), W * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        if (offsets) for (size_t i = 0; i < W; i++) offsets[i] = off[i];
        return RVC_OK;
    });
}

}  // extern "C"
