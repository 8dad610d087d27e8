// f0_analyze_many.hip.h -- the f0 of many recordings in one call, their order statistics in one launch, and the per-file pitch pass of rvc_convert_many
// (Applio's batch mode proposes a pitch per file), included by convert_many.hip.h (engine.hip's unit) behind its gather kernel.
//
// rvc_analyze_f0_many is rvc_analyze_f0 of every file, packed as rvc_convert_many packs its windows: global window order, S = rvc_set_streams per batch through
// ONE pitch-only plan (PlanKey::mode 2, B = S) under the neutral control block, only the last batch padded.  The rows go to a grid arena: file f's Nf_f rows at
// goff[f], the prefix sums of Nf_f (convert_many_geometry.h grid_off / many_grid_row), zeroed once so that the rows of windows the silence gate skips are 0.
// rvc_f0_stats_many is rvc_f0_stats of every file's rows in one launch (f0_select_many.hip.h).  many_pitch_run strings the two together in front of
// rvc_convert_many's first batch: analysis, lower median per file, the medians and counts down in one copy, the transpose of every file on the host in double.
#pragma once
#include "convert_many_geometry.h"
#include "f0_select_many.hip.h"

namespace rvc {

// f0_export_kernel for a packed batch: hop rows [C, C + H) of stream s = global window g (j0 + s, or win_of[j0 + s] under the silence gate) = window w of file
// f go to rows [w H, min((w + 1) H, Nf_f)) of that file's region of the arena -- the last, partial hop of a file stops at its own end.  Streams at or beyond nw
// (the padding of the call's last batch) write nothing.  Grid (ceil(H / 256), S)
static __global__ __launch_bounds__(256) void f0_export_many_kernel(const float *__restrict__ f0, int Tm, const int *__restrict__ P, const long long *__restrict__ goff, int n_files,
                                                                    const int *__restrict__ win_of, int j0, int nw, int H, int C, float *__restrict__ grid)
{
    const int h = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (h >= H || C + h >= Tm || s >= nw) return;
    const int g = win_of ? win_of[j0 + s] : j0 + s;
    const long long at = many_grid_row(P, goff, n_files, g, h, H);
    if (at >= 0) grid[at] = f0[(long long)s * Tm + C + h];
}

// analyze_run for a packed call, device to device: sig = the signal arena, tabs its tables, d_goff [F + 1] the grid arena's offsets on the device, grid the arena,
// zeroed by the caller.  Begins with what rvc_reset_state does; returns synchronised, the streams' status words checked.  gate: only its active windows run
static rvc_status analyze_many_run(rvc_engine *e, const float *sig, const ConvertManyGeometry &m, const ManyTables &tabs, const long long *d_goff, float *grid,
                                   const SilenceWork *gate)
{
    hipStream_t st = e->stream;
    const ConvertGeometry &g = m.g;
    const size_t S = (size_t)e->n_streams, W = m.windows_total(), N = gate ? gate->A : W, batches = (N + S - 1) / S;
    const int Cg = analyze_cg(g);
    HIPCHK(hipDeviceSynchronize());
    reset_state(e);
    if (N == 0) { HIPCHK(hipStreamSynchronize(st)); return RVC_OK; }      // (a gated call without an active window: no plan is built, the zeroed arena is the result)
    Plan *pl = get_plan(e, plan_key(e, 2, g.n, g.sf, 0, 0));
    if (pl->key.B != (int)S || !pl->d_f0 || (size_t)Cg + g.H > (size_t)pl->Tm) throw ShapeError("analyze_f0_many: a window's hop lies outside its f0 rows");
    pl->cur_in = nullptr; pl->cur_out = nullptr;
    push_call_params(e, 0, nullptr, nullptr, true);
    for (size_t b = 0; b < batches; b++) {
        const size_t g0 = b * S; const int nw = (int)std::min(S, N - g0);      // (gated: g0 is the batch's first place)
        if (gate) gate->gather(st, sig, tabs, pl->d_in, S, g0, g);
        else hipLaunchKernelGGL(window_gather_many_kernel, dim3((unsigned)((g.n + 255) / 256), (unsigned)S), dim3(256), 0, st, sig, tabs, pl->d_in, (int)g.n, (int)g0, nw, (int)g.H,
                                (int)g.C);
        run_plan(e, *pl);
        hipLaunchKernelGGL(f0_export_many_kernel, dim3((unsigned)((g.H + 255) / 256), (unsigned)S), dim3(256), 0, st, (const float *)pl->d_f0, pl->Tm, tabs.P, d_goff, tabs.n_files,
                           gate ? (const int *)gate->win_of.get() : (const int *)nullptr, (int)g0, nw, (int)g.H, Cg, grid);
    }
    queue_status(e);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return final_status(e);
}

// the signal arena of a call and its tables on the device, copied before it returns (rvc_convert_many's step 1)
static void many_upload(const float *const *pcm, const ConvertManyGeometry &m, DevBuf<float> *arena, ManyDeviceTables *tabs)
{
    const size_t F = m.files();
    std::vector<float> stage(m.sig_total());
    for (size_t f = 0; f < F; f++) memcpy(stage.data() + m.sig_off[f], pcm[f], m.n[f] * sizeof(float));
    arena->alloc(m.sig_total());
    HIPCHK(hipMemcpy(arena->get(), stage.data(), stage.size() * sizeof(float), hipMemcpyHostToDevice));
    std::vector<long long> sig_n(F), out_n(F);
    for (size_t f = 0; f < F; f++) { sig_n[f] = (long long)m.n[f]; out_n[f] = (long long)m.out_samples[f]; }
    tabs->upload(m.P, m.sig_off, sig_n, m.out_off, out_n);
}

// the silence gate over the files of a call: every file measured on its own, the active windows of all files compacted in global window order (synchronises)
static void many_gate(rvc_engine *e, const float *sig, const ConvertManyGeometry &m, size_t zero_len, SilenceWork *gate)
{
    hipStream_t st = e->stream;
    size_t frames = 0;
    for (size_t f = 0; f < m.files(); f++) frames += m.out_samples[f] / m.g.zc;
    gate->begin(st, frames, m.windows_total(), e->sil_db, e->sil_hang, zero_len);
    size_t at = 0;
    for (size_t f = 0; f < m.files(); f++) {
        const size_t Nf = m.out_samples[f] / m.g.zc;
        gate->queue_file(st, sig + m.sig_off[f], m.n[f], Nf, at, m.windows[f], (size_t)m.P[f], m.g);
        at += Nf;
    }
    gate->finish(st);
}

// In front of rvc_convert_many's first batch (a per-file setting is on and the model has pitch guidance): the analysis of the signals the model will see, the lower
// median m_f of every file, t_f = semitones[f] + a_f with a_f = auto_transpose_semitones(target, m_f, v_f, ..) (0 with the target off or no voiced row).
// -> mul [F]: the factor (float)2^(t_f / 12) the streams that hold a window of file f take, 0 = none.  Ends with the engine in the reset state the conversion starts from
static rvc_status many_pitch_run(rvc_engine *e, const float *sig, const ConvertManyGeometry &m, const ManyTables &tabs, const SilenceWork *gate, std::vector<float> *mul)
{
    hipStream_t st = e->stream;
    const size_t F = m.files();
    e->many_pitch.valid = false;
    const std::vector<long long> goff = m.grid_off();
    DevBuf<float> grid; DevBuf<long long> d_goff; DevBuf<uint32_t> res;
    grid.alloc((size_t)goff.back()); d_goff.alloc(F + 1); res.alloc(F * F0_SEL_MANY_STRIDE);
    HIPCHK(hipMemcpy(d_goff.get(), goff.data(), (F + 1) * sizeof(long long), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(grid.get(), 0, (size_t)goff.back() * sizeof(float), st));
    DevTimer t_an, t_sel;
    t_an.start(st);
    const rvc_status rc = analyze_many_run(e, sig, m, tabs, d_goff.get(), grid.get(), gate);
    if (rc != RVC_OK) return rc;
    t_an.stop(st);
    t_sel.start(st);
    const double half = 0.5;
    launch_f0_select_many(st, grid.get(), d_goff.get(), F, &half, 1, res.get());
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
        DevBuf<float> arena, filtered, grid; DevBuf<long long> d_goff;
        ManyDeviceTables tabs;
        many_upload(pcm16k, m, &arena, &tabs);
        const float *sig = arena.get();
        if (highpass) {      // each file on its own: rvc_highpass's bits
            filtered.alloc(m.sig_total());
            for (size_t f = 0; f < F; f++) launch_highpass(e, arena.get() + m.sig_off[f], m.n[f], filtered.get() + m.sig_off[f]);
            sig = filtered.get();
        }
        const bool gated = silence_gate_on(e);
        SilenceWork gate;
        if (gated) many_gate(e, sig, m, 0, &gate);
        grid.alloc((size_t)goff.back()); d_goff.alloc(F + 1);
        HIPCHK(hipMemcpy(d_goff.get(), goff.data(), (F + 1) * sizeof(long long), hipMemcpyHostToDevice));
        HIPCHK(hipMemsetAsync(grid.get(), 0, (size_t)goff.back() * sizeof(float), st));
        const rvc_status rc = analyze_many_run(e, sig, m, tabs.t, d_goff.get(), grid.get(), gated ? &gate : nullptr);
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
