// convert.hip.h -- conversion of a whole recording (upstream's "model inference" tab, vc_single), included by engine.hip.
//
// The recording is cut into windows of ONE geometry (convert_geometry.h), so one plan serves the whole file; the windows run S at a time through
// infer_common on the engine's S streams (window w = i S + s on stream s in batch i) and are stitched by the plugin's SOLA step in its LINEAR crossfade,
// chained over the windows on the device (stitch.hip.h).  In front of it the optional 48 Hz high-pass (highpass.hip.h).  Per batch: one gather launch,
// one infer call with its one synchronisation, two stitch launches; the signal, S window inputs, S window outputs, the tails and the output stay in HBM.
#pragma once
#include "convert_geometry.h"
#include "highpass.hip.h"
#include "stitch.hip.h"

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

// the two stitch launches for windows [w0, w0 + nw) whose outputs lie in y [nw][y_bs]
static void launch_stitch(hipStream_t st, const float *y, long long y_bs, int w0, int nw, int sola_len, int search, int frame, float *tails, int *offsets, float *out, long long n_out)
{
    hipLaunchKernelGGL(stitch_chain_kernel, dim3(1), dim3(STITCH_CHAIN_THREADS), 0, st, y, y_bs, w0, nw, sola_len, search, frame, tails, offsets);
    hipLaunchKernelGGL(stitch_assemble_kernel, dim3((unsigned)((frame + STITCH_TILE - 1) / STITCH_TILE), (unsigned)nw), dim3(256), 0, st, y, y_bs, w0, sola_len, frame,
                       (const float *)tails, (const int *)offsets, out, n_out);
}

// statuses and arguments of rvc_convert / rvc_convert_device, in the order the header documents; fills the geometry and *out_len
static rvc_status convert_check(rvc_engine *e, const void *pcm, size_t n, size_t k, size_t context, size_t crossfade, const void *out, size_t cap, size_t *out_len, ConvertGeometry *g)
{
    if (!e->sy) return RVC_MODEL_NOT_LOADED;
    if (!e->cv) return RVC_CONTENTVEC_NOT_LOADED;
    if (!e->f0_method) return RVC_F0_NOT_LOADED;
    if (n == 0) throw ShapeError("convert: empty recording");
    if (e->sy->sr <= 0 || e->sy->sr % 100 != 0) throw ShapeError("convert: the synthesizer's sample rate is not a multiple of 100");
    if (const char *why = convert_geometry(n, (size_t)e->sy->sr, k, context, crossfade, g)) throw ShapeError(why);
    if (g->windows > (size_t)1 << 30 || g->out_samples > (size_t)1 << 40) throw ShapeError("convert: recording too long");
    if (out_len) *out_len = g->out_samples;
    if (cap < g->out_samples) { e->err = "convert: output buffer too small"; return RVC_SHAPE; }
    if (!pcm || !out) throw ShapeError("convert: null buffer");
    return RVC_OK;
}

// the conversion proper, device to device.  Begins with what rvc_reset_state does (pitch caches and chunk counters zeroed), so that a window's result depends
// on the recording alone; every per-stream setting, the index, the f0 method and graph replay apply as to any infer call
static rvc_status convert_run(rvc_engine *e, const float *d_pcm, size_t n, const ConvertGeometry &g, int32_t pitch_shift, bool highpass, float *d_out)
{
    hipStream_t st = e->stream;
    const size_t S = (size_t)e->n_streams, W = g.windows, batches = (W + S - 1) / S;
    const size_t sola_len = g.X * g.zc, search = g.Q * g.zc, frame = g.H * g.zc, ylen = g.return_length * g.zc;
    e->conv.valid = false;
    HIPCHK(hipDeviceSynchronize());
    reset_state(e);
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
    DevBuf<float> win, y, tails; DevBuf<int> offs;
    win.alloc(S * g.n + 64); y.alloc(S * ylen + 64); tails.alloc((W + 1) * sola_len); offs.alloc(W);
    HIPCHK(hipMemsetAsync(win.get(), 0, (S * g.n + 64) * sizeof(float), st));
    HIPCHK(hipMemsetAsync(tails.get(), 0, sola_len * sizeof(float), st));       // tails[0]: the stitch starts from silence
    std::vector<DevEvent> ev(3 * batches);
    for (size_t b = 0; b < batches; b++) {
        const size_t w0 = b * S; const int nw = (int)std::min(S, W - w0);
        ev[3 * b].record(st);
        hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)((g.n + 255) / 256), (unsigned)S), dim3(256), 0, st, sig, (long long)n, win.get(), (int)g.n, (long long)w0, nw,
                           (int)g.H, (int)g.C);
        size_t got = 0;
        const rvc_status rc = infer_common(e, win.get(), true, g.n, g.sf, pitch_shift, (uint32_t)g.skip_head, (uint32_t)g.return_length, y.get(), true, ylen, &got, true);
        if (rc != RVC_OK) return rc;
        if (got != ylen) throw ShapeError("convert: the synthesizer does not produce sample_rate / 100 samples per frame");
        ev[3 * b + 1].record(st);
        launch_stitch(st, y.get(), (long long)ylen, (int)w0, nw, (int)sola_len, (int)search, (int)frame, tails.get(), offs.get(), d_out, (long long)g.out_samples);
        ev[3 * b + 2].record(st);
    }
    t_total.stop(st);
    e->conv.offsets.assign(W, 0);
    HIPCHK(hipMemcpyAsync(e->conv.offsets.data(), offs.get(), W * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    double ms_model = 0, ms_stitch = 0;
    for (size_t b = 0; b < batches; b++) {
        float a = 0.f, c = 0.f;
        HIPCHK(hipEventElapsedTime(&a, ev[3 * b].get(), ev[3 * b + 1].get())); HIPCHK(hipEventElapsedTime(&c, ev[3 * b + 1].get(), ev[3 * b + 2].get()));
        ms_model += a; ms_stitch += c;
    }
    e->conv.windows = W; e->conv.batches = batches;
    e->conv.ms[0] = highpass ? (double)t_hp.ms() : 0.0; e->conv.ms[1] = ms_model; e->conv.ms[2] = ms_stitch; e->conv.ms[3] = (double)t_total.ms();
    e->conv.valid = true;
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
