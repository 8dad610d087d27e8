// session.hip.h -- the plugin's per-chunk state machine `process_one_frame` (obs-rvc/src/lib.rs:659-795, geometry from
// lib.rs:200-227) as ONE native call with every buffer resident in HBM (SURVEY.md section 8 rows f1-f3 chained), included by engine.hip.
//
// The reference moves each chunk host -> rubato -> pipe -> ONNX Runtime -> pipe -> rubato -> envelope -> SOLA -> host.  Here the
// host-rate ring, the 16 kHz ring, the model output, both resampler states and the SOLA tail live on the device and the chunk
// costs one H2D copy (the new samples), one D2H copy (the finished frame) and one stream synchronisation; everything else is
// queued on the engine's stream:
//   shift+append (ping-pong ring) -> polyphase downsampler -> 16 kHz ring update -> infer plan -> polyphase upsampler
//   -> RMS envelope mixing -> SOLA search / crossfade / tail save.
// Two per-stream stages of this project's own (crossfade.hip.h, DESIGN.md "Phase-vocoder crossfade and input gate"), both off by default: the input
// gate in front of shift+append and the phase-vocoder blend (analysis + synthesis launches) behind the SOLA search.
// Spectral-gate noise reduction (denoise.hip.h, DESIGN.md "Spectral-gate noise reduction"), per stream and per side, off by default: the input side
// sits between the input gate and shift+append, the output side behind the SOLA / phase-vocoder launches on the finished frame.  Each side owns
// a denoiser that is created the first time a stream switches the side on and is not launched before that.
#pragma once

namespace rvc {

// out[i] = i < n - f ? in[i + f] : chunk[i - (n - f)]        (lib.rs:661-665 "move and append the last n samples")
// (blockIdx.y = stream; rings are [streams][n], chunks [streams][f])
__global__ void ring_shift_append_kernel(const float *in, float *out, int n, int f, const float *chunk)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    in += (long long)blockIdx.y * n; out += (long long)blockIdx.y * n; chunk += (long long)blockIdx.y * f;
    if (i < n) out[i] = i < n - f ? in[i + f] : chunk[i - (n - f)];
}

// 16 kHz ring (lib.rs:669-679): shift by f, then overwrite [copy_begin, n) with res[skip ..] (copy_begin = n - f - skip: the
// converter's output re-writes the `skip` samples before the new chunk as well)
__global__ void ring16_update_kernel(const float *in, float *out, int n, int f, const float *res, int skip, int copy_begin, long long res_bs)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    in += (long long)blockIdx.y * n; out += (long long)blockIdx.y * n; res += blockIdx.y * res_bs;
    if (i < n) out[i] = i >= copy_begin ? res[skip + i - copy_begin] : in[i + f];
}

}  // namespace rvc

using namespace rvc;

struct rvc_session {
    rvc_engine *e = nullptr;
    // lib.rs:200-227
    int sample_rate = 0, zc = 0, sample_frame_size = 0, sample_frame_16k = 0, crossfade_frame_size = 0, sola_buffer_frame_size = 0,
        sola_search_frame_size = 0, extra_frame_size = 0, input_buffer_size = 0, input_buffer_16k_size = 0, model_return_length = 0,
        model_return_size = 0, skip_head = 0, model_rate = 0, up_out = 0;
    bool skip_inference = false;
    // per-stream settings (every stream is a caller of its own, obs-rvc/src/lib.rs:701-707, 174-185): pitch shift and RMS mix rate
    std::vector<int32_t> pitch_shift; std::vector<double> rms_mix_rate; float *d_mixpow = nullptr; bool mix_dirty = true;
    rvc_resampler *down = nullptr, *up = nullptr;
    float *d_in[2] = {nullptr, nullptr}, *d_in16[2] = {nullptr, nullptr};
    int par = 0, par16 = 0;
    float *d_chunk = nullptr, *d_down = nullptr, *d_model = nullptr, *d_up = nullptr, *d_sola = nullptr, *d_frame = nullptr, *d_cor = nullptr;
    int *d_off = nullptr; int n_rms = 0; double *d_rms = nullptr;      // the two RMS tracks of envelope mixing, [B][2][n_rms] in f64
    int B = 1;                     // streams (= the engine's stream count at creation); every buffer below has a leading [B] axis
    std::vector<int> h_off;
    // crossfade mode per stream (RVC_CROSSFADE_*); the phase-vocoder buffers exist when the seam fits its kernels (sola_buffer_frame_size <= PV_MAX_N)
    std::vector<int> xfade; int *d_xfade = nullptr; bool xfade_dirty = false; int n_pv = 0;
    float *d_pva = nullptr, *d_pvtab = nullptr, *d_pvspec = nullptr;
    // input gate: threshold per stream (-inf = off), the ungated history (ping-pong) and the gated chunk.  The stage is launched from the first
    // time any stream's gate is switched on; until then the history is the zeros of creation
    std::vector<float> gate_thr; float *d_gate_thr = nullptr, *d_hist[2] = {nullptr, nullptr}, *d_gated = nullptr; bool gate_dirty = false, gate_used = false; int par_h = 0;
    // noise reduction, [RVC_DENOISE_INPUT | RVC_DENOISE_OUTPUT]: the settings per stream, the side's denoiser (null until a stream switches the side on) and
    // the buffer it writes (the denoised chunk in front of the ring / the denoised frame that is copied to the host)
    std::vector<double> dn_strength[2], dn_threshold[2]; rvc_denoiser *dn[2] = {nullptr, nullptr}; float *d_dn[2] = {nullptr, nullptr};
    // rvc_debug_session_denoise_ms: HIP events around both noise-reduction stages
    bool time_dn = false; hipEvent_t ev_dn[4] = {nullptr, nullptr, nullptr, nullptr}; float dn_ms = 0.f;
    // rvc_debug_session_sola_ms: HIP events around the SOLA stage
    bool time_sola = false; hipEvent_t ev_sola[2] = {nullptr, nullptr}; float sola_ms = 0.f;
};

extern "C" {

void rvc_session_destroy(rvc_session *s)
{
    if (!s) return;
    (void)hipSetDevice(s->e->device);
    (void)hipStreamSynchronize(s->e->stream);
    rvc_resampler_destroy(s->down); rvc_resampler_destroy(s->up);
    for (int side = 0; side < 2; side++) { rvc_denoiser_destroy(s->dn[side]); (void)hipFree(s->d_dn[side]); }
    for (hipEvent_t ev : s->ev_dn) if (ev) (void)hipEventDestroy(ev);
    for (float *p : {s->d_in[0], s->d_in[1], s->d_in16[0], s->d_in16[1], s->d_chunk, s->d_down, s->d_model, s->d_up, s->d_sola, s->d_frame, s->d_cor}) (void)hipFree(p);
    (void)hipFree(s->d_rms);
    (void)hipFree(s->d_off); (void)hipFree(s->d_mixpow);
    for (float *p : {s->d_pva, s->d_pvtab, s->d_pvspec, s->d_gate_thr, s->d_hist[0], s->d_hist[1], s->d_gated}) (void)hipFree(p);
    (void)hipFree(s->d_xfade);
    for (hipEvent_t ev : s->ev_sola) if (ev) (void)hipEventDestroy(ev);
    delete s;
}

// `create` / `update` of the filter (lib.rs:181-260): host sample rate, the three length settings (seconds), the synthesizer's output
// rate; skip_inference != 0 is the plugin's pass-through mode (lib.rs:224-227, 697-699).  The session covers every stream of the
// engine (rvc_set_streams before creating it): all rings, converter states and SOLA tails get a leading [streams] axis.
rvc_status rvc_session_create(rvc_engine *e, size_t sample_rate, double sample_length, double crossfade_length, double extra_inference_time,
                              size_t model_output_sample_rate, int32_t pitch_shift, double rms_mix_rate, int skip_inference, rvc_session **out)
{
    if (out) *out = nullptr;
    return guarded(e, [&]() {
        if (!out || sample_rate < 1000 || sample_rate % 100 != 0 || sample_rate > 384000 || model_output_sample_rate % 100 != 0 || model_output_sample_rate == 0)
            throw ShapeError("session: unsupported sample rate");
        // destroyed through rvc_session_destroy on every failure path (a throwing hipMalloc part-way through included): both converters
        // and every device buffer allocated so far are released
        std::unique_ptr<rvc_session, void (*)(rvc_session *)> sp(new rvc_session(), rvc_session_destroy);
        rvc_session *s = sp.get();
        s->e = e; s->B = e->n_streams; s->h_off.resize(s->B); s->sample_rate = (int)sample_rate; s->pitch_shift.assign(s->B, pitch_shift); s->rms_mix_rate.assign(s->B, rms_mix_rate); s->skip_inference = skip_inference != 0;
        const int zc = s->zc = (int)sample_rate / 100;                                                             // lib.rs:200
        const int sft = (int)llround(sample_length * (double)sample_rate / zc);                                     // lib.rs:202
        s->sample_frame_size = sft * zc; s->sample_frame_16k = sft * 160;                                           // lib.rs:203-205
        s->crossfade_frame_size = (int)llround(crossfade_length * (double)sample_rate / zc) * zc;                   // lib.rs:206-207
        s->sola_buffer_frame_size = std::min(s->crossfade_frame_size, 4 * zc);                                      // lib.rs:208
        s->sola_search_frame_size = zc;                                                                             // lib.rs:209
        s->extra_frame_size = (int)llround(extra_inference_time * (double)sample_rate / zc) * zc;                   // lib.rs:210-211
        s->input_buffer_size = s->extra_frame_size + s->crossfade_frame_size + s->sola_search_frame_size + s->sample_frame_size;   // lib.rs:213-214
        s->input_buffer_16k_size = 160 * s->input_buffer_size / zc;                                                 // lib.rs:217
        s->model_return_length = (s->sample_frame_size + s->sola_buffer_frame_size + s->sola_search_frame_size) / zc;   // lib.rs:220-221
        s->model_rate = s->skip_inference ? 16000 : (int)model_output_sample_rate;                                  // lib.rs:224-226
        s->model_return_size = s->model_return_length * (s->model_rate / 100);                                      // lib.rs:222,226
        s->skip_head = s->extra_frame_size / zc;                                                                    // lib.rs:694
        if (sft < 1 || s->sola_buffer_frame_size < 1 || s->sola_search_frame_size + 1 > 1024) throw ShapeError("session: unsupported length settings");
        // lib.rs:236-242
        rvc_status rc = resampler_create_n(e, sample_rate, 16000, (size_t)s->sample_frame_size + 2 * zc, s->B, &s->down);
        if (rc != RVC_OK) return rc;
        rc = resampler_create_n(e, (size_t)s->model_rate, sample_rate, (size_t)s->model_return_size, s->B, &s->up);
        if (rc != RVC_OK) return rc;
        s->up_out = s->up->fft_out;
        const bool ok = s->down->fft_in == s->sample_frame_size + 2 * zc && s->down->fft_out == s->sample_frame_16k + 320 && s->up->fft_in == s->model_return_size &&
                        s->up_out >= s->sola_buffer_frame_size + s->sola_search_frame_size + s->sample_frame_size;
        if (!ok) {   // rubato would return WrongNumberOfInputFrames on the first chunk and the plugin would panic (lib.rs:680-682)
            throw ShapeError("session: chunk sizes are not multiples of the resampling ratios");
        }
        const size_t NB = (size_t)s->B;
        auto dev = [&](float **p, size_t n) { n = std::max<size_t>(n, 4) * NB; HIPCHK(hipMalloc(p, n * 4)); HIPCHK(hipMemsetAsync(*p, 0, n * 4, e->stream)); };
        for (int i = 0; i < 2; i++) { dev(&s->d_in[i], s->input_buffer_size); dev(&s->d_in16[i], s->input_buffer_16k_size); }
        dev(&s->d_chunk, s->sample_frame_size); dev(&s->d_down, s->down->fft_out); dev(&s->d_model, s->model_return_size); dev(&s->d_up, s->up_out);
        const int frame = 4 * zc, hop = zc;
        s->n_rms = (s->up_out + 2 * (frame / 2) - frame) / hop + 1;
        HIPCHK(hipMalloc(&s->d_rms, (size_t)2 * s->n_rms * NB * 8)); HIPCHK(hipMemsetAsync(s->d_rms, 0, (size_t)2 * s->n_rms * NB * 8, e->stream));
        dev(&s->d_sola, s->sola_buffer_frame_size); dev(&s->d_frame, s->sample_frame_size);
        dev(&s->d_cor, (size_t)s->sola_search_frame_size + 1);
        HIPCHK(hipMalloc(&s->d_off, 4 * NB));
        HIPCHK(hipMalloc(&s->d_mixpow, 4 * NB));
        s->xfade.assign(s->B, RVC_CROSSFADE_LINEAR); s->gate_thr.assign(s->B, -INFINITY);
        for (int side = 0; side < 2; side++) { s->dn_strength[side].assign(s->B, 0.0); s->dn_threshold[side].assign(s->B, 2.0); }
        HIPCHK(hipMalloc(&s->d_xfade, 4 * NB)); HIPCHK(hipMemsetAsync(s->d_xfade, 0, 4 * NB, e->stream));
        if (s->sola_buffer_frame_size >= 2 && s->sola_buffer_frame_size <= PV_MAX_N) {
            std::vector<float> tab; pv_tables(s->sola_buffer_frame_size, tab);
            HIPCHK(hipMalloc(&s->d_pvtab, tab.size() * 4)); HIPCHK(hipMemcpy(s->d_pvtab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
            dev(&s->d_pva, s->sola_buffer_frame_size); dev(&s->d_pvspec, (size_t)3 * (s->sola_buffer_frame_size / 2 + 1));
        }
        dev(&s->d_gate_thr, 1); dev(&s->d_hist[0], (size_t)3 * zc); dev(&s->d_hist[1], (size_t)3 * zc); dev(&s->d_gated, s->sample_frame_size);
        HIPCHK(hipStreamSynchronize(e->stream));
        *out = sp.release();
        return RVC_OK;
    });
}

size_t rvc_session_frame_size(rvc_session *s) { return s ? (size_t)s->sample_frame_size : 0; }
void rvc_session_set_params(rvc_session *s, int32_t pitch_shift, double rms_mix_rate)
{
    if (!s) return;
    s->pitch_shift.assign(s->B, pitch_shift); s->rms_mix_rate.assign(s->B, rms_mix_rate); s->mix_dirty = true;
}
// one stream's settings (the other streams keep theirs)
rvc_status rvc_session_set_params_stream(rvc_session *s, int stream, int32_t pitch_shift, double rms_mix_rate)
{
    if (!s) return RVC_BACKEND;
    if (stream < 0 || stream >= s->B) { s->e->err = "session: stream out of range"; return RVC_SHAPE; }
    s->pitch_shift[stream] = pitch_shift; s->rms_mix_rate[stream] = rms_mix_rate; s->mix_dirty = true;
    return RVC_OK;
}

// crossfade of the SOLA seam, every stream or one: RVC_CROSSFADE_LINEAR (the plugin's sin^2 blend) or RVC_CROSSFADE_PHASE_VOCODER
static rvc_status session_set_crossfade(rvc_session *s, int first, int last, int mode)
{
    if (!s) return RVC_BACKEND;
    if (first < 0 || last > s->B || first >= last) { s->e->err = "session: stream out of range"; return RVC_SHAPE; }
    if (mode != RVC_CROSSFADE_LINEAR && mode != RVC_CROSSFADE_PHASE_VOCODER) { s->e->err = "session: unknown crossfade mode"; return RVC_SHAPE; }
    if (mode == RVC_CROSSFADE_PHASE_VOCODER && s->sola_buffer_frame_size > PV_MAX_N) { s->e->err = "session: the phase-vocoder crossfade takes a seam of at most 4096 samples"; return RVC_SHAPE; }
    for (int b = first; b < last; b++) s->xfade[b] = mode;
    s->n_pv = 0;
    // (a seam of one sample has nothing to analyse: the linear blend serves it)
    for (int b = 0; b < s->B; b++) s->n_pv += s->xfade[b] == RVC_CROSSFADE_PHASE_VOCODER && s->sola_buffer_frame_size >= 2;
    s->xfade_dirty = true;
    return RVC_OK;
}
rvc_status rvc_session_set_crossfade(rvc_session *s, int mode) { return session_set_crossfade(s, 0, s ? s->B : 0, mode); }
rvc_status rvc_session_set_crossfade_stream(rvc_session *s, int stream, int mode) { return session_set_crossfade(s, stream, stream + 1, mode); }
// input gate, every stream or one: 10 ms blocks whose 40 ms RMS is below threshold_db are zeroed in front of the host-rate ring; <= -60 = off
static rvc_status session_set_gate(rvc_session *s, int first, int last, double threshold_db)
{
    if (!s) return RVC_BACKEND;
    if (first < 0 || last > s->B || first >= last) { s->e->err = "session: stream out of range"; return RVC_SHAPE; }
    if (threshold_db != threshold_db) { s->e->err = "session: the gate threshold is not a number"; return RVC_SHAPE; }
    for (int b = first; b < last; b++) s->gate_thr[b] = gate_threshold(threshold_db);
    if (threshold_db > -60.0) s->gate_used = true;
    s->gate_dirty = true;
    return RVC_OK;
}
rvc_status rvc_session_set_input_gate(rvc_session *s, double threshold_db) { return session_set_gate(s, 0, s ? s->B : 0, threshold_db); }
rvc_status rvc_session_set_input_gate_stream(rvc_session *s, int stream, double threshold_db) { return session_set_gate(s, stream, stream + 1, threshold_db); }
// noise reduction of one side, every stream or one.  The side's denoiser and its output buffer are created the first time a stream asks for strength > 0
// (a stream at strength 0 passes bit for bit, undelayed); from the chunk after that call the stream's signal on that side is delayed by zc samples (10 ms)
static rvc_status session_set_noise_reduction(rvc_session *s, int first, int last, int side, double strength, double threshold)
{
    if (!s) return RVC_BACKEND;
    return guarded(s->e, [&]() {
        if (first < 0 || last > s->B || first >= last) throw ShapeError("session: stream out of range");
        if (side != RVC_DENOISE_INPUT && side != RVC_DENOISE_OUTPUT) throw ShapeError("session: unknown noise-reduction side");
        denoiser_check(strength, threshold);
        if (strength > 0.0 && !s->dn[side]) {
            if (2 * s->zc > DN_MAX_N) throw ShapeError("session: noise reduction takes sample rates up to 192000");
            if (!s->d_dn[side]) {
                const size_t bytes = (size_t)s->B * std::max(s->sample_frame_size, 4) * 4;
                HIPCHK(hipMalloc(&s->d_dn[side], bytes)); HIPCHK(hipMemsetAsync(s->d_dn[side], 0, bytes, s->e->stream));
            }
            rvc_status rc = denoiser_create_n(s->e, (size_t)s->sample_rate, s->B, s->sample_frame_size / s->zc, &s->dn[side]);
            if (rc != RVC_OK) return rc;
            for (int b = 0; b < s->B; b++) denoiser_set_range(s->dn[side], b, b + 1, s->dn_strength[side][b], s->dn_threshold[side][b]);
        }
        for (int b = first; b < last; b++) { s->dn_strength[side][b] = strength; s->dn_threshold[side][b] = threshold; }
        if (s->dn[side]) denoiser_set_range(s->dn[side], first, last, strength, threshold);
        return RVC_OK;
    });
}
rvc_status rvc_session_set_noise_reduction(rvc_session *s, int side, double strength, double threshold)
{
    return session_set_noise_reduction(s, 0, s ? s->B : 0, side, strength, threshold);
}
rvc_status rvc_session_set_noise_reduction_stream(rvc_session *s, int stream, int side, double strength, double threshold)
{
    return session_set_noise_reduction(s, stream, stream + 1, side, strength, threshold);
}
// test / measurement hook (include/rvc_mi355x_debug.h): enable != 0 records HIP events around both noise-reduction stages of every later chunk; -> ms of the
// last chunk (the two sides added; 0 while neither side is in use)
float rvc_debug_session_denoise_ms(rvc_session *s, int enable)
{
    if (!s) return -1.f;
    s->time_dn = enable != 0;
    return s->dn_ms;
}
// test / measurement hook (include/rvc_mi355x_debug.h): enable != 0 records HIP events around the SOLA stage of every later chunk; -> ms of the last chunk
float rvc_debug_session_sola_ms(rvc_session *s, int enable)
{
    if (!s) return -1.f;
    s->time_sola = enable != 0;
    return s->sola_ms;
}

// geometry as the plugin derives it (tests): 0 sample_frame_size, 1 sample_frame_16k, 2 input_buffer_size, 3 input_buffer_16k_size,
// 4 model_return_length, 5 model_return_size, 6 skip_head, 7 sola_buffer_frame_size, 8 sola_search_frame_size, 9 extra_frame_size
void rvc_session_geometry(rvc_session *s, int32_t out[10])
{
    if (!s) return;
    const int v[10] = {s->sample_frame_size, s->sample_frame_16k, s->input_buffer_size, s->input_buffer_16k_size, s->model_return_length,
                       s->model_return_size, s->skip_head, s->sola_buffer_frame_size, s->sola_search_frame_size, s->extra_frame_size};
    for (int i = 0; i < 10; i++) out[i] = v[i];
}

// process_one_frame (lib.rs:659-795) for every stream of the engine: input_sample [B][n] with n = sample_frame_size samples at the host
// rate, output [B][cap_per_stream] (sample_frame_size samples each), sola_offset [B] (may be NULL).  B = 1 is the plugin's case.
rvc_status rvc_session_process(rvc_session *s, const float *input_sample, size_t n, float *output, size_t cap, size_t *sola_offset)
{
    if (!s) return RVC_BACKEND;
    rvc_engine *e = s->e;
    return guarded(e, [&]() {
        if (n != (size_t)s->sample_frame_size || cap < (size_t)s->sample_frame_size || !input_sample || !output) throw ShapeError("session: wrong chunk size");
        if (e->n_streams != s->B) throw ShapeError("session: the engine's stream count changed since the session was created");
        hipStream_t st = e->stream;
        const int B = s->B;
        HIPCHK(hipMemcpyAsync(s->d_chunk, input_sample, (size_t)B * n * 4, hipMemcpyHostToDevice, st));
        // settings that changed since the last chunk (as d_mixpow below: a blocking copy, paid by the chunk after a setter call only)
        if (s->xfade_dirty) { HIPCHK(hipMemcpy(s->d_xfade, s->xfade.data(), 4 * (size_t)B, hipMemcpyHostToDevice)); s->xfade_dirty = false; }
        if (s->gate_dirty) { HIPCHK(hipMemcpy(s->d_gate_thr, s->gate_thr.data(), 4 * (size_t)B, hipMemcpyHostToDevice)); s->gate_dirty = false; }
        const float *chunk = s->d_chunk;
        if (s->gate_used) {
            hipLaunchKernelGGL(input_gate_kernel, dim3(s->sample_frame_size / s->zc + 1, B), dim3(256), 0, st, s->d_chunk, s->d_gated, s->d_hist[s->par_h], s->d_hist[s->par_h ^ 1],
                               s->d_gate_thr, 0.f, s->zc, s->sample_frame_size, (long long)s->sample_frame_size, 3LL * s->zc);
            s->par_h ^= 1;
            chunk = s->d_gated;
        }
        // a side whose streams are all back at strength 0 is skipped like one that was never switched on
        const bool dn_on[2] = {s->dn[0] && s->dn[0]->n_on > 0, s->dn[1] && s->dn[1]->n_on > 0};
        const bool time_dn = s->time_dn && (dn_on[0] || dn_on[1]);
        if (time_dn) for (hipEvent_t &ev : s->ev_dn) if (!ev) HIPCHK(hipEventCreate(&ev));
        if (dn_on[RVC_DENOISE_INPUT]) {
            if (time_dn) HIPCHK(hipEventRecord(s->ev_dn[0], st));
            denoiser_launch(s->dn[0], chunk, s->d_dn[0], s->sample_frame_size, (long long)s->sample_frame_size, (long long)s->sample_frame_size);
            if (time_dn) HIPCHK(hipEventRecord(s->ev_dn[1], st));
            chunk = s->d_dn[0];
        }
        // lib.rs:661-665
        launch_ring_shift_append(st, B, s->d_in[s->par], s->d_in[s->par ^ 1], s->input_buffer_size, s->sample_frame_size, chunk);
        s->par ^= 1;
        const float *ring = s->d_in[s->par];
        // lib.rs:669-683: the converter sees the new chunk plus the 2*zc samples before it; its first 160 outputs are dropped
        const int down_start = s->input_buffer_size - s->sample_frame_size - 2 * s->sample_rate / 100;
        resampler_launch(s->down, ring + down_start, s->d_down, s->input_buffer_size, s->down->fft_out);
        const int copy_begin = s->input_buffer_16k_size - (s->sample_frame_size / (s->sample_rate / 100) + 1) * 160;
        launch_ring16_update(st, B, s->d_in16[s->par16], s->d_in16[s->par16 ^ 1], s->input_buffer_16k_size, s->sample_frame_16k, s->d_down, 160, copy_begin, (long long)s->down->fft_out);
        s->par16 ^= 1;
        const float *ring16 = s->d_in16[s->par16];
        // lib.rs:694-707
        if (s->skip_inference) {
            HIPCHK(hipMemcpy2DAsync(s->d_model, (size_t)s->model_return_size * 4, ring16 + (s->input_buffer_16k_size - s->model_return_size),
                                    (size_t)s->input_buffer_16k_size * 4, (size_t)s->model_return_size * 4, B, hipMemcpyDeviceToDevice, st));
        } else {
            size_t got = 0;
            // with retrieval on, the chunk is synchronised before the post-processing chain: a hand-off time-out of the one-launch retrieval is
            // recovered inside infer_common (the SOLA / envelope state behind it must only ever see the recovered chunk)
            // (only plans that CAN be recovered pay for that -- the one-launch retrieval of up to 11 streams, whose plan carries the fallback launches;
            //  many-stream plans search through the distance GEMM and hand nothing over inside a launch: their chain stays asynchronous)
            bool sync_infer = false;
            if (e->index.rows && e->index_rate > 0.f) {
                // (the plan infer_common will run: its formant key; streams in several formant buckets run synchronously anyway)
                uint32_t r2 = 0; bool fstage = false;
                if (formant_key(e, (uint32_t)s->model_return_length, nullptr, &r2, &fstage)) {
                    Plan *peek = get_plan(e, plan_key(e, 0, (size_t)s->input_buffer_16k_size, (size_t)s->sample_frame_16k, (uint32_t)s->skip_head, (uint32_t)s->model_return_length));
                    sync_infer = !peek->knn_fallback.empty();
                } else sync_infer = true;
            }
            rvc_status rc = infer_common(e, ring16, true, (size_t)s->input_buffer_16k_size, (size_t)s->sample_frame_16k, 0, (uint32_t)s->skip_head,
                                         (uint32_t)s->model_return_length, s->d_model, true, (size_t)s->model_return_size, &got, sync_infer, s->pitch_shift.data());
            if (rc != RVC_OK) return rc;
            if (got != (size_t)s->model_return_size) throw ShapeError("session: the loaded synthesizer's output rate does not match model_output_sample_rate");
        }
        // lib.rs:742-756
        resampler_launch(s->up, s->d_model, s->d_up, s->model_return_size, s->up_out);
        // lib.rs:758-765
        const long long up_bs = s->up_out;
        bool any_mix = false;
        for (int b = 0; b < B; b++) any_mix = any_mix || s->rms_mix_rate[b] < 1.0;
        if (any_mix) {
            if (s->mix_dirty) {      // exponent 1 - rate per stream; a stream at rate >= 1 gets 0: powf(x, 0) = 1 leaves it untouched (lib.rs:758)
                std::vector<float> mp(B);
                for (int b = 0; b < B; b++) mp[b] = s->rms_mix_rate[b] < 1.0 ? (float)(1.0 - s->rms_mix_rate[b]) : 0.f;
                HIPCHK(hipMemcpy(s->d_mixpow, mp.data(), 4 * (size_t)B, hipMemcpyHostToDevice));
                s->mix_dirty = false;
            }
            const int nn = s->up_out, frame = 4 * s->zc, hop = s->zc, nf = s->n_rms;
            launch_post_rms(st, B, ring + s->extra_frame_size, nn, frame, hop, nf, s->d_rms, (long long)s->input_buffer_size, 2LL * nf);
            launch_post_rms(st, B, s->d_up, nn, frame, hop, nf, s->d_rms + nf, up_bs, 2LL * nf);
            launch_post_mix(st, B, s->d_up, nn, s->d_rms, nf, s->d_rms + nf, nf, 0.f, up_bs, 2LL * nf, s->d_mixpow);
        }
        // lib.rs:768-794
        const long long cor_bs = s->sola_search_frame_size + 1;
        if (s->time_sola) {
            for (hipEvent_t &ev : s->ev_sola) if (!ev) HIPCHK(hipEventCreate(&ev));
            HIPCHK(hipEventRecord(s->ev_sola[0], st));
        }
        launch_post_sola_corr(st, B, s->d_up, s->d_sola, s->sola_buffer_frame_size, s->sola_search_frame_size, s->d_cor, up_bs, (long long)s->sola_buffer_frame_size, cor_bs);
        launch_post_sola(st, B, s->d_up, s->d_sola, s->sola_buffer_frame_size, s->sola_search_frame_size, s->sample_frame_size, s->d_frame, s->d_off, s->d_cor, up_bs,
                         (long long)s->sola_buffer_frame_size, (long long)s->sample_frame_size, cor_bs, s->n_pv ? s->d_xfade : (const int *)nullptr, 0, s->d_pva,
                         (long long)s->sola_buffer_frame_size);
        if (s->n_pv) {      // phase-vocoder streams: the blend over output / frame / tail, from the offset the kernel above left on the device
            const int pn = s->sola_buffer_frame_size, K = pn / 2 + 1;
            hipLaunchKernelGGL(pv_analysis_kernel, dim3((K + PV_AT - 1) / PV_AT, B), dim3(PV_AT), pv_analysis_lds(pn), st, s->d_up, s->d_pva, s->d_off, s->d_xfade, 0,
                               s->d_pvtab, pn, s->d_pvspec, up_bs, (long long)pn);
            hipLaunchKernelGGL(pv_synth_kernel, dim3((pn + PV_JT - 1) / PV_JT, B), dim3(PV_JT * PV_KS), pv_synth_lds(pn), st, s->d_up, s->d_pva, s->d_sola, s->d_frame, s->d_off,
                               s->d_xfade, 0, s->d_pvtab, s->d_pvspec, pn, s->sample_frame_size, up_bs, (long long)pn, (long long)pn, (long long)s->sample_frame_size);
        }
        if (s->time_sola) HIPCHK(hipEventRecord(s->ev_sola[1], st));
        const float *frame = s->d_frame;
        if (dn_on[RVC_DENOISE_OUTPUT]) {
            if (time_dn) HIPCHK(hipEventRecord(s->ev_dn[2], st));
            denoiser_launch(s->dn[1], s->d_frame, s->d_dn[1], s->sample_frame_size, (long long)s->sample_frame_size, (long long)s->sample_frame_size);
            if (time_dn) HIPCHK(hipEventRecord(s->ev_dn[3], st));
            frame = s->d_dn[1];
        }
        HIPCHK(hipMemcpy2DAsync(output, cap * 4, frame, (size_t)s->sample_frame_size * 4, (size_t)s->sample_frame_size * 4, B, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(s->h_off.data(), s->d_off, 4 * (size_t)B, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        if (s->time_sola) HIPCHK(hipEventElapsedTime(&s->sola_ms, s->ev_sola[0], s->ev_sola[1]));
        if (time_dn) {
            s->dn_ms = 0.f;
            for (int side = 0; side < 2; side++) if (dn_on[side]) { float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, s->ev_dn[2 * side], s->ev_dn[2 * side + 1])); s->dn_ms += ms; }
        }
        if (sola_offset) for (int b = 0; b < B; b++) sola_offset[b] = (size_t)s->h_off[b];
        return s->skip_inference ? RVC_OK : final_status(e);
    });
}

}  // extern "C"
