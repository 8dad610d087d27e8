// engine.hip -- the engine object and the C ABI of the MI355X-native RVC streaming inference engine.
//
// Mirrors rvc::RvcInfer (reference: rvc/src/rvc.rs:18-220): model handles, the 1024-entry
// pitch cache, and the per-chunk pipeline hubert -> (retrieval) -> pitch -> synthesizer.
// All compute is launched as hand-written gfx950 kernels (the *.hip.h headers); nothing here falls
// back to a CPU path: without a HIP device every entry point returns RVC_BACKEND.
#include "engine_int.h"
#include "chunk.hip.h"
#include "crossfade.hip.h"
#include "f0_override.hip.h"
#include <chrono>

// The HIP runtime multiplexes all streams of a process onto GPU_MAX_HW_QUEUES hardware queues (default 4).  The engine runs four
// streams concurrently per chunk; a second engine in the process, or the streams an RCCL communicator leaves behind, then share
// queues with them and the per-chunk latency rises by 5-20 % (measured: 2.38 -> 2.84 ms for an engine created after a communicator;
// flat 2.38 ms with 16 queues).  The variable is read when the runtime initialises, so a default is planted when this library is
// loaded -- it does not override a value the host has set, and a host that has already initialised HIP should set it itself
// (the variable then has no effect: rvc_create says so once on stderr).  A host that wants its environment left alone sets
// RVC_NO_RUNTIME_DEFAULTS=1 (documented in include/rvc_mi355x.h and INTEGRATION.md).
static bool g_planted_queues = false;
__attribute__((constructor)) static void rvc_runtime_defaults()
{
    if (getenv("RVC_NO_RUNTIME_DEFAULTS")) return;
    if (!getenv("GPU_MAX_HW_QUEUES")) { setenv("GPU_MAX_HW_QUEUES", "16", 0); g_planted_queues = true; }
}

namespace rvc {

static void init_kernel_attrs()
{
    // per device: function attributes belong to the device that is current when they are set (an engine on a second GPU of one process needs its own)
    static std::mutex mu; static bool done[64] = {};
    int dev = 0; HIPCHK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if (dev >= 0 && dev < 64) { if (done[dev]) return; done[dev] = true; }
    plan_kernel_attrs(); retrieval_kernel_attrs();
}

void launch_protect_mix(hipStream_t s, int B, const StreamState *st, const float *pitchf, const float *cv, int cv_cs, long long cv_bs, int C, int T, int skip_head, int R,
                        float *phone, int ph_cs, long long ph_bs)
{
    hipLaunchKernelGGL(protect_mix_kernel, protect_grid(R, B, C), dim3(PROTECT_ROWS, PROTECT_LANES), 0, s, st, pitchf, cv, cv_cs, cv_bs, C, T, skip_head, R, phone, ph_cs, ph_bs);
}

// f0 from outside (f0_override.hip.h): the launches, for the engine below and for rvc_debug_f0_override (debug.hip)
void launch_f0_override(hipStream_t s, int B, int Tm, const float *f, float *out, const F0OvCall *call, const int *cnt, const float *rows, const int *map)
{
    hipLaunchKernelGGL(f0_override_kernel, dim3((Tm + 255) / 256, B), dim3(256), 0, s, f, out, Tm, call, cnt, rows, map);
}
void launch_f0_curve_grid(hipStream_t s, const double *t, const float *hz, int n, float *grid, long long Nf)
{
    hipLaunchKernelGGL(f0_curve_grid_kernel, dim3((unsigned)((Nf + 255) / 256)), dim3(256), 0, s, t, hz, n, grid, Nf);
}
// (launch_f0_export, the third: windows.hip.h, beside the export kernel of the windowed calls)

// the caller-side post-processing launches (chunk.hip.h), B streams each: rvc_envelop_mixing, sola_step_host and rvc_session_process queue them through
// these, and so does rvc_debug_post (debug.hip)
void launch_post_rms(hipStream_t s, int B, const float *y, int n, int frame, int hop, int nf, double *out, long long y_bs, long long out_bs)
{
    hipLaunchKernelGGL(post_rms_kernel, dim3(nf, B), dim3(256), 0, s, y, n, frame, hop, out, y_bs, out_bs);
}
void launch_post_mix(hipStream_t s, int B, float *out, int n, const double *r1, int n1, const double *r2, int n2, float mix_power, long long out_bs, long long r_bs, const float *mix_power_v)
{
    hipLaunchKernelGGL(post_mix_kernel, dim3((n + 255) / 256, B), dim3(256), 0, s, out, n, r1, n1, r2, n2, mix_power, out_bs, r_bs, mix_power_v);
}
void launch_post_sola_corr(hipStream_t s, int B, const float *output, const float *sola, int sola_len, int search, float *cor, long long out_bs, long long sola_bs, long long cor_bs)
{
    hipLaunchKernelGGL(post_sola_corr_kernel, dim3((unsigned)(search + 4) / 4, B), dim3(256), 0, s, output, sola, sola_len, search, cor, out_bs, sola_bs, cor_bs);
}
void launch_post_sola(hipStream_t s, int B, float *output, float *sola, int sola_len, int search, int frame, float *frame_out, int *offset_out, const float *cor, long long out_bs,
                      long long sola_bs, long long frame_bs, long long cor_bs, const int *mode_v, int mode_all, float *pv_a, long long pva_bs)
{
    hipLaunchKernelGGL(post_sola_kernel, dim3(B), dim3(1024), 0, s, output, sola, sola_len, search, frame, frame_out, offset_out, cor, out_bs, sola_bs, frame_bs, cor_bs,
                       mode_v, mode_all, pv_a, pva_bs);
}

static void init_constants(rvc_engine *e)
{
    init_kernel_attrs();
    // periodic Hann, f64 cosine cast to f32 then 0.5*(1-c) in f32 (rmvpe.rs:33-37, Q9)
    std::vector<float> win(1024), tw(1024), basis((size_t)128 * 513);
    for (int i = 0; i < 1024; i++) { float c = (float)cos(2.0 * M_PI * (double)i / 1024.0); win[i] = 0.5f * (1.0f - c); }
    for (int j = 0; j < 512; j++) { double a = -2.0 * M_PI * (double)j / 1024.0; tw[2 * j] = (float)cos(a); tw[2 * j + 1] = (float)sin(a); }
    // mel_spec::mel::mel(16000, 1024, 128, 30, 8000, htk=true, norm=true) (rmvpe.rs:146-148,220): HTK mel scale,
    // triangular filters, Slaney area normalisation, computed in f64 then cast to f32
    const int nb = 513, nm = 128;
    const double sr = 16000.0, fmin = 30.0, fmax = 8000.0;
    std::vector<double> melf(nm + 2);
    double mlo = 2595.0 * log10(1.0 + fmin / 700.0), mhi = 2595.0 * log10(1.0 + fmax / 700.0);
    for (int i = 0; i < nm + 2; i++) { double m = mlo + (mhi - mlo) * (double)i / (double)(nm + 1); melf[i] = 700.0 * (pow(10.0, m / 2595.0) - 1.0); }
    for (int i = 0; i < nm; i++) {
        double fd0 = melf[i + 1] - melf[i], fd1 = melf[i + 2] - melf[i + 1], enorm = 2.0 / (melf[i + 2] - melf[i]);
        for (int j = 0; j < nb; j++) {
            double f = (sr / 2.0) * (double)j / (double)(nb - 1);
            double lower = -(melf[i] - f) / fd0, upper = (melf[i + 2] - f) / fd1;
            double v = std::max(0.0, std::min(lower, upper));
            basis[(size_t)i * nb + j] = (float)(v * enorm);
        }
    }
    e->d_window = upload_f(win); e->d_twiddle = upload_f(tw); e->d_basis = upload_f(basis);
    std::vector<int> band(256);
    for (int i = 0; i < nm; i++) {
        int lo = nb, hi = 0;
        for (int j = 0; j < nb; j++) if (basis[(size_t)i * nb + j] != 0.f) { lo = std::min(lo, j); hi = std::max(hi, j + 1); }
        if (hi <= lo) { lo = 0; hi = 0; }
        band[2 * i] = lo; band[2 * i + 1] = hi;
    }
    HIPCHK(hipMalloc(&e->d_band, band.size() * sizeof(int)));
    HIPCHK(hipMemcpy(e->d_band, band.data(), band.size() * sizeof(int), hipMemcpyHostToDevice));
}

static void reset_state(rvc_engine *e)
{
    std::vector<StreamState> st(e->n_streams);
    for (int b = 0; b < e->n_streams; b++) { memset(&st[b], 0, sizeof(StreamState)); st[b].stream_id = e->stream_id0 + (uint32_t)b; }
    HIPCHK(hipMemcpy(e->d_state, st.data(), sizeof(StreamState) * e->n_streams, hipMemcpyHostToDevice));
    e->pushed_valid = false;       // (the per-stream multipliers live in StreamState)
    for (auto &v : e->ov) v.clear();      // pending f0 overrides go with the state; the curve of rvc_set_f0_curve stays
    e->ov_dirty = true;
}

// the device block of the f0 overrides: F0OvCall (64 bytes) | one count per stream | rows [streams][F0_OV_ROWS].  `streams` is e->ov.size(): the engine's own
// stream count, also while a bucket plan is being built on fewer
static_assert(sizeof(F0OvCall) <= 64, "the override block keeps 64 bytes for the call");
static inline size_t ov_rows_off(size_t S) { return 64 + (S * sizeof(int) + 63) / 64 * 64; }
static void ensure_ov(rvc_engine *e)
{
    if (e->d_ov) return;
    const size_t S = e->ov.size(), bytes = ov_rows_off(S) + S * F0_OV_ROWS * sizeof(float);
    HIPCHK(hipMalloc(&e->d_ov, bytes));
    HIPCHK(hipMemset(e->d_ov, 0, bytes));
    e->ov_dirty = true;
}

// CU partition for the two concurrent branches of a chunk at low stream counts: the f0 branch (RMVPE: ~140 short weight-streaming
// kernels) gets 1/8 of the CUs (one XCD), ContentVec the rest.  Sharing CUs slows the f0 branch by ~35 % (measured).  With
// many streams every kernel fills the chip and the streams are plain.
//
// CU-masked streams are never destroyed: the runtime recycles the hardware queue of a destroyed stream, mask included, for the next
// stream it creates -- an engine created after another one had been destroyed then ran its MAIN stream on a partition (measured:
// 2.41 -> 2.79-3.1 ms per chunk for the second engine of a process; no effect without masks).  Masked pairs live in a per-device
// pool for the life of the process; engines borrow a pair and hand it back.
// Round 3: the same holds, less visibly, for plain streams: every stream an engine creates takes the next hardware queue, and after a
// few create / destroy cycles in one process (the bench's sub-configurations, a host that reloads engines) a new engine's main stream
// can share a queue with its own masked f0 stream -- the two then serialise (measured in one bench process: v1 2.15 -> 2.71 ms, two
// streams 3.35 -> 4.79 ms per chunk for engines created after several others had come and gone).  So ALL streams of an engine come
// from a per-device pool of complete sets (main + three plain auxiliaries + the masked pair), created together -- six consecutive
// hardware queues -- and never destroyed; an engine borrows a set and hands it back.
struct StreamSet { int device; hipStream_t main, plain[3], f0, cv; bool masked_ok, in_use; int nf0; };      // nf0: CUs of the masked f0 stream (sets differ only in this)
static std::mutex g_pool_mu;
static std::vector<StreamSet *> g_pool;

static StreamSet *acquire_stream_set(int device, int ncu, int nf0, bool want_masks)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (StreamSet *m : g_pool)
        if (m->device == device && !m->in_use && m->nf0 == nf0) { m->in_use = true; return m; }
    StreamSet *m = new StreamSet{device, nullptr, {nullptr, nullptr, nullptr}, nullptr, nullptr, false, true, nf0};
    // creation order = the order a lone engine always used: main, the masked pair, the side stream (the first bench run of this
    // pool created all plain streams first: 2.17 -> 2.80 ms per chunk -- queue assignment follows creation order); the two plain
    // streams that stand in for the masked pair at more than 4 streams are created when such an engine first borrows the set
    // tuning aid: RVC_STREAM_ORDER = a permutation of "mfcs" (main, f0 masked, ContentVec masked, side), RVC_STREAM_PAD = dummy streams first
    const char *ord = tune_env("RVC_STREAM_ORDER"); if (!ord || strlen(ord) != 4) ord = "mfcs";
    if (const char *pd = tune_env("RVC_STREAM_PAD")) for (int i = 0; i < atoi(pd); i++) { hipStream_t d; HIPCHK(hipStreamCreateWithFlags(&d, hipStreamNonBlocking)); }
    m->masked_ok = want_masks;
    for (int k = 0; k < 4; k++) {
        const char w = ord[k];
        if (w == 'm') HIPCHK(hipStreamCreateWithFlags(&m->main, hipStreamNonBlocking));
        else if (w == 's') HIPCHK(hipStreamCreateWithFlags(&m->plain[1], hipStreamNonBlocking));
        else if (want_masks && m->masked_ok) {
            const int i = w == 'f' ? 0 : 1;
            std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
            for (int c = 0; c < ncu; c++) if ((c < nf0) == (i == 0)) mask[c / 32] |= 1u << (c % 32);
            hipStream_t *dst = i == 0 ? &m->f0 : &m->cv;
            if (hipExtStreamCreateWithCUMask(dst, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
                (void)hipGetLastError();
                m->masked_ok = false;        // (a first stream that did get created stays allocated: it must not be destroyed either)
            }
        }
    }
    g_pool.push_back(m);
    return m;
}
static void release_stream_set(StreamSet *m)
{
    if (!m) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    m->in_use = false;
}

static void configure_aux_streams(rvc_engine *e)
{
    hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, e->device));
    // The f0 branch gets ONE whole XCD (an eighth of the CUs), ContentVec the other seven.  Round 5 tried two XCDs after ContentVec's GEMMs had become
    // faster.  The tuning build (per-wave probe stamps compiled in) said 2.253 -> 2.167 ms at one stream and 4.99 -> 4.61 at four; the PRODUCT build on
    // the same pool says the opposite: 2.044-2.048 -> 2.06-2.08 at one stream, 2.87 -> 3.03 at two, 4.21 -> 4.46 at four (only the v1 model, whose
    // ContentVec stops at layer 9, gains: 2.075 -> 1.994).  Partitions that cut an XCD in two lose badly either way (56: 2.244, 72: 2.469, 80: 2.484).
    // Lesson kept here: partition sizes are tuned on the product build only.
    // The one exception is measured on the product build too (tests/tools/f0_xcds.py, same box, two alternating runs): the v1 model (ContentVec stops at
    // layer 9: the chunk waits for the f0 branch) with two XCDs for f0 runs 1.98-2.02 -> 1.92-1.93 ms at one stream, 2.72-2.77 -> 2.68 at two,
    // 3.45 -> 3.43 at three (and 3.87 -> 3.95 at four: one XCD there; v2 loses at every count: 1.98-2.02 -> 2.04-2.06, 2.77 -> 2.96, 3.65 -> 3.79, 4.09 -> 4.36).
    // Sets with that partition are separate members of the pool (masks are fixed at creation).
    int ncu = prop.multiProcessorCount;
    int xcds = e->cv && e->cv->run_layers <= 9 && e->n_streams <= 3 ? 2 : 1;
    if (const char *f = test_opt("RVC_F0_XCDS")) { const int v = atoi(f); if (v >= 1 && v <= 4) xcds = v; }     // test hook: both partitions are covered by the parity tests
    int nf0 = xcds * (ncu / 8);
    g_ncu = ncu > 0 ? ncu : 256;
    if (const char *f = tune_env("RVC_F0_CUS")) { const int v = atoi(f); if (v >= 8 && v < ncu) nf0 = v; }   // tuning aid
    if (e->sset && e->sset->nf0 != nf0 && e->sset->masked_ok) {      // (callers have synchronised the device and dropped the plans)
        release_stream_set(e->sset); e->sset = nullptr;
    }
    if (!e->sset) {
        e->sset = acquire_stream_set(e->device, ncu, nf0, e->partition_ok && ncu >= 64 && ncu <= 1024);
        e->stream = e->sset->main;
        if (!e->sset->masked_ok) e->partition_ok = false;
    }
    const bool want = e->partition_ok && e->sset->masked_ok && e->n_streams <= 4;
    e->partitioned = want;
    e->cv_cus = want ? g_ncu - nf0 : g_ncu;
    // Without the partition (more than 4 streams) ContentVec runs on the main stream and the f0 branch on the SIDE stream: the side work (NSF source,
    // noise convolutions) is forked behind the join of the f0 branch, so the two never need the stream at the same time, and an engine needs no
    // stream beyond the set's four.  (Round 3 created two more plain streams for such engines.  A one-stream engine that runs late in a long
    // process -- the bench's last leg -- sometimes has its f0 branch at 1 150 us instead of 1 085 (chunk 2.06 -> 2.15-2.25 ms); with two streams
    // fewer in the process that happened in 3 of 6 bench runs instead of 4 of 6: not the cause, or not the only one.  DESIGN.md section 7.)
    e->aux[0] = want ? e->sset->f0 : e->sset->plain[1];
    e->aux[1] = e->sset->plain[1];
    e->aux[2] = want ? e->sset->cv : e->sset->plain[1];
}

void drop_plans(rvc_engine *e)
{
    HIPCHK(hipDeviceSynchronize());      // unsynchronised calls may still be running on the plans freed here
    e->plans.clear(); e->last_plan = nullptr;
}
// the `keep` most recently used plans stay (each owns its activation arena and graph)
static void evict_lru(rvc_engine *e, size_t keep)
{
    while (e->plans.size() > keep) { if (e->last_plan == e->plans.front().get()) e->last_plan = nullptr; e->plans.erase(e->plans.begin()); }
}

static void alloc_state(rvc_engine *e)
{
    drop_plans(e);                       // (their kernels bake the address of the state block)
    if (e->d_state) (void)hipFree(e->d_state);
    if (e->d_state_bucket) { (void)hipFree(e->d_state_bucket); e->d_state_bucket = nullptr; }
    if (e->d_bucket_idx) { (void)hipFree(e->d_bucket_idx); e->d_bucket_idx = nullptr; }
    if (e->d_ov) { (void)hipFree(e->d_ov); e->d_ov = nullptr; }
    e->ov.assign((size_t)e->n_streams, std::vector<float>());
    HIPCHK(hipMalloc(&e->d_state, sizeof(StreamState) * e->n_streams));
    e->settings.resize(e->n_streams, e->settings_default);   // existing streams keep their settings, new ones get the default
    reset_state(e);
}

// ------------------------------- plan -------------------------------------------------
static inline bool is_crepe(int method) { return method == RVC_F0_CREPE || method == RVC_F0_CREPE_TINY; }
// the f0 branch of the engine's method: RMVPE's network and salience decode, the YIN launch, PM's three launches, CREPE's or FCPE's network and decoder, or -- a hybrid -- several of
// them and the launch that combines their rows; behind each the same pitch tail (shift, cache, get_f0_post)
// f0 from outside: between the method's row buffer and the pitch tail, one launch that selects every row against the override the call
// brings for it.  The launch reads the engine's override block (push_overrides fills it in front of the chunk), a bucket plan through the bucket's stream numbers
static const float *add_f0_override(rvc_engine *e, Plan &pl, int B, const float *f0)
{
    ensure_ov(e);
    const int Tm = pl.Tm;
    if (Tm < 1 || Tm > F0_OV_ROWS) throw ShapeError("f0 override: the f0 window has more than 1024 rows");
    float *out = pl.arena.floats((size_t)B * Tm);
    const F0OvCall *call = (const F0OvCall *)e->d_ov; const int *cnt = (const int *)(e->d_ov + 64); const float *rows = (const float *)(e->d_ov + ov_rows_off(e->ov.size()));
    const int *map = pl.key.bucket ? e->d_bucket_idx : nullptr;
    pl.ops.push_back([=](hipStream_t s) { launch_f0_override(s, B, Tm, f0, out, call, cnt, rows, map); });
    add_stamp(pl, "f0.override");
    { T1 t; t.p = out; t.B = B; t.C = 1; t.T = Tm; t.ld = Tm; t.bs = Tm; add_tap(pl, "ov.f0", t); }
    return out;
}

static void build_f0(rvc_engine *e, Plan &pl, int B, size_t L, size_t frame16k, bool update_cache, size_t hubert_length, float **pitchf_out, int **pitch_out)
{
    if (pl.key.f0_override) {
        // the method's rows as a plain buffer -- RMVPE through the stand-alone decode of a hybrid of one, which is RMVPE bit for bit (section 25) --, the select, the tail
        const float *f0 = nullptr;
        if (e->f0_method == RVC_F0_YIN) f0 = build_yin(e, pl, B, L, frame16k);
        else if (e->f0_method == RVC_F0_PM) f0 = build_pm(e, pl, B, L, frame16k);
        else if (is_crepe(e->f0_method)) f0 = build_crepe(e, pl, B, L, frame16k, e->f0_method);
        else if (e->f0_method == RVC_F0_FCPE) f0 = build_fcpe(e, pl, B, L, frame16k);
        else if (e->f0_method == RVC_F0_RMVPE) {
            if (!e->rm) throw std::logic_error("f0 method");
            const T1 sal = build_rmvpe(e, pl, B, L, frame16k, update_cache);
            const float *rows[HYBRID_MEMBERS_MAX] = {};
            f0 = add_f0_hybrid(e, pl, B, 1, RVC_HYBRID_VOTE, rows, 0, sal);
        }
        if (f0) {
            build_pitch_post(e, pl, B, T1{}, update_cache, frame16k, hubert_length, pitchf_out, pitch_out, add_f0_override(e, pl, B, f0));
            return;
        }
    }
    if (e->f0_method == RVC_F0_YIN) {
        const float *f0 = build_yin(e, pl, B, L, frame16k);
        build_pitch_post(e, pl, B, T1{}, update_cache, frame16k, hubert_length, pitchf_out, pitch_out, f0);
        return;
    }
    if (e->f0_method == RVC_F0_PM) {
        const float *f0 = build_pm(e, pl, B, L, frame16k);
        build_pitch_post(e, pl, B, T1{}, update_cache, frame16k, hubert_length, pitchf_out, pitch_out, f0);
        return;
    }
    if (e->f0_method == RVC_F0_HYBRID) {
        // hybrid: the members' own builders one after another on this branch's stream -- no further stream, fork or join --, then one
        // launch that decodes RMVPE's salience (if a member) and combines the rows, and the pitch tail on the combined row as on any f0_in
        int mem[HYBRID_MEMBERS_MAX]; const int n = hybrid_unpack(pl.key.hybrid, mem);
        if (n < 1) throw std::logic_error("f0 method");
        const float *rows[HYBRID_MEMBERS_MAX] = {}; int rm_at = -1; T1 sal;
        bool both_crepe = false;
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) both_crepe = both_crepe || (mem[i] == RVC_F0_CREPE && mem[j] == RVC_F0_CREPE_TINY);
        for (int i = 0; i < n; i++) {
            if (mem[i] == RVC_F0_RMVPE) {
                if (!e->rm) throw std::logic_error("f0 method");
                sal = build_rmvpe(e, pl, B, L, frame16k, update_cache); rm_at = i;
            } else if (mem[i] == RVC_F0_YIN) rows[i] = build_yin(e, pl, B, L, frame16k);
            else if (mem[i] == RVC_F0_PM) rows[i] = build_pm(e, pl, B, L, frame16k);
            else if (is_crepe(mem[i])) rows[i] = build_crepe(e, pl, B, L, frame16k, mem[i], both_crepe && mem[i] == RVC_F0_CREPE_TINY ? "crt" : "cr");
            else if (mem[i] == RVC_F0_FCPE) rows[i] = build_fcpe(e, pl, B, L, frame16k);
            else throw std::logic_error("f0 method");
        }
        const float *f0 = add_f0_hybrid(e, pl, B, n, pl.key.hybrid_mode, rows, rm_at, sal);
        build_pitch_post(e, pl, B, T1{}, update_cache, frame16k, hubert_length, pitchf_out, pitch_out, pl.key.f0_override ? add_f0_override(e, pl, B, f0) : f0);
        return;
    }
    if (is_crepe(e->f0_method)) {
        const float *f0 = build_crepe(e, pl, B, L, frame16k, e->f0_method);
        build_pitch_post(e, pl, B, T1{}, update_cache, frame16k, hubert_length, pitchf_out, pitch_out, f0);
        return;
    }
    if (e->f0_method == RVC_F0_FCPE) {
        const float *f0 = build_fcpe(e, pl, B, L, frame16k);
        build_pitch_post(e, pl, B, T1{}, update_cache, frame16k, hubert_length, pitchf_out, pitch_out, f0);
        return;
    }
    if (!e->rm) throw std::logic_error("f0 method");
    const T1 sal = build_rmvpe(e, pl, B, L, frame16k, update_cache);
    build_pitch_post(e, pl, B, sal, update_cache, frame16k, hubert_length, pitchf_out, pitch_out);
}

// the cached plan of key k (engine.hip plan_key), built on a miss
static Plan *get_plan(rvc_engine *e, const PlanKey &k)
{
    // A bucket plan serves k.B of the engine's streams, whose states the caller gathers into d_state_bucket.  The builders read the stream count and the state
    // block from the engine: both are swapped for the duration of the build.
    struct Swap {
        rvc_engine *e; int n0; StreamState *s0; bool on;
        Swap(rvc_engine *e_, int B, StreamState *st) : e(e_), n0(e_->n_streams), s0(e_->d_state), on(B > 0) { if (on) { e->n_streams = B; e->d_state = st; } }
        ~Swap() { if (on) { e->n_streams = n0; e->d_state = s0; } }
    } swap_guard(e, k.bucket ? k.B : 0, e->d_state_bucket);
    // plans built before a test hook changed are stale (the hooks are process-global and not part of the key)
    const unsigned gen = g_opt_gen.load();
    for (size_t i = 0; i < e->plans.size();)
        if (e->plans[i]->opt_gen != gen) {
            HIPCHK(hipDeviceSynchronize());
            if (e->last_plan == e->plans[i].get()) e->last_plan = nullptr;
            e->plans.erase(e->plans.begin() + i);
        } else i++;
    for (auto &p : e->plans)
        if (p->key == k) {
            // least recently used first: a hit moves to the back, so eviction (front) never takes a plan the current call has just fetched
            Plan *hit = p.get();
            std::rotate(&p, &p + 1, e->plans.data() + e->plans.size());
            return hit;
        }
    e->plan_builds++;
    const auto build_t0 = std::chrono::steady_clock::now();
    std::unique_ptr<Plan> up(new Plan());
    Plan &pl = *up;
    pl.key = k; pl.opt_gen = gen;
    const int mode = k.mode, B = k.B; const size_t L = k.L, frame16k = k.frame16k; const uint32_t skip_head = k.skip_head, R = k.R;
    const bool with_index = k.with_index, with_protect = k.with_protect;
    const bool nof0 = mode == 0 && e->sy && !e->sy->has_f0;      // a model without pitch guidance: no pitch branch, no source, no protect launch (plan_key)
    pl.autotune = e->autotune != 0 && B > 4;          // (queue_igemm: trials on this device while the plan is built; plans of <= 4 streams keep the latency-tuned rules)
    pl.d_in = pl.arena.floats((size_t)B * L + 64);
    T1 src0; float *d_pitchf0 = nullptr; int *d_pitch0 = nullptr;
    size_t rm_begin = 0, rm_end = 0;
    // YIN's f0 branch is two short launches.  Test hook RVC_YIN_CV_ALL_CUS = 1 leaves ContentVec on the main stream with every CU under it (measured against
    // the partition: DESIGN.md section 11); not for pipelined calls, whose front branches are the masked pair
    // Without pitch guidance there is no f0 branch at all: the plan is one chain on the main stream, ContentVec with every CU under it
    const bool part = mode == 0 && !nof0 && e->partitioned && !(e->f0_method == RVC_F0_YIN && !e->pipeline && test_opt_int("RVC_YIN_CV_ALL_CUS", 0) == 1);
    const int f0_sid = 1, cv_sid = part ? 3 : 0;
    if (mode == 0 && !nof0) {
        // f0 branch first (auxiliary stream): independent of ContentVec until the synthesizer
        const int Tcv = e->cv->out_frames(L);
        if (Tcv < 1) throw ShapeError("input too short for ContentVec");
        const size_t hubert_length0 = std::min(L / 160, 2 * (size_t)Tcv + 1);   // rvc.rs:153
        pl.ops.fork(f0_sid);
        rm_begin = pl.ops.v.size();
        pl.ops.cur = f0_sid;
        build_f0(e, pl, B, L, frame16k, true, hubert_length0, &d_pitchf0, &d_pitch0);
        pl.ops.cur = 0;
        rm_end = pl.ops.v.size();
    }
    if (mode == 0 || mode == 1) {
        if (!e->cv) throw std::logic_error("contentvec");
        if (e->cv->out_frames(L) < 1) throw ShapeError("input too short for ContentVec");
        if (cv_sid) { pl.ops.fork(cv_sid); pl.ops.cur = cv_sid; }
        pl.cv_out = build_contentvec(e, pl, B, L);
        if (mode == 1) {
            const int T = pl.T, C = pl.C;
            pl.d_feat = pl.arena.floats((size_t)(2 * T + 1) * C);
            T1 cvo = pl.cv_out; float *df = pl.d_feat;
            dim3 grid(((2 * T + 1) * C + 255) / 256);
            pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(extract_feature_kernel, grid, dim3(256), 0, s, cvo.p, cvo.ld, C, T, df); });
        }
    }
    if (mode == 2) {
        float *pf; int *pi;
        build_f0(e, pl, B, L, frame16k, false, 0, &pf, &pi);
    }
    if (mode == 0) {
        const int T = pl.T, C = pl.C;
        const size_t T2 = 2 * (size_t)T + 1;
        const size_t hubert_length = std::min(L / 160, T2);                 // rvc.rs:153
        if ((size_t)skip_head + R > T2) throw PanicError("feature slice out of range (rvc.rs:155)");
        if (R < 1) throw ShapeError("return_length must be >= 1");
        if (e->sy->phone_dim != C) throw std::runtime_error("synthesizer phone dimension does not match the ContentVec output");
        T1 phone = make_t1(pl.arena, B, C, (int)R, 0);
        pl.op_phone = pl.ops.v.size();
        {
            T1 cvo = pl.cv_out; dim3 grid((C * (int)R + 255) / 256, B);
            pl.ops.push_back([=](hipStream_t s) {
                hipLaunchKernelGGL(gather_phone_kernel, grid, dim3(256), 0, s, cvo.p, cvo.ld, cvo.bs, C, T, (int)skip_head, (int)R, phone.p, phone.ld, phone.bs);
            });
        }
        pl.op_ret_begin = pl.ops.v.size();
        if (with_index) build_retrieval(e, pl, B, T, C, skip_head, R, phone);
        pl.op_ret_end = pl.ops.v.size();
        add_tap(pl, "phone_ct", phone);
        float *d_pitchf = d_pitchf0; int *d_pitch = d_pitch0;
        (void)hubert_length;
        pl.ops.cur = 0;
        if (rm_end > rm_begin) {
            // Two concurrent branches: f0 (ops [rm_begin, rm_end), aux stream 1) and ContentVec (ops [rm_end, here), main stream).
            // Launches reach the hardware queues in host order (~3 us each).  Eager: interleave the branches in proportion to
            // their lengths so both queues are fed from the start (the f0 branch is the longer one once they share the chip).
            // Graph replay submits a whole branch at a time: put ContentVec first, the f0 branch then starts ~0.2 ms late.
            OpList &ol = pl.ops;
            const size_t cv_end = ol.v.size(), na = rm_end - rm_begin, nb = cv_end - rm_end;
            for (size_t i = 0; i < rm_begin; i++) { ol.order_eager.push_back((int)i); ol.order_graph.push_back((int)i); }
            size_t ia = 0, ib = 0;
            while (ia < na || ib < nb) {
                const bool take_a = ib >= nb || (ia < na && (2 * ia + 1) * nb <= (2 * ib + 1) * na);
                ol.order_eager.push_back((int)(take_a ? rm_begin + ia++ : rm_end + ib++));
            }
            for (size_t i = rm_end; i < cv_end; i++) ol.order_graph.push_back((int)i);
            for (size_t i = rm_begin; i < rm_end; i++) ol.order_graph.push_back((int)i);
        }
        if (nof0) {
            // ContentVec -> gather (-> retrieval) -> synthesizer -> advance_chunk_kernel, nothing forked and nothing joined.  The pitch cache is not written;
            // the chunk counter advances (the prior's Philox stream reads it)
            build_synth(e, pl, B, phone, T1{}, nullptr, nullptr, 0, nullptr);
        } else {
        if (cv_sid) pl.ops.join(cv_sid);
        pl.ops.join(f0_sid);
        // consonant protection: `phone` is final (the retrieval has blended into it) and the pitch tail has written this call's pitchf rows; nothing of the
        // synthesizer is queued yet.  Behind op_ret_end, so recover_retrieval replays it with the rest of the chunk (on the re-gathered, re-blended phone)
        if (with_protect) {
            T1 cvo = pl.cv_out; const StreamState *stp = e->d_state; const float *pf = d_pitchf0;
            if (pl.key.with_taps && phone.bs == (long long)C * phone.ld && cvo.bs == (long long)C * cvo.ld) {       // (streams back to back, as make_t1 lays them out)
                // what the stage reads, every stream of the plan (phone_ct and cv.out are stream 0's): the blended rows [B][C][R] and the ContentVec output [B][C][T]
                T1 blend = phone; blend.B = 1; blend.C = B * C;
                add_tap(pl, "phone_blend", blend);
                T1 cva = cvo; cva.B = 1; cva.C = B * C;
                add_tap(pl, "cv.out_all", cva);
            }
            pl.ops.push_back([=](hipStream_t s) { launch_protect_mix(s, B, stp, pf, cvo.p, cvo.ld, cvo.bs, C, T, (int)skip_head, (int)R, phone.p, phone.ld, phone.bs); });
            // tap of every stream of the plan, stream-major [B][C][R] (the streams of a plan tensor lie back to back)
            T1 all = phone; all.B = 1; all.C = B * C;
            if (pl.key.with_taps) add_tap(pl, "phone_prot", all);
        }
        if (pl.key.with_taps) {
            // the call's pitchf rows as the synthesizer gets them, every stream of the plan: [B][R]
            T1 pft; pft.p = d_pitchf0; pft.B = 1; pft.C = B; pft.T = (int)R; pft.ld = (int)R; pft.halo = 0; pft.bs = (long long)B * R;
            add_tap(pl, "pitchf", pft);
        }
        // the NSF harmonic source is first needed by the decoder: it runs on a side stream next to the text encoder and the flow
        pl.ops.fork(2); pl.ops.cur = 2;
        src0 = build_nsf_source(e, pl, B, d_pitchf0);
        std::vector<T1> nz;
        const bool side_nz = !tune_env("RVC_NO_SIDE_NOISE_CONVS");
        if (side_nz) nz = build_noise_convs(e, pl, B, src0);
        pl.ops.cur = 0;
        build_synth(e, pl, B, phone, src0, d_pitchf, d_pitch, 2, side_nz ? &nz : nullptr);
        }
        StreamState *st = e->d_state;
        int *hst = e->h_status;      // (pinned host memory, mapped: the kernel writes the status words where the host reads them)
        pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(advance_chunk_kernel, dim3((B + 63) / 64), dim3(64), 0, s, st, B, hst); });
    }
    HIPCHK(hipDeviceSynchronize());
    e->last_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - build_t0).count();
    e->last_tuned = pl.tuned_layers; e->last_changed = pl.tune_changed; e->last_hits = pl.tune_hits; e->last_tune_ms = pl.tune_ms;
    evict_lru(e, (size_t)e->plan_cap - 1);      // bounded plan cache (rvc_set_plan_cache)
    e->plans.push_back(std::move(up));
    return e->plans.back().get();
}

static void run_plan(rvc_engine *e, Plan &pl);

static void issue_ops(rvc_engine *e, Plan &pl, bool capturing)
{
    // fork/join through events; under stream capture the auxiliary streams become parallel branches of the hipGraph
    const std::vector<int> &ord = capturing ? pl.ops.order_graph : pl.ops.order_eager;
    const size_t n = pl.ops.v.size();
    // Every op on the main stream: as a tuning aid (environment), and for the per-launch profile when the branches share the CUs
    // (more than 4 streams, no partition).  There a short f0 kernel that is co-scheduled with a 3 ms ContentVec GEMM is stretched to
    // the GEMM's length by the workgroup dispatcher (19 us alone, 3158 us measured); its HIP-event duration then says nothing about
    // the kernel.  With a CU partition the branches own disjoint CUs and are profiled as they run.
    const bool serial_env = test_opt("RVC_SERIAL_BRANCHES") != nullptr;
    const bool serial = serial_env || (pl.profile && !capturing && !e->partitioned);
    for (size_t k = 0; k < n; k++) {
        const size_t i = (k < ord.size() && !serial) ? (size_t)ord[k] : k;      // ops queued after the reordered prefix keep their position
        const int sid = serial ? 0 : pl.ops.sid[i];
        if (serial && pl.ops.kind[i] != 0) continue;
        hipStream_t st = sid == 0 ? e->stream : e->aux[sid - 1];
        if (pl.ops.kind[i] == 1) {
            if (e->pipe_now && (sid == 1 || sid == 3)) continue;      // pipelined: the front branches are ordered by events, not by the main stream
            HIPCHK(hipEventRecord(e->ev_fork[sid - 1], e->stream));
            HIPCHK(hipStreamWaitEvent(st, e->ev_fork[sid - 1], 0));
        } else if (pl.ops.kind[i] == 2) {
            HIPCHK(hipEventRecord(e->ev_join[sid - 1], st));
            HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join[sid - 1], 0));
        } else {
            pl.ops.v[i](st);
        }
    }
}

static void run_plan(rvc_engine *e, Plan &pl)
{
    pl.profile = e->profile_on;
    pl.prof_used = 0;
    // run-time speaker selection: a set call since the last chunk (or a late compose_flows under a mix) refolds the conditioned biases in place, one launch on
    // the main stream in front of the chunk -- behind the previous chunk's synthesizer, in front of this one's, eager, pipelined or replayed from a graph
    if (e->sy) e->sy->queue_speaker_fold(e->stream, e->profile_on);
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    if (e->use_graph && !e->profile_on) {
        if (!pl.graph_exec) {
            hipGraph_t g;
            HIPCHK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
            issue_ops(e, pl, true);
            HIPCHK(hipStreamEndCapture(e->stream, &g));
            HIPCHK(hipGraphInstantiate(&pl.graph_exec, g, nullptr, nullptr, 0));
            HIPCHK(hipGraphDestroy(g));
        }
        HIPCHK(hipGraphLaunch(pl.graph_exec, e->stream));
    } else {
        issue_ops(e, pl, false);
    }
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    HIPCHK(hipGetLastError());
    e->last_plan = &pl;
}


// ------------------------------- formant shift ----------------------------------------
static_assert(sizeof(StreamState) % 4 == 0, "state_gather_kernel copies StreamState in 32-bit words");

// the device form of the filter table o -> n, built once per engine (the descriptors of a captured graph's streams point at it)
static const FormantTable &formant_table_dev(rvc_engine *e, int o, int n)
{
    auto it = e->ftabs.find({o, n});
    if (it != e->ftabs.end()) return it->second;
    std::vector<float> ht; std::vector<int> kb; FormantTable t; t.o = o; t.n = n;
    formant_table_compact((size_t)o, (size_t)n, ht, kb, &t.w, &t.Kt);
    HIPCHK(hipMalloc(&t.tab, ht.size() * sizeof(float)));
    HIPCHK(hipMalloc(&t.kb, kb.size() * sizeof(int)));
    HIPCHK(hipMemcpy(t.tab, ht.data(), ht.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.kb, kb.data(), kb.size() * sizeof(int), hipMemcpyHostToDevice));
    return e->ftabs[{o, n}] = t;
}

// stream s of a call with return_length R: its decoder length R2 and whether it resamples (upp_res != upp)
static void formant_geo(rvc_engine *e, int s, uint32_t R, uint32_t *R2, bool *res)
{
    size_t r2 = R, ur = 0;
    const size_t upp = (size_t)e->sy->upp();
    if (R < 1) { *R2 = R; *res = false; return; }        // (rejected by the planner)
    if (!formant_geometry(R, (size_t)e->sy->sr, e->settings[s].formant, &r2, &ur)) throw ShapeError("formant shift: geometry out of range");
    *R2 = (uint32_t)r2; *res = ur != upp;
}

// the descriptor of stream s (StreamCtl::f) for return_length R
static FormantDesc formant_desc(rvc_engine *e, int s, uint32_t R)
{
    size_t R2 = R, ur = 0;
    const size_t upp = (size_t)e->sy->upp();
    FormantDesc d{};
    if (R < 1) return d;
    if (!formant_geometry(R, (size_t)e->sy->sr, e->settings[s].formant, &R2, &ur)) throw ShapeError("formant shift: geometry out of range");
    if (ur == upp) {
        if (R2 < R) throw ShapeError("formant shift: decoder shorter than the chunk");
        d.ident = 1;
        return d;
    }
    if ((size_t)R * ur > R2 * upp) throw ShapeError("formant shift: resampler input beyond the decoder output");
    const size_t g = formant_gcd(ur, upp);
    const FormantTable &t = formant_table_dev(e, (int)(ur / g), (int)(upp / g));
    d.tab = t.tab; d.kb = t.kb; d.o = t.o; d.n = t.n; d.w = t.w; d.kt = t.Kt; d.nx = (int)((size_t)R * ur);
    return d;
}

// the plan key of a set of streams (all of them: ids == nullptr) at return_length R -> false when their decoder lengths differ
static bool formant_key(rvc_engine *e, uint32_t R, const std::vector<int> *ids, uint32_t *R2, bool *fstage)
{
    const int n = ids ? (int)ids->size() : e->n_streams;
    bool any = false;
    for (int j = 0; j < n; j++) {
        uint32_t r2; bool res;
        formant_geo(e, ids ? (*ids)[j] : j, R, &r2, &res);
        if (j == 0) *R2 = r2;
        else if (r2 != *R2) return false;
        any = any || res;
    }
    *fstage = any || *R2 != R;
    return true;
}

// The key of the plan that serves a call: everything PlanKey holds but `slot` (the caller's), from the call's geometry and the engine's settings.  bucket_ids: the
// streams of a bucket plan (else every stream).  An infer key of streams whose formant shifts give different decoder lengths does not exist: callers ask
// formant_key first and bucket such streams by R2.
static PlanKey plan_key(rvc_engine *e, int mode, size_t L, size_t frame16k, uint32_t skip_head, uint32_t R, const std::vector<int> *bucket_ids = nullptr)
{
    PlanKey k;
    k.mode = mode; k.L = L; k.frame16k = frame16k; k.skip_head = skip_head; k.R = k.R2 = R;
    k.bucket = bucket_ids != nullptr; k.B = bucket_ids ? (int)bucket_ids->size() : e->n_streams;
    if (mode == 0 && !formant_key(e, R, bucket_ids, &k.R2, &k.fstage)) throw std::logic_error("plan key: streams with different decoder lengths");
    if (!k.fstage) k.R2 = R;
    // A model without pitch guidance (ModelSY::has_f0 false): its infer plan has no pitch branch, no source and no protect launch.  The
    // engine's f0 method and CREPE decoder are no part of such a plan's key; the hubert and pitch plans keep theirs
    const bool nof0 = mode == 0 && e->sy && !e->sy->has_f0;
    k.f0_method = nof0 ? 0 : e->f0_method;
    // a hybrid (rvc_load_f0_hybrid): the ordered members and the mode, and a member's setting where that member is present
    bool has_crepe = is_crepe(k.f0_method), has_fcpe = k.f0_method == RVC_F0_FCPE;
    if (k.f0_method == RVC_F0_HYBRID) {
        k.hybrid = hybrid_pack(e->hybrid_m, e->hybrid_n); k.hybrid_mode = e->hybrid_mode;
        for (int i = 0; i < e->hybrid_n; i++) { has_crepe = has_crepe || is_crepe(e->hybrid_m[i]); has_fcpe = has_fcpe || e->hybrid_m[i] == RVC_F0_FCPE; }
    }
    k.crepe_decoder = has_crepe ? e->crepe_decoder : 0;
    k.fcpe_threshold = has_fcpe ? e->fcpe_threshold : 0.0;          // FCPE's voicing threshold is baked into its decoder's launch
    // f0 from outside: whether ANY stream of the plan brings an override -- or the call is a conversion window under a curve -- decides the
    // plan's launch list (the rule of with_protect); which values is no part of the key.  A model without pitch guidance ignores both
    if (!nof0 && mode != 1 && k.f0_method) {
        if (e->conv_curve) k.f0_override = mode == 0;
        else for (int j = 0; j < k.B; j++) { const size_t s = (size_t)(bucket_ids ? (*bucket_ids)[j] : j); k.f0_override = k.f0_override || (s < e->ov.size() && !e->ov[s].empty()); }
    }
    k.with_index = mode == 0 && e->index.rows && e->index_rate > 0.f;
    // consonant protection (protect.hip.h): one more launch, only on plans that use the index and only when one of the plan's streams has it on.  Which value
    // a stream has is no part of the key: the kernel reads it every chunk.  (Upstream applies protect only where it has a pitch)
    if (k.with_index && !nof0)
        for (int j = 0; j < k.B; j++) k.with_protect = k.with_protect || e->settings[bucket_ids ? (*bucket_ids)[j] : j].protect < PROTECT_OFF;
    k.bf3 = e->gemm_precision == 1; k.with_taps = e->taps_on != 0; k.plain_plan = e->taps_on == 1;
    k.nprobe = k.with_index ? e->index_nprobe : 0; k.knn_k = k.with_index ? e->index_k : KNN_K;
    return k;
}

// what the index builder (retrieval.hip) needs of the planner: rvc_hubert's plan whatever the stream count, and one run of it
Plan *hubert_plan(rvc_engine *e, size_t L)
{
    struct One { rvc_engine *e; int n; explicit One(rvc_engine *e_) : e(e_), n(e_->n_streams) { e->n_streams = 1; } ~One() { e->n_streams = n; } } one(e);
    return get_plan(e, plan_key(e, 1, L, 0, 0, 0));
}
void run_hubert_plan(rvc_engine *e, Plan &pl) { run_plan(e, pl); }

static float uppower(int32_t pitch_shift) { return ldexpf(1.0f, pitch_shift / 12); }   // rvc.rs:121, truncating division (Q1)

// Per-call parameters: the seed (CallParams) and the controls of every stream (StreamState::ctl: every stream of a batch is its own caller with its own
// settings, obs-rvc/src/lib.rs:701-707).  The multiplier: uppower(pitch_shift) -- shifts == nullptr: `pitch_shift` for every stream --, with Rs (infer calls: the
// return_length of every stream) times the stream's formant factor (float)2^(-phi / 12), and a semitone transpose st != 0 multiplies (float)2^(st / 12) in last
// (st = 0 multiplies by nothing).  The formant descriptor is made for Rs; without Rs (hubert / pitch) the descriptors stay what the device holds.
// neutral (rvc_analyze_f0): the multiplier is 1 and every pitch control is off whatever the streams' settings say -- the tracker's own rows come out of the tail;
// the settings themselves are not touched, and the next call pushes them again because the block it compares against differs.
// rvc_engine::auto_mul (a conversion under auto-transpose): one more factor behind the semitone factor; rvc_engine::many_mul (rvc_convert_many with a per-file
// pitch): the same, per stream
static void push_call_params(rvc_engine *e, int32_t pitch_shift, const int32_t *shifts = nullptr, const uint32_t *Rs = nullptr, bool neutral = false)
{
    const int B = e->n_streams;
    std::vector<StreamCtl> ctl((size_t)B, StreamCtl{});
    const bool keep_f = !Rs && (int)e->pushed_ctl.size() == B;
    for (int b = 0; b < B; b++) {
        const rvc_engine::StreamSettings &set = e->settings[b];
        StreamCtl &c = ctl[b];
        c.uppower = uppower(shifts ? shifts[b] : pitch_shift);
        if (Rs) {
            c.uppower *= (float)std::pow(2.0, -set.formant / 12.0);
            c.f = formant_desc(e, b, Rs[b]);
        } else if (keep_f) c.f = e->pushed_ctl[b].f;
        if (neutral) { c.c = f0cond_pack(0.f, INFINITY, 0, 0u, 0.f); c.protect = (float)set.protect; continue; }
        if (set.pitch.semitones != 0.0) c.uppower *= (float)std::pow(2.0, set.pitch.semitones / 12.0);
        if (e->auto_mul != 0.f) c.uppower *= e->auto_mul;
        if ((size_t)b < e->many_mul.size() && e->many_mul[b] != 0.f) c.uppower *= e->many_mul[b];
        c.c = f0cond_pack(set.pitch.lo, set.pitch.hi, set.pitch.radius, set.pitch.mask, set.pitch.strength);
        c.protect = (float)set.protect;
    }
    // The device already holds these values (every write to them is ordered on the main stream, and the last one wrote exactly this):
    // nothing to copy -- a small H2D copy is a 4-5 us blit kernel in front of both branches of every chunk otherwise.
    if (e->pushed_valid && e->pushed_seed == e->seed && e->pushed_ctl == ctl) return;
    if (e->pipeline) HIPCHK(hipDeviceSynchronize());   // the f0 branch of the next chunk may already be running: drain before the values change
    // every call writes its own pinned block: an unsynchronised call's copy may still be pending when the next call arrives
    if (!e->pushed_valid || e->pushed_seed != e->seed) {
        CallParams *h = e->h_cp + (e->cp_slot++ & 63u);
        h->uppower = uppower(shifts ? shifts[0] : pitch_shift);
        h->seed = e->seed;
        h->chunk_base = 0;
        HIPCHK(hipMemcpyAsync(e->d_cp, h, sizeof(CallParams), hipMemcpyHostToDevice, e->stream));
    }
    // a block is rewritten only after the strided copy that last read it has completed (nine unsynchronised calls with changing shifts
    // would otherwise overwrite a block whose copy is still pending: ADVICE r3)
    const unsigned us = e->up_slot++ & 7u;
    if (e->ev_up_used[us]) HIPCHK(hipEventSynchronize(e->ev_up[us]));
    StreamCtl *h = e->h_ctl + (size_t)us * 4096;
    std::copy(ctl.begin(), ctl.end(), h);
    HIPCHK(hipMemcpy2DAsync((char *)e->d_state + offsetof(StreamState, ctl), sizeof(StreamState), h, sizeof(StreamCtl), sizeof(StreamCtl), (size_t)B, hipMemcpyHostToDevice, e->stream));
    e->pushed_ctl = std::move(ctl);
    if (!e->ev_up[us]) HIPCHK(hipEventCreateWithFlags(&e->ev_up[us], hipEventDisableTiming));
    HIPCHK(hipEventRecord(e->ev_up[us], e->stream)); e->ev_up_used[us] = true;
    e->pushed_seed = e->seed; e->pushed_valid = true;
    if (e->pipeline) {
        // pipelined calls do not fork the front branches from the main stream: order them behind the parameter copy explicitly
        HIPCHK(hipEventRecord(e->ev_cp, e->stream));
        HIPCHK(hipStreamWaitEvent(e->aux[0], e->ev_cp, 0));
        HIPCHK(hipStreamWaitEvent(e->aux[2], e->ev_cp, 0));
    }
}

// f0 from outside: what a call does about the pending overrides.
// override_fits: an override longer than the plan's f0 window is refused by the call that would consume it, before anything is queued.
static void override_fits(rvc_engine *e, const Plan &pl, const std::vector<int> *ids = nullptr)
{
    if (!pl.key.f0_override || e->conv_curve) return;
    for (int j = 0; j < pl.key.B; j++) {
        const size_t s = (size_t)(ids ? (*ids)[j] : j);
        if (s < e->ov.size() && e->ov[s].size() > (size_t)pl.Tm) throw ShapeError("f0 override: more rows than the call's f0 window has");
    }
}
// push_overrides: in front of a chunk whose plan has the select, the override block goes to the device when it is behind the host's -- the call, the counts and the
// rows of the streams that have any, from one pinned block -- on the stream the chunk's f0 branch is ordered behind: the main stream (the branch forks from it;
// a replayed graph is launched into it; the copy is never captured), or the f0 stream itself for a pipelined call, whose front branches do not fork.
static void push_overrides(rvc_engine *e, const Plan &pl, bool pipe)
{
    if (!pl.key.f0_override || !e->d_ov) return;
    if (!e->conv_curve && !e->ov_dirty) return;
    hipStream_t cs = pipe ? e->aux[0] : e->stream;
    if (e->ov_stream && e->ov_stream != cs) HIPCHK(hipStreamSynchronize(e->ov_stream));      // (a call of the other kind: its copies and its select ran over there)
    e->ov_stream = cs;
    const size_t S = e->ov.size(), head = 64 + S * sizeof(int);
    size_t need = head;
    if (!e->conv_curve) for (auto &v : e->ov) need += v.size() * sizeof(float);
    rvc_engine::OvBlock &blk = e->ov_ring[e->ov_slot++ & 7u];
    if (blk.used) HIPCHK(hipEventSynchronize(blk.ev));      // a block is rewritten only after the copies that read it have completed
    if (blk.cap < need) {
        if (blk.p) (void)hipHostFree(blk.p);
        blk.p = nullptr; blk.cap = 0;
        const size_t cap = (need + 4095) / 4096 * 4096;
        HIPCHK(hipHostMalloc((void **)&blk.p, cap));
        blk.cap = cap;
    }
    memset(blk.p, 0, head);
    F0OvCall *call = (F0OvCall *)blk.p; int *cnt = (int *)(blk.p + 64);
    if (e->conv_curve) *call = e->conv_call;
    else for (size_t s = 0; s < S; s++) cnt[s] = (int)e->ov[s].size();
    HIPCHK(hipMemcpyAsync(e->d_ov, blk.p, head, hipMemcpyHostToDevice, cs));
    if (!e->conv_curve) {
        size_t at = head;
        for (size_t s = 0; s < S; s++) {
            const size_t nb = e->ov[s].size() * sizeof(float);
            if (!nb) continue;
            memcpy(blk.p + at, e->ov[s].data(), nb);
            HIPCHK(hipMemcpyAsync(e->d_ov + ov_rows_off(S) + s * F0_OV_ROWS * sizeof(float), blk.p + at, nb, hipMemcpyHostToDevice, cs));
            at += nb;
        }
    }
    if (!blk.ev) HIPCHK(hipEventCreateWithFlags(&blk.ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(blk.ev, cs)); blk.used = true;
    e->ov_dirty = e->conv_curve;      // (a conversion leaves its own call in the block)
}
// consume_overrides: behind the call that read them, unless they are held
static void consume_overrides(rvc_engine *e, const std::vector<int> *ids = nullptr)
{
    if (e->ov_hold) return;
    const size_t n = ids ? ids->size() : e->ov.size();
    for (size_t j = 0; j < n; j++) {
        const size_t s = ids ? (size_t)(*ids)[j] : j;
        if (s < e->ov.size() && !e->ov[s].empty()) { e->ov[s].clear(); e->ov_dirty = true; }
    }
}

// Status words of all streams (0 ok, 6 = the reference would have panicked at rmvpe.rs:124, 7 = GRU hand-off time-out): one strided
// copy into pinned memory, queued in front of the call's final synchronisation so that reading them costs no extra round trip.
static void queue_status(rvc_engine *e)
{
    HIPCHK(hipMemcpy2DAsync(e->h_status, sizeof(int), (char *)e->d_state + offsetof(StreamState, status), sizeof(StreamState), sizeof(int), (size_t)e->n_streams,
                            hipMemcpyDeviceToHost, e->stream));
    e->status_queued = true;
}

// -> RVC_OK / RVC_PANIC / RVC_BACKEND, or RVC_KNN_RETRY (internal): only the one-launch retrieval reported (ST_KNN_TIMEOUT) -- its counters are
// re-armed here and the caller may recompute the chunk from the retrieval on (recover_retrieval).  Every stream's word is looked at before anything
// is decided: a lost GRU hand-off on ANY stream means the plans are rebuilt, whatever a lower-numbered stream reported.
static const rvc_status RVC_KNN_RETRY = (rvc_status)100;
static rvc_status check_status(rvc_engine *e)
{
    if (!e->status_queued) { queue_status(e); HIPCHK(hipStreamSynchronize(e->stream)); }
    e->status_queued = false;
    int any = 0;
    for (int b = 0; b < e->n_streams; b++) any |= e->h_status[b];
    if (!any) return RVC_OK;
    const int zero = 0;
    for (int c = 0; c < e->n_streams; c++)
        if (e->h_status[c] != 0) { HIPCHK(hipMemcpy((char *)(e->d_state + c) + offsetof(StreamState, status), &zero, sizeof(int), hipMemcpyHostToDevice)); e->h_status[c] = 0; }
    if (any & ST_HANDOFF) {
        // a GRU step that gave up waiting left its hand-off granules behind: the plans are rebuilt before the next call
        drop_plans(e);
        e->err = "a cross-workgroup hand-off timed out (GRU recurrence)";
        return RVC_BACKEND;
    }
    if (any & ST_KNN_TIMEOUT) {
        // the retrieval's counters were poisoned by the selector that gave up (knn.hip.h): re-arm them, whatever else happens
        HIPCHK(hipDeviceSynchronize());
        for (auto &p : e->plans) if (p->knn_ticket) HIPCHK(hipMemset(p->knn_ticket, 0, p->knn_ticket_bytes));
    }
    if (any & ST_PANIC) {
        e->err = "to_local_average_cents: index out of bounds (argmax bin >= 348), the reference panics here";
        return RVC_PANIC;
    }
    e->err = "the one-launch retrieval's hand-off timed out";
    return RVC_KNN_RETRY;
}

// A selector of knn_scan_select_kernel gave up (a workgroup of the launch did not arrive in time -- e.g. a GPU shared with another process): some
// queries of the chunk were not blended.  Nothing is lost: the inputs of the retrieval (ContentVec output, pitch) are still in the plan's arena.
// Rewind the chunk counters, then run [phone gather] + [exhaustive exact scan, merge, blend: the definition] + [everything behind the retrieval]
// in list order on the main stream.  Same hits (the one-launch form is tested bit-exact against this scan), same PCM.
static rvc_status final_status(rvc_engine *e)      // callers that cannot recompute the chunk: the internal retry code becomes an error
{
    const rvc_status st = check_status(e);
    return st == RVC_KNN_RETRY ? RVC_BACKEND : st;
}
static rvc_status recover_retrieval(rvc_engine *e, Plan &pl)
{
    if (pl.knn_fallback.empty() || pl.op_ret_end <= pl.op_ret_begin) { e->err = "the one-launch retrieval's hand-off timed out (no fallback on this plan)"; return RVC_BACKEND; }
    hipLaunchKernelGGL(rewind_chunk_kernel, dim3((pl.key.B + 63) / 64), dim3(64), 0, e->stream, e->d_state, pl.key.B);
    const size_t n = pl.ops.v.size();
    for (size_t i = pl.op_phone; i < pl.op_ret_begin; i++) if (pl.ops.kind[i] == 0) pl.ops.v[i](e->stream);
    for (auto &op : pl.knn_fallback) op(e->stream);
    for (size_t i = pl.op_ret_end; i < n; i++) if (pl.ops.kind[i] == 0) pl.ops.v[i](e->stream);
    HIPCHK(hipGetLastError());
    e->knn_recoveries++;
    return RVC_OK;
}

// Streams in buckets (rvc_infer_batch_g: one per geometry; the other infer calls: one per formant decoder length R2): every bucket runs as one batch
// through its own plan on a gathered copy of its streams' states (pitch cache, counters, status, multiplier, formant descriptor), scattered back
// afterwards.  in(s) / out(s): stream s's input / output buffer.
struct BucketRun { Plan *pl; std::vector<int> ids; };
// the gathered state block the bucket plans are built on (their kernels bake its address): allocated before the first bucket plan
static void ensure_bucket_state(rvc_engine *e)
{
    if (!e->d_state_bucket) { HIPCHK(hipMalloc(&e->d_state_bucket, sizeof(StreamState) * e->n_streams)); HIPCHK(hipMalloc(&e->d_bucket_idx, sizeof(int) * e->n_streams)); }
}
static rvc_status run_buckets(rvc_engine *e, std::vector<BucketRun> &work, const std::function<const void *(int)> &in, bool in_dev,
                              const std::function<void *(int)> &out, bool out_dev)
{
    for (auto &w : work)
        { bool ok = false; for (auto &p : e->plans) ok = ok || p.get() == w.pl; if (!ok) throw std::logic_error("bucketed call: a plan of this call left the cache"); }
    for (auto &w : work) override_fits(e, *w.pl, &w.ids);
    for (auto &w : work) {
        Plan *pl = w.pl; const std::vector<int> &ids = w.ids; const int Bk = (int)ids.size();
        push_overrides(e, *pl, false);
        HIPCHK(hipMemcpyAsync(e->d_bucket_idx, ids.data(), sizeof(int) * Bk, hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(state_gather_kernel, dim3(Bk), dim3(256), 0, e->stream, e->d_state, e->d_state_bucket, e->d_bucket_idx, 0);
        for (int j = 0; j < Bk; j++) HIPCHK(hipMemcpyAsync(pl->d_in + (size_t)j * pl->key.L, in(ids[j]), pl->key.L * sizeof(float), in_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
        pl->cur_in = nullptr; pl->cur_out = nullptr;
        run_plan(e, *pl);
        for (int j = 0; j < Bk; j++) HIPCHK(hipMemcpyAsync(out(ids[j]), pl->audio.p + (size_t)j * pl->N, pl->N * sizeof(float), out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream));
        hipLaunchKernelGGL(state_gather_kernel, dim3(Bk), dim3(256), 0, e->stream, e->d_state, e->d_state_bucket, e->d_bucket_idx, 1);
        consume_overrides(e, &ids);
        HIPCHK(hipStreamSynchronize(e->stream));        // (ids / the pinned-less host buffers of this bucket are free again; the next bucket reuses the state block)
    }
    e->last_knn_rows = 0;
    queue_status(e);                                     // the streams' own status words (the plans wrote bucket-local ones)
    HIPCHK(hipStreamSynchronize(e->stream));
    return final_status(e);
}

static std::string native_path(const std::string &p)
{
    if (p.size() > 5 && p.substr(p.size() - 5) == ".onnx") return p.substr(0, p.size() - 5) + ".rvcw";
    return p;
}

}  // namespace rvc

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
extern "C" {

// rvc_version(): version.cpp; rvc_debug_option: plan.hip; the index entry points: retrieval.hip

rvc_status rvc_create(const char *data_path, int device, rvc_engine **out)
{
    if (!out) return RVC_BACKEND;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return RVC_BACKEND;   // no CPU fallback, by design
    rvc_engine *e = new rvc_engine();
    e->data_path = data_path ? data_path : "";
    if (device < 0) { const char *lr = getenv("LOCAL_RANK"); device = lr ? atoi(lr) % ndev : 0; }
    e->device = device;
    try {
        set_device(e);
        for (int i = 0; i < 3; i++) { HIPCHK(hipEventCreateWithFlags(&e->ev_fork[i], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&e->ev_join[i], hipEventDisableTiming)); }
        e->partition_ok = !tune_env("RVC_NO_CUMASK");
        configure_aux_streams(e);
        HIPCHK(hipEventCreate(&e->ev0)); HIPCHK(hipEventCreate(&e->ev1));
        HIPCHK(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
        HIPCHK(hipMalloc(&e->d_cp, sizeof(CallParams)));
        HIPCHK(hipHostMalloc((void **)&e->h_cp, 64 * sizeof(CallParams)));
        HIPCHK(hipEventCreateWithFlags(&e->ev_cp, hipEventDisableTiming));
        HIPCHK(hipHostMalloc((void **)&e->h_status, 4096 * sizeof(int)));
        memset(e->h_status, 0, 4096 * sizeof(int));
        HIPCHK(hipHostMalloc((void **)&e->h_ctl, (size_t)8 * 4096 * sizeof(StreamCtl)));
        init_constants(e);
        alloc_state(e);
    } catch (const std::exception &x) {
        fprintf(stderr, "rvc_create: %s\n", x.what());
        release_stream_set(e->sset);
        delete e;
        return RVC_BACKEND;
    }
    *out = e;
    return RVC_OK;
}

void rvc_destroy(rvc_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    e->plans.clear();
    index_build_abort(e);
    e->cv.reset(); e->rm.reset(); e->cr_full.reset(); e->cr_tiny.reset(); e->fc.reset(); e->sy.reset();
    wfree(e->d_window); wfree(e->d_twiddle); wfree(e->d_basis);      // (upload_f: slab memory)
    if (e->d_band) (void)hipFree(e->d_band);
    if (e->d_state) (void)hipFree(e->d_state);
    if (e->d_state_bucket) (void)hipFree(e->d_state_bucket);
    if (e->d_bucket_idx) (void)hipFree(e->d_bucket_idx);
    if (e->d_cp) (void)hipFree(e->d_cp);
    if (e->h_cp) (void)hipHostFree(e->h_cp);
    if (e->h_status) (void)hipHostFree(e->h_status);
    if (e->h_ctl) (void)hipHostFree(e->h_ctl);
    if (e->d_ov) (void)hipFree(e->d_ov);
    for (auto &b : e->ov_ring) { if (b.p) (void)hipHostFree(b.p); if (b.ev) (void)hipEventDestroy(b.ev); }
    for (auto &kv : e->ftabs) { (void)hipFree(kv.second.tab); (void)hipFree(kv.second.kb); }
    for (int i = 0; i < 8; i++) if (e->ev_up[i]) (void)hipEventDestroy(e->ev_up[i]);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->ev_in) (void)hipEventDestroy(e->ev_in);
    if (e->ev_cp) (void)hipEventDestroy(e->ev_cp);
    for (int i = 0; i < 3; i++) {
        if (e->ev_fork[i]) (void)hipEventDestroy(e->ev_fork[i]);
        if (e->ev_join[i]) (void)hipEventDestroy(e->ev_join[i]);
    }
    release_stream_set(e->sset);      // (the streams stay in the per-device pool)
    delete e;
}

const char *rvc_last_error_message(rvc_engine *e) { return e ? e->err.c_str() : "null engine"; }
int rvc_device(rvc_engine *e) { return e ? e->device : -1; }

// rvc.rs:46-54 + models.rs:52-64
rvc_status rvc_load_contentvec(rvc_engine *e, int model_version)
{
    return guarded(e, [&]() {
        const int dim = model_version == RVC_VERSION_V1 ? 256 : 768, layer = model_version == RVC_VERSION_V1 ? 9 : 12;   // enums.rs:10-23
        char name[64]; snprintf(name, sizeof name, "vec-%d-layer-%d.rvcw", dim, layer);
        Blob b(e->data_path + "/contentvec/" + name);
        drop_plans(e);
        e->cv.reset(new ModelCV(b));
        configure_aux_streams(e);       // (the f0 partition depends on the ContentVec depth)
        return RVC_OK;
    });
}
// rvc.rs:56-60
rvc_status rvc_load_model(rvc_engine *e, const char *model_path)
{
    return guarded(e, [&]() {
        Blob b(native_path(model_path ? model_path : ""));
        drop_plans(e);
        e->sy.reset(new ModelSY(b));
        return RVC_OK;
    });
}
// rvc.rs:62-75 + models.rs:66-76
rvc_status rvc_load_f0(rvc_engine *e, int pitch_algorithm)
{
    (void)pitch_algorithm;   // only Rmvpe exists (enums.rs:26-28); unknown values map to it (enums.rs:96-103)
    return guarded(e, [&]() {
        Blob b(e->data_path + "/f0/rmvpe.rvcw");
        drop_plans(e);
        e->rm.reset(new ModelRM(b));
        e->f0_method = RVC_F0_RMVPE; e->hybrid_n = 0;
        return RVC_OK;
    });
}
// the f0 method by its own constants (rvc_load_f0 keeps the reference's one-variant enum): RMVPE loads its weights, YIN and PM have none.  The method is part of
// a plan's key, so a plan built for one never serves the other.
rvc_status rvc_load_f0_method(rvc_engine *e, int method)
{
    if (method == RVC_F0_RMVPE) return rvc_load_f0(e, RVC_PITCH_RMVPE);
    return guarded(e, [&]() {
        if (is_crepe(method)) {
            // a preset is read once and kept: the plans built on its weights stay valid, so going back to it finds them
            std::unique_ptr<ModelCR> &slot = method == RVC_F0_CREPE ? e->cr_full : e->cr_tiny;
            if (!slot) {
                Blob b(e->data_path + (method == RVC_F0_CREPE ? "/f0/crepe-full.rvcw" : "/f0/crepe-tiny.rvcw"));
                slot.reset(new ModelCR(b));
            }
            e->f0_method = method; e->hybrid_n = 0;
            return RVC_OK;
        }
        if (method == RVC_F0_FCPE) {
            if (!e->fc) { Blob b(e->data_path + "/f0/fcpe.rvcw"); e->fc.reset(new ModelFC(b)); }          // read once and kept, as the CREPE presets are
            e->f0_method = method; e->hybrid_n = 0;
            return RVC_OK;
        }
        if (method == RVC_F0_HYBRID) throw ShapeError("f0 method: RVC_F0_RMVPE, RVC_F0_YIN, RVC_F0_CREPE, RVC_F0_CREPE_TINY, RVC_F0_FCPE or RVC_F0_PM (RVC_F0_HYBRID names no members: rvc_load_f0_hybrid)");
        if (method != RVC_F0_YIN && method != RVC_F0_PM) throw ShapeError("f0 method: RVC_F0_RMVPE, RVC_F0_YIN, RVC_F0_CREPE, RVC_F0_CREPE_TINY, RVC_F0_FCPE or RVC_F0_PM");
        e->f0_method = method; e->hybrid_n = 0;          // (YIN and PM have no weights)
        return RVC_OK;
    });
}
// Hybrid f0: `n` distinct single methods, the first one the lead, combined per frame under `mode`.  Every member is loaded as
// rvc_load_f0_method loads it -- RMVPE's file is read again and the plans are dropped, a CREPE preset and FCPE are read once and kept -- but all files are read
// before anything of the engine changes: a refusal leaves the method, the members and the loaded weights as they were.
rvc_status rvc_load_f0_hybrid(rvc_engine *e, const int *methods, int n, int mode)
{
    return guarded(e, [&]() {
        if (!methods || n < 1 || n > HYBRID_MEMBERS_MAX) throw ShapeError("f0 hybrid: 1 to 4 members");
        if (mode != RVC_HYBRID_VOTE && mode != RVC_HYBRID_MEDIAN) throw ShapeError("f0 hybrid: mode RVC_HYBRID_VOTE or RVC_HYBRID_MEDIAN");
        for (int i = 0; i < n; i++) {
            const int m = methods[i];
            if (m != RVC_F0_RMVPE && m != RVC_F0_YIN && !is_crepe(m) && m != RVC_F0_FCPE && m != RVC_F0_PM)
                throw ShapeError("f0 hybrid: a member is RVC_F0_RMVPE, RVC_F0_YIN, RVC_F0_CREPE, RVC_F0_CREPE_TINY, RVC_F0_FCPE or RVC_F0_PM");
            for (int j = 0; j < i; j++) if (methods[j] == m) throw ShapeError("f0 hybrid: a member is named twice");
        }
        std::unique_ptr<ModelRM> rm; std::unique_ptr<ModelCR> cr_full, cr_tiny; std::unique_ptr<ModelFC> fc;
        for (int i = 0; i < n; i++) {
            const int m = methods[i];
            if (m == RVC_F0_RMVPE) { Blob b(e->data_path + "/f0/rmvpe.rvcw"); rm.reset(new ModelRM(b)); }
            else if (m == RVC_F0_CREPE && !e->cr_full) { Blob b(e->data_path + "/f0/crepe-full.rvcw"); cr_full.reset(new ModelCR(b)); }
            else if (m == RVC_F0_CREPE_TINY && !e->cr_tiny) { Blob b(e->data_path + "/f0/crepe-tiny.rvcw"); cr_tiny.reset(new ModelCR(b)); }
            else if (m == RVC_F0_FCPE && !e->fc) { Blob b(e->data_path + "/f0/fcpe.rvcw"); fc.reset(new ModelFC(b)); }
        }
        if (rm) { drop_plans(e); e->rm = std::move(rm); }      // (as rvc_load_f0: the plans were built on the weights replaced here)
        if (cr_full) e->cr_full = std::move(cr_full);
        if (cr_tiny) e->cr_tiny = std::move(cr_tiny);
        if (fc) e->fc = std::move(fc);
        e->f0_method = RVC_F0_HYBRID; e->hybrid_n = n; e->hybrid_mode = mode;
        for (int i = 0; i < HYBRID_MEMBERS_MAX; i++) e->hybrid_m[i] = i < n ? methods[i] : 0;
        return RVC_OK;
    });
}
// the members (the lead first; at most `cap` are written) and the mode of the hybrid in force -> its number of members, 0 when the method is no hybrid
int rvc_f0_hybrid(rvc_engine *e, int *methods, int cap, int *mode)
{
    if (!e || e->f0_method != RVC_F0_HYBRID) return 0;
    for (int i = 0; i < e->hybrid_n && i < cap && methods; i++) methods[i] = e->hybrid_m[i];
    if (mode) *mode = e->hybrid_mode;
    return e->hybrid_n;
}
int rvc_f0_method(rvc_engine *e) { return e ? e->f0_method : 0; }
// the kind of the loaded synthesizer: 1 = trained with pitch guidance, 0 = without (config key f0 = 0: no tracker runs), -1 = none loaded
int rvc_model_has_f0(rvc_engine *e) { return e && e->sy ? (e->sy->has_f0 ? 1 : 0) : -1; }
// CREPE's decoder (crepe_decode_kernel): part of a CREPE plan's key, so a plan built for one never serves the other
rvc_status rvc_set_crepe_decoder(rvc_engine *e, int decoder)
{
    return guarded(e, [&]() {
        if (decoder != RVC_CREPE_VITERBI && decoder != RVC_CREPE_ARGMAX) throw ShapeError("crepe decoder: RVC_CREPE_VITERBI or RVC_CREPE_ARGMAX");
        e->crepe_decoder = decoder;
        return RVC_OK;
    });
}
int rvc_crepe_decoder(rvc_engine *e) { return e ? e->crepe_decoder : 0; }
// FCPE's voicing threshold (fcpe_decode_kernel): part of an FCPE plan's key, so a changed value holds from the next call on
rvc_status rvc_set_fcpe_threshold(rvc_engine *e, double threshold)
{
    return guarded(e, [&]() {
        if (!(threshold >= 0.0 && threshold < 1.0)) throw ShapeError("fcpe threshold: a value in [0, 1)");
        e->fcpe_threshold = threshold;
        return RVC_OK;
    });
}
double rvc_fcpe_threshold(rvc_engine *e) { return e ? e->fcpe_threshold : 0.0; }
// Run-time speaker selection (model_synth.hip, speaker.hip.h).  The setting is the model's: a load or an unload puts it back to
// "the speaker is sy.g".  A set call only records the mix; the fold is queued by the next chunk (run_plan), so no call here touches the device.
int rvc_model_speakers(rvc_engine *e) { return e && e->sy ? e->sy->n_spk : 0; }
rvc_status rvc_set_speaker_mix(rvc_engine *e, const int32_t *sid, const double *weight, size_t n)
{
    return guarded(e, [&]() {
        if (!e->sy) return RVC_MODEL_NOT_LOADED;
        e->sy->set_speaker_mix(sid, weight, n);
        return RVC_OK;
    });
}
rvc_status rvc_set_speaker(rvc_engine *e, int sid)
{
    const int32_t id = (int32_t)sid; const double one = 1.0;
    return rvc_set_speaker_mix(e, &id, &one, 1);
}
rvc_status rvc_speaker_mix(rvc_engine *e, int32_t *sid, double *weight, size_t cap, size_t *n)
{
    return guarded(e, [&]() {
        if (!e->sy) return RVC_MODEL_NOT_LOADED;
        const ModelSY &m = *e->sy;
        if (n) *n = (size_t)m.mix_n;
        if (cap < (size_t)m.mix_n) return RVC_SHAPE;
        for (int i = 0; i < m.mix_n; i++) { if (sid) sid[i] = m.mix_id[i]; if (weight) weight[i] = m.mix_w[i]; }
        return RVC_OK;
    });
}
// rvc.rs:77-79
void rvc_unload_model(rvc_engine *e)
{
    if (!e) return;
    (void)guarded(e, [&]() { drop_plans(e); e->sy.reset(); return RVC_OK; });
}

static rvc_status run_single_input(rvc_engine *e, Plan *pl, const float *input, size_t n, int32_t pitch_shift)
{
    HIPCHK(hipMemcpyAsync(pl->d_in, input, n * sizeof(float) * (size_t)pl->key.B, hipMemcpyHostToDevice, e->stream));
    push_call_params(e, pitch_shift);
    run_plan(e, *pl);
    return RVC_OK;
}

// rvc.rs:81-97
rvc_status rvc_hubert(rvc_engine *e, const float *input, size_t n, float *out, size_t cap, size_t dims[3])
{
    return guarded(e, [&]() {
        if (!e->cv) return RVC_CONTENTVEC_NOT_LOADED;
        if (e->n_streams != 1) throw ShapeError("hubert() is a single-stream call");
        Plan *pl = get_plan(e, plan_key(e, 1, n, 0, 0, 0));
        dims[0] = 1; dims[1] = (size_t)pl->C; dims[2] = (size_t)pl->T;
        if (cap < (size_t)pl->C * pl->T) return RVC_SHAPE;
        run_single_input(e, pl, input, n, 0);
        HIPCHK(hipMemcpy2DAsync(out, (size_t)pl->T * 4, pl->cv_out.p, (size_t)pl->cv_out.ld * 4, (size_t)pl->T * 4, pl->C, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return RVC_OK;
    });
}
// rvc.rs:99-109
rvc_status rvc_extract_feature(rvc_engine *e, const float *input, size_t n, float *out, size_t cap, size_t dims[3])
{
    return guarded(e, [&]() {
        if (!e->cv) return RVC_CONTENTVEC_NOT_LOADED;
        if (e->n_streams != 1) throw ShapeError("extract_feature() is a single-stream call");
        Plan *pl = get_plan(e, plan_key(e, 1, n, 0, 0, 0));
        const size_t T2 = 2 * (size_t)pl->T + 1;
        dims[0] = 1; dims[1] = T2; dims[2] = (size_t)pl->C;
        if (cap < T2 * pl->C) return RVC_SHAPE;
        run_single_input(e, pl, input, n, 0);
        HIPCHK(hipMemcpyAsync(out, pl->d_feat, T2 * pl->C * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return RVC_OK;
    });
}
// rvc.rs:111-131
rvc_status rvc_pitch(rvc_engine *e, const float *input, size_t n, int32_t pitch_shift, size_t sample_frame_16k_size, float *out, size_t cap, size_t *out_len)
{
    return guarded(e, [&]() {
        if (!e->f0_method) return RVC_F0_NOT_LOADED;   // the reference hits unreachable!() here (rvc.rs:125)
        if (e->n_streams != 1) throw ShapeError("pitch() is a single-stream call");
        Plan *pl = get_plan(e, plan_key(e, 2, n, sample_frame_16k_size, 0, 0));
        *out_len = (size_t)pl->Tm;
        if (cap < (size_t)pl->Tm) return RVC_SHAPE;
        override_fits(e, *pl);
        push_overrides(e, *pl, false);
        run_single_input(e, pl, input, n, pitch_shift);
        consume_overrides(e);
        HIPCHK(hipMemcpyAsync(out, pl->d_f0, (size_t)pl->Tm * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        queue_status(e);
        HIPCHK(hipStreamSynchronize(e->stream));
        return final_status(e);
    });
}

// Streams whose formant shifts give different decoder lengths R2: one bucket per R2 (run_buckets), synchronous
static rvc_status infer_r2_buckets(rvc_engine *e, const void *input, bool input_on_device, size_t n, size_t frame16k, int32_t pitch_shift,
                                   uint32_t skip_head, uint32_t return_length, void *out, bool out_on_device, size_t cap, size_t *out_len, const int32_t *shifts)
{
    if (e->pipeline || e->use_graph) throw ShapeError("formant shift: streams with different decoder lengths in one call are not served with chunk pipelining / graph replay");
    const int S = e->n_streams;
    std::map<uint32_t, std::vector<int>> by;
    for (int s = 0; s < S; s++) { uint32_t r2; bool res; formant_geo(e, s, return_length, &r2, &res); by[r2].push_back(s); }
    if ((int)by.size() > e->plan_cap) throw ShapeError("formant shift: more different decoder lengths in one call than the plan cache holds (rvc_set_plan_cache)");
    ensure_bucket_state(e);
    std::vector<BucketRun> work;
    for (auto &kv : by) {
        Plan *pl = get_plan(e, plan_key(e, 0, n, frame16k, skip_head, return_length, &kv.second));
        if (out_len) *out_len = pl->N;
        if (cap < pl->N) return RVC_SHAPE;
        work.push_back({pl, kv.second});
    }
    std::vector<uint32_t> Rs((size_t)S, return_length);
    push_call_params(e, pitch_shift, shifts, Rs.data());
    return run_buckets(e, work, [&](int s) { return (const void *)((const float *)input + (size_t)s * n); }, input_on_device,
                       [&](int s) { return (void *)((float *)out + (size_t)s * cap); }, out_on_device);
}

static rvc_status infer_common(rvc_engine *e, const void *input, bool input_on_device, size_t n, size_t frame16k, int32_t pitch_shift,
                               uint32_t skip_head, uint32_t return_length, void *out, bool out_on_device, size_t cap, size_t *out_len, bool sync,
                               const int32_t *shifts = nullptr)
{
    if (!e->sy) return RVC_MODEL_NOT_LOADED;             // rvc.rs:141-143
    if (!e->cv) return RVC_CONTENTVEC_NOT_LOADED;        // rvc.rs:85-88 (via extract_feature at rvc.rs:151)
    if (!e->f0_method && e->sy->has_f0) return RVC_F0_NOT_LOADED;         // reference: unreachable!() at rvc.rs:125; a model without pitch guidance needs no tracker
    if (!e->sy->has_f0 && e->pipeline) throw ShapeError("chunk pipelining overlaps the two front branches of consecutive chunks: a model without pitch guidance has no such pair (rvc_set_pipeline(e, 0))");
    uint32_t r2 = 0; bool fstage = false;
    if (!formant_key(e, return_length, nullptr, &r2, &fstage))      // streams with different decoder lengths have no one plan: bucketed by R2
        return infer_r2_buckets(e, input, input_on_device, n, frame16k, pitch_shift, skip_head, return_length, out, out_on_device, cap, out_len, shifts);
    const bool pipe = e->pipeline && !sync && input_on_device && out_on_device && e->partitioned && !e->use_graph && !e->profile_on && !e->taps_on;
    PlanKey key = plan_key(e, 0, n, frame16k, skip_head, return_length);
    key.slot = pipe ? (e->pipe_slot ^= 1) : 0;
    Plan *pl = get_plan(e, key);
    if (out_len) *out_len = pl->N;
    if (cap < pl->N) return RVC_SHAPE;
    const int B = pl->key.B;
    override_fits(e, *pl);
    {
        std::vector<uint32_t> Rs((size_t)B, return_length);
        push_call_params(e, pitch_shift, shifts, Rs.data());
    }
    push_overrides(e, *pl, pipe);
    // Device-resident callers: the first kernels read the caller's buffer and the last one writes the caller's buffer (eager launches
    // take the pointers at launch time) -- no staging copy in front of the chunk, no copy behind it.  A captured graph bakes its
    // pointers and keeps both copies; pipelined calls keep the input copy (it decouples the caller's buffer from the chunk in flight).
    static const bool no_direct = tune_env("RVC_NO_DIRECT_IO") != nullptr;
    const bool direct_in = input_on_device && !pipe && !e->use_graph && pl->in_direct_ok && !no_direct;
    // (folded streams address the output with 32-bit offsets stream * cap: a caller-chosen cap beyond that range keeps the copy)
    const bool direct_out = out_on_device && !e->use_graph && pl->out_direct_ok && !no_direct && (long long)pl->key.B * (long long)cap < (1LL << 29);
    pl->cur_in = direct_in ? (const float *)input : nullptr;
    pl->cur_out = direct_out ? (float *)out : nullptr; pl->cur_out_bs = (long long)cap;
    if (pipe) {
        // chunk pipelining: the two front branches of this chunk start as soon as THEIR previous work and this plan slot's previous
        // chunk are done -- not after the previous chunk's synthesizer on the main stream
        hipStream_t cvs = e->aux[2], rms = e->aux[0];
        if (pl->ev_done_valid) { HIPCHK(hipStreamWaitEvent(cvs, pl->ev_done, 0)); HIPCHK(hipStreamWaitEvent(rms, pl->ev_done, 0)); }
        HIPCHK(hipMemcpyAsync(pl->d_in, input, (size_t)B * n * sizeof(float), hipMemcpyDeviceToDevice, cvs));
        HIPCHK(hipEventRecord(e->ev_in, cvs));
        HIPCHK(hipStreamWaitEvent(rms, e->ev_in, 0));
    } else if (!direct_in) {
        HIPCHK(hipMemcpyAsync(pl->d_in, input, (size_t)B * n * sizeof(float), input_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
    }
    e->pipe_now = pipe;
    run_plan(e, *pl);
    e->pipe_now = false;
    if (!e->conv_curve) consume_overrides(e);
    if (!direct_out)
        HIPCHK(hipMemcpy2DAsync(out, cap * sizeof(float), pl->audio.p, pl->N * sizeof(float), pl->N * sizeof(float), B,
                                out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream));
    if (!pl->ev_done) HIPCHK(hipEventCreateWithFlags(&pl->ev_done, hipEventDisableTiming));
    HIPCHK(hipEventRecord(pl->ev_done, e->stream));
    pl->ev_done_valid = true;
    e->last_knn_rows = pl->key.with_index ? return_length : 0;
    e->status_queued = true;        // the chunk's last kernel writes the status words into the host-mapped block (advance_chunk_kernel)
    if (!sync) return RVC_OK;
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipEventElapsedTime(&e->last_ms, e->ev0, e->ev1));
    rvc_status st = check_status(e);
    if (st == RVC_KNN_RETRY) {
        // degrade, don't fail: the chunk's retrieval through the exhaustive launches, the rest of the chunk again, the output copy again
        st = recover_retrieval(e, *pl);
        if (st != RVC_OK) return st;
        if (!direct_out)
            HIPCHK(hipMemcpy2DAsync(out, cap * sizeof(float), pl->audio.p, pl->N * sizeof(float), pl->N * sizeof(float), B,
                                    out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream));
        e->status_queued = true;
        HIPCHK(hipStreamSynchronize(e->stream));
        st = check_status(e);
        if (st == RVC_KNN_RETRY) st = RVC_BACKEND;
    }
    return st;
}

// rvc.rs:133-220
rvc_status rvc_infer(rvc_engine *e, const float *input, size_t n, size_t sample_frame_16k_size, int has_pitch_shift, int32_t pitch_shift,
                     uint32_t skip_head, uint32_t return_length, float *out, size_t cap, size_t *out_len)
{
    return guarded(e, [&]() {
        if (e->n_streams != 1) throw ShapeError("infer() is a single-stream call; use rvc_infer_batch");
        return infer_common(e, input, false, n, sample_frame_16k_size, has_pitch_shift ? pitch_shift : 0, skip_head, return_length, out, false, cap, out_len, true);
    });
}

rvc_status rvc_infer_batch(rvc_engine *e, const float *input, size_t n, size_t sample_frame_16k_size, int32_t pitch_shift, uint32_t skip_head,
                           uint32_t return_length, float *out, size_t cap_per_stream, size_t *out_len)
{
    return guarded(e, [&]() { return infer_common(e, input, false, n, sample_frame_16k_size, pitch_shift, skip_head, return_length, out, false, cap_per_stream, out_len, true); });
}

rvc_status rvc_infer_device(rvc_engine *e, const void *d_input, size_t n, size_t sample_frame_16k_size, int32_t pitch_shift, uint32_t skip_head,
                            uint32_t return_length, void *d_out, size_t cap_per_stream, size_t *out_len, int sync)
{
    return guarded(e, [&]() { return infer_common(e, d_input, true, n, sample_frame_16k_size, pitch_shift, skip_head, return_length, d_out, true, cap_per_stream, out_len, sync != 0); });
}

// many streams, every stream with its own pitch shift (each stream of a batch is a caller of its own: obs-rvc/src/lib.rs:701-707)
rvc_status rvc_infer_batch_v(rvc_engine *e, const float *input, size_t n, size_t sample_frame_16k_size, const int32_t *pitch_shift, uint32_t skip_head,
                             uint32_t return_length, float *out, size_t cap_per_stream, size_t *out_len)
{
    return guarded(e, [&]() {
        if (!pitch_shift) throw ShapeError("infer_batch_v: pitch_shift[n_streams] is required");
        return infer_common(e, input, false, n, sample_frame_16k_size, 0, skip_head, return_length, out, false, cap_per_stream, out_len, true, pitch_shift);
    });
}

rvc_status rvc_infer_device_v(rvc_engine *e, const void *d_input, size_t n, size_t sample_frame_16k_size, const int32_t *pitch_shift, uint32_t skip_head,
                              uint32_t return_length, void *d_out, size_t cap_per_stream, size_t *out_len, int sync)
{
    return guarded(e, [&]() {
        if (!pitch_shift) throw ShapeError("infer_device_v: pitch_shift[n_streams] is required");
        return infer_common(e, d_input, true, n, sample_frame_16k_size, 0, skip_head, return_length, d_out, true, cap_per_stream, out_len, sync != 0, pitch_shift);
    });
}

// Many streams, every stream with ITS OWN geometry.  In the reference every stream is a process of its own with its own chunk length,
// crossfade and extra context (obs-rvc/src/lib.rs:200-227, 694, 701-707); a server that batches such callers cannot ask them to agree on
// (n, sample_frame_16k_size, skip_head, return_length).  Streams with equal geometry form a bucket; every bucket runs as one batch through
// its own plan on a gathered copy of its streams' states (pitch cache, counters, status), which is scattered back afterwards.
rvc_status rvc_infer_batch_g(rvc_engine *e, const float *const *inputs, const size_t *n, const size_t *sample_frame_16k_size, const int32_t *pitch_shift,
                             const uint32_t *skip_head, const uint32_t *return_length, float *const *outs, const size_t *caps, size_t *out_lens)
{
    return guarded(e, [&]() {
        if (!inputs || !n || !sample_frame_16k_size || !skip_head || !return_length || !outs || !caps) throw ShapeError("infer_batch_g: null argument array");
        if (!e->sy) return RVC_MODEL_NOT_LOADED;
        if (!e->cv) return RVC_CONTENTVEC_NOT_LOADED;
        if (!e->f0_method && e->sy->has_f0) return RVC_F0_NOT_LOADED;
        const int S = e->n_streams;
        if (e->pipeline || e->use_graph) throw ShapeError("infer_batch_g: not with chunk pipelining / graph replay");
        // (R2, fstage: the formant decoder length of the stream and whether its bucket carries the formant stage, formant.hip.h)
        struct Key { size_t n, f; uint32_t sh, rl, r2; bool operator<(const Key &o) const { return std::tie(n, f, sh, rl, r2) < std::tie(o.n, o.f, o.sh, o.rl, o.r2); } };
        std::map<Key, std::vector<int>> buckets;
        for (int s = 0; s < S; s++) {
            if (!inputs[s] || !outs[s]) throw ShapeError("infer_batch_g: null stream buffer");
            uint32_t r2; bool res; formant_geo(e, s, return_length[s], &r2, &res);
            buckets[Key{n[s], sample_frame_16k_size[s], skip_head[s], return_length[s], r2}].push_back(s);
        }
        // every bucket's plan must stay cached until the call has run it: the cache is LRU and the call's plans are its most recent entries, so the
        // only way to lose one is more buckets than slots
        if ((int)buckets.size() > e->plan_cap) throw ShapeError("infer_batch_g: more different geometries in one call than the plan cache holds (rvc_set_plan_cache)");
        ensure_bucket_state(e);
        // plans first (a geometry the engine rejects must not leave some buckets already advanced), then the work
        std::vector<BucketRun> work;
        for (auto &kv : buckets) {
            Plan *pl = get_plan(e, plan_key(e, 0, kv.first.n, kv.first.f, kv.first.sh, kv.first.rl, &kv.second));
            for (int s : kv.second) { if (out_lens) out_lens[s] = pl->N; if (caps[s] < pl->N) return RVC_SHAPE; }
            work.push_back({pl, kv.second});
        }
        push_call_params(e, 0, pitch_shift, return_length);      // per-stream multipliers into the streams' own states (a null array: no shift)
        return run_buckets(e, work, [&](int s) { return (const void *)inputs[s]; }, false, [&](int s) { return (void *)outs[s]; }, false);
    });
}

rvc_status rvc_synchronize(rvc_engine *e)
{
    return guarded(e, [&]() {
        HIPCHK(hipStreamSynchronize(e->stream));
        if (e->ev0 && e->last_plan) (void)hipEventElapsedTime(&e->last_ms, e->ev0, e->ev1);
        return final_status(e);
    });
}

rvc_status rvc_set_streams(rvc_engine *e, int n_streams)
{
    return guarded(e, [&]() {
        if (n_streams < 1 || n_streams > 4096) throw ShapeError("n_streams out of range");
        HIPCHK(hipDeviceSynchronize());
        e->n_streams = n_streams;
        alloc_state(e);
        configure_aux_streams(e);
        return RVC_OK;
    });
}

void rvc_set_use_graph(rvc_engine *e, int on) { if (e) e->use_graph = on != 0; }

// EXPLORATORY, off by default and never part of the headline figure: mode 1 runs the 1-D layers with >= 128 output rows (ContentVec's projections and convolution stem, the decoder's
// 128- / 256-channel stages) as three bf16 MFMAs per fp32 product (a_hi b_hi + a_hi b_lo + a_lo b_hi, fp32 accumulation; igemm_bf3_kernel) wherever a launch has >= 250 workgroups of 128 x 128
// (at 64 streams 2.5 of the 3.6 TFLOP of a step).  gfx950's fp32 MFMA runs at 1/16 of its bf16 rate and there is no xf32.  Results differ from the fp32 path by ~2^-16 relative
// per product (tests/test_gpu_round5.py measures it against the oracle); mode 0 is the reference's arithmetic.
rvc_status rvc_set_gemm_precision(rvc_engine *e, int mode)
{
    return guarded(e, [&]() {
        if (mode != 0 && mode != 1) throw ShapeError("gemm precision: 0 (fp32) or 1 (split bf16, exploratory)");
        e->gemm_precision = mode;
        return RVC_OK;
    });
}

// Plan cache: one plan (activation arena, composed weights, launch list) per geometry (mode, n, frame, skip_head, return_length, streams,
// retrieval on/off, pipeline slot).  Every plugin instance has its own geometry (obs-rvc/src/lib.rs:200-227): a server that serves more
// geometries than the cache holds rebuilds a plan on every miss.
// Plan-time selection by measurement (plan.hip, queue_igemm): on = 1 (default) lets plans of more than 4 streams time the eligible kernels / tiles of every
// layer on this device while the plan is built and keep the fastest; on = 0: the planner's rules only.  Cached plans are dropped when the setting changes.
rvc_status rvc_set_plan_autotune(rvc_engine *e, int on)
{
    return guarded(e, [&]() {
        const int v = on ? 1 : 0;
        if (v != e->autotune) {
            drop_plans(e);
            e->autotune = v;
        }
        return RVC_OK;
    });
}
// the engine's LAST plan build: layers tuned by trials in it, layers whose choice differs from the rules, layers taken from the process-wide cache of earlier
// trials, milliseconds spent in trials, milliseconds of the whole build
rvc_status rvc_plan_autotune_info(rvc_engine *e, int *tuned, int *changed, int *cache_hits, double *tune_ms, double *build_ms)
{
    return guarded(e, [&]() {
        if (tuned) *tuned = e->last_tuned;
        if (changed) *changed = e->last_changed;
        if (cache_hits) *cache_hits = e->last_hits;
        if (tune_ms) *tune_ms = e->last_tune_ms;
        if (build_ms) *build_ms = e->last_build_ms;
        return RVC_OK;
    });
}

rvc_status rvc_set_plan_cache(rvc_engine *e, int n_plans)
{
    return guarded(e, [&]() {
        if (n_plans < 2 || n_plans > 256) throw ShapeError("plan cache size out of range (2..256)");
        HIPCHK(hipDeviceSynchronize());
        e->plan_cap = n_plans;
        evict_lru(e, (size_t)e->plan_cap);
        return RVC_OK;
    });
}
int rvc_plan_cache_info(rvc_engine *e, int *capacity, int *cached, long long *builds)
{
    if (!e) return 0;
    if (capacity) *capacity = e->plan_cap;
    if (cached) *cached = (int)e->plans.size();
    if (builds) *builds = e->plan_builds;
    return 1;
}
void rvc_set_pipeline(rvc_engine *e, int on)
{
    if (!e) return;
    (void)guarded(e, [&]() { HIPCHK(hipDeviceSynchronize()); e->pipeline = on != 0; e->pushed_valid = false; return RVC_OK; });
}
void rvc_set_profile(rvc_engine *e, int on) { if (e) e->profile_on = on != 0; }
void rvc_enable_taps(rvc_engine *e, int on) { if (e) e->taps_on = on == 2 ? 2 : (on != 0 ? 1 : 0); }
float rvc_last_gpu_ms(rvc_engine *e) { return e ? e->last_ms : 0.f; }
void rvc_set_index_rate(rvc_engine *e, float rate) { if (e) e->index_rate = rate; }

void rvc_set_noise_seed(rvc_engine *e, uint32_t seed, uint32_t stream_id)
{
    if (!e) return;
    (void)guarded(e, [&]() {
        HIPCHK(hipDeviceSynchronize());
        e->seed = seed; e->stream_id0 = stream_id;
        // keep pitch caches / chunk counters, only re-stamp the stream ids
        std::vector<StreamState> st(e->n_streams);
        HIPCHK(hipMemcpy(st.data(), e->d_state, sizeof(StreamState) * e->n_streams, hipMemcpyDeviceToHost));
        for (int b = 0; b < e->n_streams; b++) st[b].stream_id = stream_id + (uint32_t)b;
        HIPCHK(hipMemcpy(e->d_state, st.data(), sizeof(StreamState) * e->n_streams, hipMemcpyHostToDevice));
        return RVC_OK;
    });
}

void rvc_reset_state(rvc_engine *e)
{
    if (!e) return;
    (void)guarded(e, [&]() { HIPCHK(hipDeviceSynchronize()); reset_state(e); return RVC_OK; });
}

void rvc_get_pitch_cache(rvc_engine *e, int stream, float *out1024)
{
    if (!e || stream < 0 || stream >= e->n_streams) return;
    (void)guarded(e, [&]() {
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(out1024, e->d_state[stream].cache_pitchf, 1024 * sizeof(float), hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

// The per-stream settings (rvc_engine::StreamSettings): formant shift (the plugin's resonance shift, obs-rvc/src/lib.rs:80,103,176,369-375,446-451; formant.hip.h;
// semitones in [-5, 5]), the pitch controls (f0cond.hip.h; DESIGN.md "Pitch controls") and consonant protection (protect.hip.h; DESIGN.md "Consonant protection";
// [0, 0.5], 0.5 = off).  stream == nullptr: the engine-wide call, which sets every stream and the default of streams rvc_set_streams adds later; rvc_reset_state
// leaves the values alone.  bad: what is wrong with the value (nullptr = nothing), reported behind a stream out of range.  The next call pushes what changed.
using StreamSettings = rvc_engine::StreamSettings;
static rvc_status set_stream_setting(rvc_engine *e, const int *stream, const char *what, const char *bad, const std::function<void(StreamSettings &)> &set)
{
    return guarded(e, [&]() {
        if (stream && (*stream < 0 || *stream >= e->n_streams)) throw ShapeError(std::string(what) + ": stream out of range");
        if (bad) throw ShapeError(std::string(what) + ": " + bad);
        if (stream) set(e->settings[*stream]);
        else { set(e->settings_default); for (auto &c : e->settings) set(c); }
        return RVC_OK;
    });
}
static rvc_status set_formant(rvc_engine *e, const int *stream, double st)
{
    return set_stream_setting(e, stream, "formant shift", st >= -FORMANT_MAX && st <= FORMANT_MAX ? nullptr : "semitones outside [-5, 5]", [&](StreamSettings &c) { c.formant = st; });
}
static rvc_status set_pitch_semitones(rvc_engine *e, const int *stream, double st)
{
    return set_stream_setting(e, stream, "pitch semitones", st >= -PITCH_SEMITONES_MAX && st <= PITCH_SEMITONES_MAX ? nullptr : "semitones outside [-24, 24]",
                              [&](StreamSettings &c) { c.pitch.semitones = st; });
}
static rvc_status set_f0_range(rvc_engine *e, const int *stream, double lo, double hi)
{
    return set_stream_setting(e, stream, "f0 range", lo >= 0.0 && hi >= lo ? nullptr : "needs 0 <= lo_hz <= hi_hz", [&](StreamSettings &c) { c.pitch.lo = (float)lo; c.pitch.hi = (float)hi; });
}
static rvc_status set_f0_median(rvc_engine *e, const int *stream, int radius)
{
    return set_stream_setting(e, stream, "f0 median", radius >= 0 && radius <= F0_MEDIAN_MAX ? nullptr : "radius outside 0..7", [&](StreamSettings &c) { c.pitch.radius = radius; });
}
static rvc_status set_f0_snap(rvc_engine *e, const int *stream, uint32_t mask, double strength)
{
    return set_stream_setting(e, stream, "f0 snap", mask > 0xFFFu ? "pitch-class mask has bits above bit 11" : (strength >= 0.0 && strength <= 1.0 ? nullptr : "strength outside [0, 1]"),
                              [&](StreamSettings &c) { c.pitch.mask = mask; c.pitch.strength = (float)strength; });
}
static rvc_status set_protect(rvc_engine *e, const int *stream, double protect)
{
    return set_stream_setting(e, stream, "protect", protect >= 0.0 && protect <= PROTECT_OFF ? nullptr : "value outside [0, 0.5]", [&](StreamSettings &c) { c.protect = protect; });
}
rvc_status rvc_set_formant_shift(rvc_engine *e, double semitones) { return set_formant(e, nullptr, semitones); }
rvc_status rvc_set_formant_shift_stream(rvc_engine *e, int stream, double semitones) { return set_formant(e, &stream, semitones); }
rvc_status rvc_set_pitch_semitones(rvc_engine *e, double semitones) { return set_pitch_semitones(e, nullptr, semitones); }
rvc_status rvc_set_pitch_semitones_stream(rvc_engine *e, int stream, double semitones) { return set_pitch_semitones(e, &stream, semitones); }
rvc_status rvc_set_f0_range(rvc_engine *e, double lo_hz, double hi_hz) { return set_f0_range(e, nullptr, lo_hz, hi_hz); }
rvc_status rvc_set_f0_range_stream(rvc_engine *e, int stream, double lo_hz, double hi_hz) { return set_f0_range(e, &stream, lo_hz, hi_hz); }
rvc_status rvc_set_f0_median(rvc_engine *e, int radius) { return set_f0_median(e, nullptr, radius); }
rvc_status rvc_set_f0_median_stream(rvc_engine *e, int stream, int radius) { return set_f0_median(e, &stream, radius); }
rvc_status rvc_set_f0_snap(rvc_engine *e, uint32_t pitch_class_mask, double strength) { return set_f0_snap(e, nullptr, pitch_class_mask, strength); }
rvc_status rvc_set_f0_snap_stream(rvc_engine *e, int stream, uint32_t pitch_class_mask, double strength) { return set_f0_snap(e, &stream, pitch_class_mask, strength); }
rvc_status rvc_set_protect(rvc_engine *e, double protect) { return set_protect(e, nullptr, protect); }
rvc_status rvc_set_protect_stream(rvc_engine *e, int stream, double protect) { return set_protect(e, &stream, protect); }

// f0 from outside.  A set call only records: the rows travel in front of the next chunk of a plan that has the select (push_overrides)
static const char *f0_value_bad(float v, bool nan_ok)
{
    if (v != v) return nan_ok ? nullptr : "a curve value is NaN";
    return v >= 0.f && v <= F0_OV_MAX_HZ ? nullptr : "a value is negative, infinite or above 20000 Hz";
}
rvc_status rvc_set_f0_override_stream(rvc_engine *e, int stream, const float *hz, size_t n)
{
    return guarded(e, [&]() {
        if (stream < 0 || (size_t)stream >= e->ov.size()) throw ShapeError("f0 override: stream out of range");
        if (!hz) n = 0;
        if (n > (size_t)F0_OV_ROWS) throw ShapeError("f0 override: more than 1024 rows");
        for (size_t i = 0; i < n; i++) if (const char *bad = f0_value_bad(hz[i], true)) throw ShapeError(std::string("f0 override: ") + bad);
        if (n == 0 && e->ov[stream].empty()) return RVC_OK;
        e->ov[stream].assign(hz, hz + n);
        e->ov_dirty = true;
        return RVC_OK;
    });
}
rvc_status rvc_set_f0_override_hold(rvc_engine *e, int hold)
{
    return guarded(e, [&]() {
        if (hold != 0 && hold != 1) throw ShapeError("f0 override hold: 0 or 1");
        e->ov_hold = hold != 0;
        return RVC_OK;
    });
}
rvc_status rvc_set_f0_curve(rvc_engine *e, const double *t_sec, const float *hz, size_t n)
{
    return guarded(e, [&]() {
        if (n == 0) { e->curve_t.reset(); e->curve_hz.reset(); e->curve_n = 0; return RVC_OK; }
        if (!t_sec || !hz) throw ShapeError("f0 curve: null array");
        if (n > (size_t)1 << 24) throw ShapeError("f0 curve: more than 2^24 breakpoints");
        for (size_t i = 0; i < n; i++) {
            if (!std::isfinite(t_sec[i])) throw ShapeError("f0 curve: a time is not finite");
            if (i && !(t_sec[i] > t_sec[i - 1])) throw ShapeError("f0 curve: times must be strictly increasing");
            if (const char *bad = f0_value_bad(hz[i], false)) throw ShapeError(std::string("f0 curve: ") + bad);
        }
        DevBuf<double> dt; DevBuf<float> dh;
        dt.alloc(n); dh.alloc(n);
        HIPCHK(hipMemcpy(dt.get(), t_sec, n * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dh.get(), hz, n * sizeof(float), hipMemcpyHostToDevice));
        e->curve_t = std::move(dt); e->curve_hz = std::move(dh); e->curve_n = n;
        return RVC_OK;
    });
}
rvc_status rvc_f0_curve_grid(rvc_engine *e, size_t n_frames, float *out, size_t cap)
{
    return guarded(e, [&]() {
        if (n_frames < 1 || n_frames > (size_t)1 << 30) throw ShapeError("f0 curve grid: frame count out of range");
        if (!out || cap < n_frames) throw ShapeError("f0 curve grid: output buffer too small");
        DevBuf<float> g; g.alloc(n_frames);
        launch_f0_curve_grid(e->stream, e->curve_t.get(), e->curve_hz.get(), (int)e->curve_n, g.get(), (long long)n_frames);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, g.get(), n_frames * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return RVC_OK;
    });
}
rvc_status rvc_convert_f0(rvc_engine *e, float *hz, size_t cap, size_t *n_frames)
{
    return guarded(e, [&]() {
        if (!e->conv_f0_valid) throw ShapeError("convert_f0: no conversion with a pitch branch has completed on this engine");
        if (n_frames) *n_frames = e->conv_f0.size();
        if (!hz || cap < e->conv_f0.size()) throw ShapeError("convert_f0: output buffer too small");
        std::copy(e->conv_f0.begin(), e->conv_f0.end(), hz);
        return RVC_OK;
    });
}

rvc_status rvc_formant_geometry(size_t return_length, size_t sample_rate, double semitones, size_t out[2])
{
    if (!out) return RVC_SHAPE;
    size_t R2 = 0, ur = 0;
    if (!formant_geometry(return_length, sample_rate, semitones, &R2, &ur)) return RVC_SHAPE;
    out[0] = R2; out[1] = ur;
    return RVC_OK;
}
// the full filter table h[n][K] of the resampler o -> n (host only): 0, -1 on bad arguments, 1 when cap < n K (*width is written)
int rvc_debug_formant_table(size_t o, size_t n, float *out, size_t cap, size_t *width)
{
    if (o < 1 || n < 1 || o > 100000 || n > 100000) return -1;
    std::vector<float> h; size_t w, K;
    formant_table(o, n, h, &w, &K);
    if (width) *width = K;
    if (!out || cap < h.size()) return 1;
    memcpy(out, h.data(), h.size() * sizeof(float));
    return 0;
}

rvc_status rvc_profile_last(rvc_engine *e, int *launches, double *kernel_ms, double *flops)
{
    return guarded(e, [&]() {
        Plan *pl = e->last_plan;
        if (!pl) return RVC_SHAPE;
        HIPCHK(hipDeviceSynchronize());
        double ms = 0, fl = 0;
        int nl = 0;
        for (size_t i = 0; i < pl->prof_used; i++) { if (pl->prof[i].retrieval) continue; float t; HIPCHK(hipEventElapsedTime(&t, pl->prof[i].a, pl->prof[i].b)); ms += t; fl += pl->prof[i].flops; nl++; }
        if (launches) *launches = nl;
        if (kernel_ms) *kernel_ms = ms;
        if (flops) *flops = pl->prof_used ? fl : pl->igemm_flops;
        return RVC_OK;
    });
}

rvc_status rvc_envelop_mixing(rvc_engine *e, const float *input, float *output, size_t output_len, size_t sample_rate, double mix_rate)
{
    return guarded(e, [&]() {
        const size_t zc = sample_rate / 100;
        if (zc == 0 || output_len < zc) throw ShapeError("envelop_mixing: output shorter than one 10 ms hop");
        const int n = (int)output_len, frame = (int)(4 * zc), hop = (int)zc;
        const int nf = (n + 2 * (frame / 2) - frame) / hop + 1;
        float *d_in, *d_out; double *d_r;
        HIPCHK(hipMalloc(&d_in, output_len * 4)); HIPCHK(hipMalloc(&d_out, output_len * 4)); HIPCHK(hipMalloc(&d_r, (size_t)2 * nf * 8));
        HIPCHK(hipMemcpyAsync(d_in, input, output_len * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(d_out, output, output_len * 4, hipMemcpyHostToDevice, e->stream));
        launch_post_rms(e->stream, 1, d_in, n, frame, hop, nf, d_r, 0LL, 0LL);
        launch_post_rms(e->stream, 1, d_out, n, frame, hop, nf, d_r + nf, 0LL, 0LL);
        launch_post_mix(e->stream, 1, d_out, n, d_r, nf, d_r + nf, nf, (float)(1.0 - mix_rate), 0LL, 0LL, nullptr);
        HIPCHK(hipMemcpyAsync(output, d_out, output_len * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_r);
        return RVC_OK;
    });
}

// rvc_sola_step / rvc_sola_step_x: one SOLA step of one stream on host buffers.  crossfade = RVC_CROSSFADE_PHASE_VOCODER queues the analysis and the
// synthesis (crossfade.hip.h) behind the offset search, which keeps the segment unblended for them; sola_len < 2 has no seam to analyse (linear blend)
static rvc_status sola_step_host(rvc_engine *e, float *output, size_t output_len, float *sola_buffer, size_t sola_len, size_t search,
                                 size_t frame, float *frame_out, size_t *sola_offset, int crossfade)
{
    return guarded(e, [&]() {
        if (crossfade != RVC_CROSSFADE_LINEAR && crossfade != RVC_CROSSFADE_PHASE_VOCODER) throw ShapeError("sola: unknown crossfade mode");
        if (search + 1 > 1024) throw ShapeError("sola search range too long");
        if (output_len < sola_len + search || output_len < search + frame + sola_len) throw PanicError("sola: output shorter than offset + frame + tail (the reference slices out of range)");
        const bool pv = crossfade == RVC_CROSSFADE_PHASE_VOCODER && sola_len >= 2;
        if (pv && sola_len > (size_t)PV_MAX_N) throw ShapeError("sola: the phase-vocoder crossfade takes a seam of at most 4096 samples");
        float *d_out, *d_sola, *d_frame, *d_cor; int *d_off;
        HIPCHK(hipMalloc(&d_out, output_len * 4)); HIPCHK(hipMalloc(&d_sola, sola_len * 4)); HIPCHK(hipMalloc(&d_frame, frame * 4)); HIPCHK(hipMalloc(&d_off, 4));
        HIPCHK(hipMalloc(&d_cor, (search + 1) * 4));
        float *d_pva = nullptr, *d_tab = nullptr, *d_spec = nullptr;
        const int n = (int)sola_len, K = n / 2 + 1;
        if (pv) {
            std::vector<float> tab; pv_tables(n, tab);
            HIPCHK(hipMalloc(&d_pva, sola_len * 4)); HIPCHK(hipMalloc(&d_tab, tab.size() * 4)); HIPCHK(hipMalloc(&d_spec, (size_t)3 * K * 4));
            HIPCHK(hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        }
        HIPCHK(hipMemcpyAsync(d_out, output, output_len * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(d_sola, sola_buffer, sola_len * 4, hipMemcpyHostToDevice, e->stream));
        launch_post_sola_corr(e->stream, 1, d_out, d_sola, (int)sola_len, (int)search, d_cor, 0LL, 0LL, 0LL);
        launch_post_sola(e->stream, 1, d_out, d_sola, (int)sola_len, (int)search, (int)frame, d_frame, d_off, d_cor, 0LL, 0LL, 0LL, 0LL, nullptr, pv ? 1 : 0, d_pva, 0LL);
        if (pv) {
            hipLaunchKernelGGL(pv_analysis_kernel, dim3((K + PV_AT - 1) / PV_AT, 1), dim3(PV_AT), pv_analysis_lds(n), e->stream, d_out, d_pva, d_off, (const int *)nullptr, 1,
                               d_tab, n, d_spec, 0LL, 0LL);
            hipLaunchKernelGGL(pv_synth_kernel, dim3((n + PV_JT - 1) / PV_JT, 1), dim3(PV_JT * PV_KS), pv_synth_lds(n), e->stream, d_out, d_pva, d_sola, d_frame, d_off,
                               (const int *)nullptr, 1, d_tab, d_spec, n, (int)frame, 0LL, 0LL, 0LL, 0LL);
        }
        int off = 0;
        HIPCHK(hipMemcpyAsync(output, d_out, output_len * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(sola_buffer, d_sola, sola_len * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(frame_out, d_frame, frame * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(&off, d_off, 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipGetLastError());
        if (sola_offset) *sola_offset = (size_t)off;
        (void)hipFree(d_out); (void)hipFree(d_sola); (void)hipFree(d_frame); (void)hipFree(d_off); (void)hipFree(d_cor);
        (void)hipFree(d_pva); (void)hipFree(d_tab); (void)hipFree(d_spec);
        return RVC_OK;
    });
}
rvc_status rvc_sola_step(rvc_engine *e, float *output, size_t output_len, float *sola_buffer, size_t sola_len, size_t search,
                         size_t frame, float *frame_out, size_t *sola_offset)
{
    return sola_step_host(e, output, output_len, sola_buffer, sola_len, search, frame, frame_out, sola_offset, RVC_CROSSFADE_LINEAR);
}
rvc_status rvc_sola_step_x(rvc_engine *e, float *output, size_t output_len, float *sola_buffer, size_t sola_len, size_t search,
                           size_t frame, float *frame_out, size_t *sola_offset, int crossfade)
{
    return sola_step_host(e, output, output_len, sola_buffer, sola_len, search, frame, frame_out, sola_offset, crossfade);
}

// the session's input gate on host buffers: hist3zc (3 zc samples before the chunk, ungated), chunk (n = a multiple of zc) -> out (n), hist_out (3 zc)
rvc_status rvc_input_gate(rvc_engine *e, const float *hist3zc, const float *chunk, size_t n, size_t sample_rate, double threshold_db, float *out, float *hist_out)
{
    return guarded(e, [&]() {
        const size_t zc = sample_rate / 100;
        if (zc == 0 || sample_rate > 384000 || n < zc || n % zc != 0 || n > (size_t)1 << 30) throw ShapeError("input_gate: the chunk must be a whole number of 10 ms blocks");
        if (threshold_db != threshold_db) throw ShapeError("input_gate: the threshold is not a number");
        if (!hist3zc || !chunk || !out || !hist_out) throw ShapeError("input_gate: null buffer");
        float *d_chunk, *d_out, *d_hist;
        HIPCHK(hipMalloc(&d_chunk, n * 4)); HIPCHK(hipMalloc(&d_out, n * 4)); HIPCHK(hipMalloc(&d_hist, 6 * zc * 4));
        HIPCHK(hipMemcpyAsync(d_chunk, chunk, n * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(d_hist, hist3zc, 3 * zc * 4, hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(input_gate_kernel, dim3((unsigned)(n / zc + 1), 1), dim3(256), 0, e->stream, d_chunk, d_out, d_hist, d_hist + 3 * zc, (const float *)nullptr,
                           gate_threshold(threshold_db), (int)zc, (int)n, 0LL, 0LL);
        HIPCHK(hipMemcpyAsync(out, d_out, n * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(hist_out, d_hist + 3 * zc, 3 * zc * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipGetLastError());
        (void)hipFree(d_chunk); (void)hipFree(d_out); (void)hipFree(d_hist);
        return RVC_OK;
    });
}

rvc_status rvc_profile_last_knn(rvc_engine *e, int *launches, double *kernel_ms, double *bytes)
{
    return guarded(e, [&]() {
        Plan *pl = e->last_plan;
        if (!pl) return RVC_SHAPE;
        HIPCHK(hipDeviceSynchronize());
        double ms = 0, by = 0; int nl = 0;
        for (size_t i = 0; i < pl->prof_used; i++) { if (!pl->prof[i].retrieval) continue; float t; HIPCHK(hipEventElapsedTime(&t, pl->prof[i].a, pl->prof[i].b)); ms += t; by += pl->prof[i].bytes; nl++; }
        if (nl && pl->d_ivf_scanned) {       // IVF retrieval: the centroid table (the coarse launch's slot) plus the rows the last run's probe sets held
            std::vector<int> rows(pl->ivf_queries);
            HIPCHK(hipMemcpy(rows.data(), pl->d_ivf_scanned, rows.size() * sizeof(int), hipMemcpyDeviceToHost));
            for (int r : rows) by += (double)r * e->index.dim * sizeof(float);
        }
        if (launches) *launches = nl;
        if (kernel_ms) *kernel_ms = ms;
        if (bytes) *bytes = by;
        return RVC_OK;
    });
}

// the named tap of one stream of the last call's plan (snapshots and RMVPE images hold every stream of the plan, stream-major)
static rvc_status read_tap(rvc_engine *e, const char *name, int stream, float *out, size_t cap, size_t *n)
{
    return guarded(e, [&]() {
        Plan *pl = e->last_plan;
        if (!pl || !name) return RVC_SHAPE;
        if (stream < 0 || stream >= pl->key.B) { e->err = "tap: the last call's plan has no such stream"; return RVC_SHAPE; }
        HIPCHK(hipDeviceSynchronize());
        for (auto &t : pl->taps) {
            if (t.name != name) continue;
            if (t.rank == 1) {
                if (stream >= t.t1.B) { e->err = std::string("tap ") + name + " is one tensor for the whole plan: stream 0 holds it"; return RVC_SHAPE; }
                size_t need = (size_t)t.t1.C * t.t1.T; if (n) *n = need;
                if (cap < need) return RVC_SHAPE;
                HIPCHK(hipMemcpy2D(out, (size_t)t.t1.T * 4, t.t1.p + (long long)stream * t.t1.bs, (size_t)t.t1.ld * 4, (size_t)t.t1.T * 4, t.t1.C, hipMemcpyDeviceToHost));
            } else {
                if (stream >= t.t2.B) return RVC_SHAPE;
                size_t need = (size_t)t.t2.C * t.t2.H * t.t2.W; if (n) *n = need;
                if (cap < need) return RVC_SHAPE;
                const float *src = t.t2.p + (long long)stream * t.t2.bs;
                for (int c = 0; c < t.t2.C; c++)
                    HIPCHK(hipMemcpy2D(out + (size_t)c * t.t2.H * t.t2.W, (size_t)t.t2.W * 4, src + (size_t)c * t.t2.cs, (size_t)t.t2.ld * 4, (size_t)t.t2.W * 4, t.t2.H, hipMemcpyDeviceToHost));
            }
            return RVC_OK;
        }
        if (!strcmp(name, "f0") && pl->d_f0) {
            if (n) *n = (size_t)pl->Tm;
            if (cap < (size_t)pl->Tm) return RVC_SHAPE;
            HIPCHK(hipMemcpy(out, pl->d_f0 + (size_t)stream * pl->Tm, (size_t)pl->Tm * 4, hipMemcpyDeviceToHost));
            return RVC_OK;
        }
        e->err = std::string("unknown tap ") + name;
        return RVC_SHAPE;
    });
}

rvc_status rvc_get_tap(rvc_engine *e, const char *name, float *out, size_t cap, size_t *n) { return read_tap(e, name, 0, out, cap, n); }

// test hook (include/rvc_mi355x_debug.h): the named tap of stream `stream` of the last call; RVC_SHAPE for a stream the plan did not have
int rvc_debug_tap(rvc_engine *e, const char *name, int stream, float *out, size_t cap, size_t *n) { return (int)read_tap(e, name, stream, out, cap, n); }

}  // extern "C"

#include "resample.hip.h"
#include "denoise.hip.h"
#include "session.hip.h"
#include "rccl_bcast.hip.h"
#include "convert_many.hip.h"

namespace rvc {

// the session's ring launches (session.hip.h) and one converter call (resample.hip.h) for rvc_session_process and rvc_debug_post (debug.hip)
void launch_ring_shift_append(hipStream_t s, int B, const float *in, float *out, int n, int f, const float *chunk)
{
    hipLaunchKernelGGL(ring_shift_append_kernel, dim3((n + 255) / 256, B), dim3(256), 0, s, in, out, n, f, chunk);
}
void launch_ring16_update(hipStream_t s, int B, const float *in, float *out, int n, int f, const float *res, int skip, int copy_begin, long long res_bs)
{
    hipLaunchKernelGGL(ring16_update_kernel, dim3((n + 255) / 256, B), dim3(256), 0, s, in, out, n, f, res, skip, copy_begin, res_bs);
}
rvc_status resampler_create_streams(rvc_engine *e, size_t rate_in, size_t rate_out, size_t chunk_size_in, int nb, rvc_resampler **out, int *fft_in, int *fft_out)
{
    const rvc_status rc = resampler_create_n(e, rate_in, rate_out, chunk_size_in, nb, out);
    if (rc == RVC_OK) { *fft_in = (*out)->fft_in; *fft_out = (*out)->fft_out; }
    return rc;
}
void launch_resampler(rvc_resampler *r, const float *d_in, float *d_out, long long in_bs, long long out_bs) { resampler_launch(r, d_in, d_out, in_bs, out_bs); }

}  // namespace rvc
