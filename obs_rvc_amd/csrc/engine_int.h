// engine_int.h -- internal declarations shared by the translation units of librvc_mi355x.so:
//   plan.hip         the planner: device memory, prepared convolution weights, the op list, implicit-GEMM tile selection, test-hook table
//   model_cv.hip     ContentVec (build_contentvec)          model_rmvpe.hip   RMVPE + decode (build_rmvpe, build_pitch_post)
//   model_yin.hip    YIN f0 (build_yin)                      model_crepe.hip   CREPE f0 (build_crepe, the decoder's launch)
//   model_fcpe.hip   FCPE f0 (build_fcpe, the decoder's and the depthwise kernel's launches)     f0_pm.hip   "pm" f0 (build_pm and its launches)     (hybrid f0: engine.hip build_f0 queues the members, model_rmvpe.hip the combine)
//   model_synth.hip  the synthesizer (build_synth, ...)      retrieval.hip     flat-L2 index: install_index, device-side layouts (RetrievalIndex), the plan's search section
//   engine.hip       the engine object, plans, the C ABI (+ session.hip.h, resample.hip.h, rccl_bcast.hip.h, convert.hip.h: the file converter, with
//                    resample_whole.hip.h, change_rms.hip.h and f0_analyze.hip.h: f0 analysis, order statistics, auto-transpose)
//   debug.hip        the test and tuning aids of include/rvc_mi355x_debug.h that build plans of their own (rvc_debug_layer / _op / _front, the *_check aids)
// The model structs (weights as prepared at load) are defined here; their loaders are in the model's unit.  Kernels: a non-template __global__ function is
// compiled into the device code of every unit that includes its definition, launched or not, so each lives in a header that exactly one unit includes
// (plan_ops.hip.h, contentvec.hip.h, rmvpe.hip.h, rmblock.hip.h, f0_hybrid.hip.h, yin.hip.h, pm.hip.h, crepe.hip.h, fcpe.hip.h, synth.hip.h, knn.hip.h, chunk.hip.h, protect.hip.h, f0_override.hip.h, f0_select.hip.h, crossfade.hip.h, stitch.hip.h, ...)
// or in that unit's .hip file, and no header included from here defines one.  The implicit-GEMM templates (igemm2 / igemm2w / igemm_lds / igemm32 / igemm_bf3 / igemm_splitk .hip.h) are instantiated by the
// *_inst.hip units.
#pragma once
#include "../../include/rvc_mi355x.h"
#include "blob.h"
#include "state.hip.h"
#include "formant.hip.h"
#include "f0cond.hip.h"
#include "f0_override.h"
#include "igemm_launch.h"
#include "dev_raii.h"
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>
#include <thread>

namespace rvc {

// ---------------------------------------------------------------------------------------
// switches
// ---------------------------------------------------------------------------------------
// The product library reads four environment variables and no others: GPU_MAX_HW_QUEUES (a default is planted, see above),
// RVC_NO_RUNTIME_DEFAULTS, LOCAL_RANK (rvc_create with device < 0) and RVC_RCCL_LIB (rccl_bcast.hip.h); the rvc-rpc executable adds
// RVC_NOISE_SEED and RVC_USE_GRAPH.  Every other switch is
//   * a TEST HOOK (kTestHooks): set with rvc_debug_option(name, value) by the parity tests and the profiling tools -- an explicit call,
//     never inherited from a host's environment -- to force a code path the planner would not pick for the geometry at hand; or
//   * a TUNING switch (tune_env): compiled out of the product (the call is a constant nullptr, its branch disappears); only builds with
//     -DRVC_TUNING (tests/tools/build_tuning.py -> librvc_tuning.so) have them, and there both kinds also fall back to the environment
//     variable of the same name.
const char *test_opt(const char *name);
extern std::atomic<unsigned> g_opt_gen;      // generation of the test-hook table (plan.hip)
extern std::atomic<int> g_knn_test_lose;     // RVC_KNN_LOSE_TICKET (retrieval.hip)
int test_opt_int(const char *name, int dflt);
#ifdef RVC_TUNING
const char *tune_env(const char *name);
#else
static inline const char *tune_env(const char *) { return nullptr; }
#endif

struct ShapeError : std::runtime_error { using std::runtime_error::runtime_error; };
struct PanicError : std::runtime_error { using std::runtime_error::runtime_error; };

// ---------------------------------------------------------------------------------------
// device memory
// ---------------------------------------------------------------------------------------
class Arena {
public:
    ~Arena() { for (void *c : chunks_) (void)hipFree(c); }
    void *alloc(size_t bytes)
    {
        bytes = (bytes + 255) / 256 * 256;
        if (bytes > left_) {
            size_t sz = std::max(bytes, chunk_min_);
            void *c;
            HIPCHK(hipMalloc(&c, sz));
            HIPCHK(hipMemset(c, 0, sz));
            if (chunks_.empty()) first_size_ = sz;
            chunks_.push_back(c);
            cur_ = (char *)c;
            left_ = sz;
            total_ += sz;
        }
        void *r = cur_;
        cur_ += bytes;
        left_ -= bytes;
        return r;
    }
    float *floats(size_t n) { return (float *)alloc(n * sizeof(float)); }
    template <typename T> T *upload(const std::vector<T> &v)
    {
        T *d = (T *)alloc(std::max<size_t>(v.size(), 1) * sizeof(T));
        if (!v.empty()) HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    size_t total() const { return total_; }
    void set_chunk_min(size_t b) { chunk_min_ = b; }          // (trial plans of the autotuner hold one layer's tables: small chunks)
    // start over in the first chunk, keeping the memory (the autotuner's scratch plan: hundreds of trials per plan build, no hipMalloc / hipFree per trial);
    // later chunks are returned.  The memory is NOT zeroed again: only for arenas that hold tables, never activation tensors with halos.
    void rewind()
    {
        while (chunks_.size() > 1) { (void)hipFree(chunks_.back()); chunks_.pop_back(); }
        if (!chunks_.empty()) { cur_ = (char *)chunks_[0]; left_ = first_size_; total_ = first_size_; }
    }

private:
    size_t chunk_min_ = (size_t)64 << 20, first_size_ = 0;
    std::vector<void *> chunks_;
    char *cur_ = nullptr;
    size_t left_ = 0, total_ = 0;
};

// 1-D activation [B][C][ld]: row = halo | T | halo (halo stays zero)
struct T1 {
    float *p = nullptr;   // -> [0][0][0]
    int B = 1, C = 0, T = 0, ld = 0, halo = 0;
    long long bs = 0;
    T1 rows(int c0, int n) const { T1 r = *this; r.p = p + (long long)c0 * ld; r.C = n; return r; }
};
// 2-D activation [B][C][H+2][W+2]
struct T2 {
    float *p = nullptr;   // -> interior (0,0) of channel 0
    int B = 1, C = 0, H = 0, W = 0, ld = 0, cs = 0;
    long long bs = 0;
    T2 chans(int c0, int n) const { T2 r = *this; r.p = p + (long long)c0 * cs; r.C = n; return r; }
};

static inline size_t t1_guard(int ld) { return (size_t)ld + 64; }
static inline size_t t2_guard(int ld) { return (size_t)ld * 2 + 64; }
static inline T1 make_t1(Arena &a, int B, int C, int T, int halo)
{
    T1 t;
    t.B = B; t.C = C; t.T = T; t.halo = halo;
    t.ld = (T + 2 * halo + 3) / 4 * 4;
    t.bs = (long long)C * t.ld;
    // guard rows in front and behind so clamped/garbage tail reads stay inside the allocation
    const size_t guard = t1_guard(t.ld);
    float *base = a.floats((size_t)B * t.bs + 2 * guard);
    t.p = base + guard + halo;
    return t;
}
static inline T2 make_t2(Arena &a, int B, int C, int H, int W)
{
    T2 t;
    t.B = B; t.C = C; t.H = H; t.W = W;
    t.ld = W + 2;
    t.cs = (H + 2) * t.ld;
    t.bs = (long long)C * t.cs;
    const size_t guard = t2_guard(t.ld);
    float *base = a.floats((size_t)B * t.bs + 2 * guard);
    t.p = base + guard + t.ld + 1;
    return t;
}

// ---------------------------------------------------------------------------------------
// prepared convolution weights: [nphase][M][Kp] panels (Kp = K rounded up to 16, zero padded)
// ---------------------------------------------------------------------------------------
struct ConvW {
    float *w = nullptr, *bias = nullptr;
    int M = 0, K = 0, Kp = 0, nphase = 1;
    int Cin = 0, Cout = 0, KW = 1, groups = 1;
    int S = 1, ntaps = 1;      // transposed convs
    bool transposed = false;
    bool owns = true;          // false: w / bias point into a buffer owned by another ConvW (merge_convs)
    std::vector<float> host_w; // row-major [Cout][K] copy kept for big 3x3 convs (plan-time tap pruning)
};

static inline int round16(int k) { return (k + 15) / 16 * 16; }


void *wmalloc(size_t bytes); void wfree(void *p);      // weight memory: slab-allocated per (device, class) (plan.hip)
void *wmalloc_plan(size_t bytes);                      // ... class 1: plan-lifetime copies, in slabs of their own
void wslab_info(int dev, int *count, size_t *bytes);
float *upload_f(const std::vector<float> &v, int cls = 0);
float *upload_f(const float *p, size_t n);
float *upload_fragments(const std::vector<float> &panel, int nphase, int M, int Kp, int cls = 0);
static inline long long phase_stride(const ConvW &c) { return (long long)((c.M + 15) / 16 * 16) * c.Kp; }
ConvW prep_conv(const float *w, const float *bias, int Cout, int Cin, int KW, int groups);
ConvW prep_convT1d(const float *w, const float *bias, int Cin, int Cout, int K, int S);
ConvW prep_convT2d(const float *w, const float *bias, int Cin, int Cout);
void free_conv(ConvW &c);
// conv32s_kernel's K order of a phase's fragment panel ((channel block, tap, channel group)-major): built ONCE per source panel by a device kernel and
// shared by every plan (and every trial of the autotuner); forgotten when the source conv is freed (plan.hip)
const float *c32s_panel(const float *src_frag, int M, int nchunks, int cin, int KW);
void merge_convs(const std::vector<ConvW *> &cs);

// ---------------------------------------------------------------------------------------
// op list ("plan") construction
// ---------------------------------------------------------------------------------------
// LayerNorm folded into the neighbouring GEMMs (ModelCV::fold_ln): one stream only.  The folded form works on streams folded into N as well
// (parity-tested in round 4), but the LayerNorm-consumer GEMM (two waves per SIMD, statistics in the operand stream) loses more on the wider
// N than the 31 launches save: 2 / 4 / 8 streams measured 3.33 / 5.09 / 8.30 ms with the fold against 3.30 / 4.83 / 7.85 without.
constexpr int LN_FOLD_MAX_STREAMS = 1;

struct ConvOpts {
    int act = ACT_NONE; float slope = 0.f; float scale = 1.f; bool accumulate = false;
    int pre_act = ACT_NONE; float pre_slope = 0.f;
    const float *res = nullptr; int res_cs = 0; long long res_bs = 0; int res_rs = 0;
    int m_off = 0, m_cnt = -1;   // output-row sub-range of the weight panel
    bool no_bias = false;
    bool glu = false;            // GLU-packed weight rows, gate fused into the epilogue (ModelSY flows)
    bool bf3 = false;            // exploratory: this 1x1 layer may run its products as three bf16 MFMAs (rvc_set_gemm_precision; igemm_bf3_kernel)
    int y_ws = 0;                // add_conv2d: output column stride in floats (0 = 1); with y.ld = 1 the layer writes its image transposed (RMVPE's head -> GRU input layout)
    bool final_out = false;      // the chunk's last convolution: writes the caller's device buffer when the call provides one (Plan::cur_out)
    // LayerNorm folded into its neighbours (IgemmP::ln_*): this layer consumes a not-yet-normalised tensor (weights pre-scaled, wsum
    // per output row, optional (mean, rstd) output) / this layer's residual is LayerNorm(stored tensor) with published statistics
    const float *ln_wsum = nullptr; float *ln_stats_out = nullptr; int ln_rows = 0;
    const float *ln_stats_in = nullptr, *ln_g = nullptr, *ln_b = nullptr;
};

// retrieval: a launch of the retrieval section (rvc_profile_last_knn counts it; bytes = its algorithmic bytes, 0 where they depend on the data); name: what
// rvc_debug_profile_dump calls a launch that has no description of its own
struct ProfEvent { hipEvent_t a, b; double flops; double bytes; int desc = -1; bool retrieval = false; const char *name = nullptr; };

struct Plan;
typedef std::function<void(hipStream_t)> Op;

struct TapRec { std::string name; int rank; T1 t1; T2 t2; };

// ops are tagged with the HIP stream they run on: 0 = main, 1 = auxiliary (the RMVPE branch runs
// concurrently with ContentVec; fork/join through events, captured as parallel branches of the hipGraph)
struct OpList {
    std::vector<Op> v;
    std::vector<int> sid;    // stream of the op (0 = main, 1..3 auxiliary)
    std::vector<int> kind;   // 0 = op, 1 = fork(sid): stream sid waits for main, 2 = join(sid): main waits for stream sid
    // issue order (indices into v): host launch order decides which concurrent branch is fed first.  Eager launches follow it
    // exactly; a captured hipGraph is submitted branch by branch, the branch of the first created node first.
    std::vector<int> order_eager, order_graph;
    int cur = 0;
    void push_back(Op o) { v.push_back(std::move(o)); sid.push_back(cur); kind.push_back(0); }
    void fork(int s) { v.push_back(Op()); sid.push_back(s); kind.push_back(1); }
    void join(int s) { v.push_back(Op()); sid.push_back(s); kind.push_back(2); }
};

// Everything that decides whether a cached plan serves a call.  engine.hip plan_key derives it from the engine and the call (callers add only `slot`), get_plan
// compares it as a whole and a new plan starts as a copy of it: a field added here is compared and assigned by construction.
struct PlanKey {
    int mode = 0;                 // 0 infer, 1 hubert only, 2 pitch only
    int B = 1; size_t L = 0, frame16k = 0; uint32_t skip_head = 0, R = 0;
    // formant shift (formant.hip.h): fstage = the plan has the formant stage (some stream stretches or resamples); the decoder then runs
    // on R2 frames and formant_resample_kernel brings every stream back to R upp samples.  fstage = false: R2 = R
    uint32_t R2 = 0; bool fstage = false;
    int slot = 0;                 // chunk pipelining (rvc_set_pipeline): plans alternate between two slots
    bool bucket = false;          // a plan of a bucketed call: built for a subset of the streams on the gathered state block (rvc_engine::d_state_bucket)
    bool with_index = false;      // an index is loaded and the index rate is above 0: the plan has the retrieval section
    bool with_protect = false;    // with_index and some stream of the plan has protect < 0.5: the plan carries protect_mix_kernel (protect.hip.h)
    bool bf3 = false;             // rvc_set_gemm_precision(e, 1): ContentVec's 1x1 GEMMs on the split-bf16 kernel (exploratory)
    bool with_taps = false;       // rvc_enable_taps: level 2 taps the production plan ...
    bool plain_plan = false;      // ... level 1 the explicit plan (LayerNorm launches, WaveNets layer by layer)
    int f0_method = 0;            // the engine's f0 method (the plan's f0 branch is that method's; 0 on the infer plan of a model without pitch guidance)
    int crepe_decoder = 0;        // ... and, for the CREPE methods, the engine's decoder (0 = Viterbi, 1 = arg-max; 0 on every other plan)
    double fcpe_threshold = 0;    // ... and, for FCPE, the engine's voicing threshold (baked into the decoder's launch; 0 on every other plan)
    // ... and, for RVC_F0_HYBRID, the members in the caller's order, 4 bits each from bit 0 (hybrid_pack), and the combination mode; both 0 on every other plan.  A
    // hybrid plan carries crepe_decoder / fcpe_threshold when a CREPE preset / FCPE is among its members
    uint32_t hybrid = 0; int hybrid_mode = 0;
    // f0 from outside: some stream of the call has a pending override, or the call is a conversion window under a curve.  Such a plan builds
    // its f0 branch through a plain row buffer, runs f0_override_kernel on it and feeds the pitch tail through f0_in; the values are no part of the key
    bool f0_override = false;
    int nprobe = 0;               // the engine's index_nprobe (with_index plans; 0 = flat search)
    int knn_k = KNN_K;            // the engine's index_k: the K of the retrieval kernels and the width of d_knn_idx / d_knn_dist
    bool operator==(const PlanKey &o) const
    {
        return std::tie(mode, B, L, frame16k, skip_head, R, R2, fstage, slot, bucket, with_index, with_protect, bf3, with_taps, plain_plan, f0_method, crepe_decoder, fcpe_threshold, hybrid, hybrid_mode, f0_override, nprobe, knn_k) ==
               std::tie(o.mode, o.B, o.L, o.frame16k, o.skip_head, o.R, o.R2, o.fstage, o.slot, o.bucket, o.with_index, o.with_protect, o.bf3, o.with_taps, o.plain_plan, o.f0_method,
                        o.crepe_decoder, o.fcpe_threshold, o.hybrid, o.hybrid_mode, o.f0_override, o.nprobe, o.knn_k);
    }
};

// the members of a hybrid f0 method as PlanKey::hybrid holds them, and back: -> the number of members
constexpr int HYBRID_MEMBERS_MAX = 4;
static inline uint32_t hybrid_pack(const int *m, int n) { uint32_t k = 0; for (int i = 0; i < n; i++) k |= (uint32_t)(m[i] & 15) << (4 * i); return k; }
static inline int hybrid_unpack(uint32_t k, int m[HYBRID_MEMBERS_MAX]) { int n = 0; for (; n < HYBRID_MEMBERS_MAX && ((k >> (4 * n)) & 15); n++) m[n] = (int)((k >> (4 * n)) & 15); return n; }

struct Plan {
    Arena arena;
    OpList ops;
    std::vector<TapRec> taps;
    PlanKey key;
    int T = 0, Tm = 0, C = 0; size_t N = 0;      // derived geometry
    // gather tables by content (round 6): the 3x3 layers of one RMVPE level have identical k -> offset tables; with one device copy per distinct table the second
    // and later layers of a level find it in the L2 instead of fetching a cold 6 KB table from HBM in front of their first operand gather
    std::map<std::vector<int>, const int *> koff_tabs;
    bool rm_fuse = false;         // RMVPE's shallow ConvBlockRes as one launch each (model_rmvpe.hip; decided per plan from the engine's f0 partition)
    bool autotune = false;        // rvc_set_plan_autotune: layers with several eligible kernels / tiles are chosen by timing them at plan build (plan.hip queue_igemm)
    double tune_ms = 0; int tuned_layers = 0, tune_changed = 0, tune_hits = 0;      // time spent in trials, layers tuned here / changed against the rules / taken from the process cache
    int dec_frames() const { return key.fstage ? (int)key.R2 : (int)key.R; }
    // I/O tensors
    float *d_in = nullptr;  // [B][L]
    T1 cv_out, audio;
    float *d_f0 = nullptr;  // [B][Tm]
    float *d_feat = nullptr; // extract_feature output (1,2T+1,C)
    int *d_knn_idx = nullptr; float *d_knn_dist = nullptr;
    int *d_ivf_scanned = nullptr; int ivf_queries = 0;  // IVF retrieval: rows scanned per (stream, query) of the last run, and how many such words
    int *d_knn_overflow = nullptr;                     // many-stream retrieval: one word per stream, raised when its candidate set overflowed (nullptr on the one-launch form)
    // one-launch retrieval: its ticket counters, and what runs instead when a selector gave up (engine.hip recover_retrieval)
    unsigned *knn_ticket = nullptr; size_t knn_ticket_bytes = 0;
    std::vector<Op> knn_fallback;
    size_t op_phone = 0, op_ret_begin = 0, op_ret_end = 0;      // ops [op_phone, op_ret_begin): phone gather; [op_ret_begin, op_ret_end): the retrieval section
    unsigned opt_gen = 0;         // test-hook generation the plan was built under
    // profiling
    bool profile = false;
    std::vector<ProfEvent> prof;
    std::vector<std::string> descs;   // per-op description for rvc_debug_profile_dump
    size_t prof_used = 0;
    double igemm_flops = 0;
    int n_igemm = 0;
    std::vector<float *> owned_dev;   // plan-time repacked weights
    // timeline probe (RVC_STAMPS=1): one device timestamp per section boundary
    unsigned long long *d_stamps = nullptr; std::vector<std::string> stamp_names;
    // chunk pipelining (rvc_set_pipeline, PlanKey::slot): ev_done marks the end of this plan's previous chunk
    hipEvent_t ev_done = nullptr; bool ev_done_valid = false;
    // per-call pointers (eager launches): the kernels that read the input / write the audio take them at launch time, so a device-resident
    // caller needs no staging copy in front of the chunk and no copy behind it (a captured graph bakes pointers: it keeps d_in / audio)
    const float *cur_in = nullptr; float *cur_out = nullptr; long long cur_out_bs = 0;
    bool in_direct_ok = true, out_direct_ok = false;
    bool final_out_honoured = false;     // the chunk's last convolution was queued on a launch path that writes Plan::cur_out (queue_igemm reports it)
    // graph
    hipGraphExec_t graph_exec = nullptr;
    // run time: the next profile slot of this run (its events are created on first use; the engine rewinds prof_used per run), nullptr when not profiling
    ProfEvent *prof_slot(double flops, double bytes, int desc, const char *retrieval_name = nullptr)
    {
        if (!profile) return nullptr;
        if (prof_used == prof.size()) { ProfEvent e; HIPCHK(hipEventCreate(&e.a)); HIPCHK(hipEventCreate(&e.b)); prof.push_back(e); }
        ProfEvent *pe = &prof[prof_used++];
        pe->flops = flops; pe->bytes = bytes; pe->desc = desc; pe->retrieval = retrieval_name != nullptr; pe->name = retrieval_name;
        return pe;
    }
    ~Plan()
    {
        for (float *p : owned_dev) wfree(p);
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        if (ev_done) (void)hipEventDestroy(ev_done);
        for (auto &e : prof) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    }
};


// ---- planner entry points (plan.hip) ----
extern unsigned long long *g_kprobe;      // tuning build (-DRVC_KPROBE): destination of the per-wave phase stamps
extern int g_last_waves, g_last_wgs, g_ncu;
extern thread_local char g_last_kernel[32];      // this thread's most recently queued launch: implicit-GEMM family ("reg", "g32", "c32s", ...) or op variant ("attn_mfma2", "ln_strip12", ...)
extern thread_local char g_last_desc[200];       // ... and the whole description of the last implicit-GEMM launch queued ("reg M=.. N=.. ... split=2")
void queue_igemm(Plan &pl, IgemmP p, int B, const std::vector<int> &koff, const std::vector<PhaseD> &phases, bool final_out = false);
// one GEMM-class launch of the planner (description, FLOPs, launch shape, profile slot, final_out): launch(q, ea, eb, stream) gets the IgemmP to use and the
// slot's events.  Defined and instantiated in plan.hip (the body is inlined into the op, as lean as a hand-written one)
template <class Launch> void queue_gemm_launch(Plan &pl, const char *desc, double flops, int wgs, int waves, bool final_out, const IgemmP &p, Launch launch);
void fill_epilogue(IgemmP &p, const ConvW &cw, const ConvOpts &o);
void add_conv1d(Plan &pl, const ConvW &cw, const T1 &x, const T1 &y, int stride, int pad, int dil, ConvOpts o = ConvOpts());
void add_conv1d_multi(Plan &pl, const std::vector<const ConvW *> &cws, const T1 &x, bool x_grouped, const T1 &y,
                      const std::vector<int> &pads, const std::vector<int> &dils, ConvOpts o = ConvOpts(), bool res_grouped = true);
void add_conv1d_two(Plan &pl, const ConvW &c0, const ConvW &c1, const float *pair_bias, const T1 &x, const T1 &y0, const T1 &y1);
void add_convT1d(Plan &pl, const ConvW &cw, const T1 &x, const T1 &y, int pad, ConvOpts o = ConvOpts());
void add_conv2d(Plan &pl, const ConvW &cw, const T2 &x, const T2 &y, ConvOpts o = ConvOpts());
void add_convT2d(Plan &pl, const ConvW &cw, const T2 &x, const T2 &y, ConvOpts o = ConvOpts());
void add_layernorm(Plan &pl, const T1 &x, const float *g, const float *b);
// multi-head self-attention over qkv [B][3E][ld] (q, k, v rows) into out [B][E][ld], scale 1/sqrt(head size): ContentVec (plain) and the synthesizer's
// text encoder (relative positions: rel_k / rel_v [2 window + 1][head size]).  Kernel variants and their test hooks: plan.hip
void add_attention(Plan &pl, const T1 &qkv, const T1 &out, int heads);
void add_relpos_attention(Plan &pl, const T1 &qkv, const T1 &out, int heads, const float *rel_k, const float *rel_v, int window);
// bidirectional GRU recurrence: gi [B][6H][ld] gate pre-activations (b_ih included) -> out [B][2H][ld]; whh / whhT / bhh: gru_prep_whh layouts (device);
// status: per-stream status words (stride status_stride ints), raised by the multi-workgroup kernel on a hand-off timeout
void add_gru(Plan &pl, const T1 &gi, const T1 &out, int H, const float *whh, const float *whhT, const float *bhh, int *status, int status_stride);
void add_stamp(Plan &pl, const char *name);
void add_tap(Plan &pl, const char *name, const T1 &t);
void add_tap2(Plan &pl, const char *name, const T2 &t);
void plan_kernel_attrs();                 // per-device function attributes of the kernels each unit launches
void retrieval_kernel_attrs();

// ---------------------------------------------------------------------------------------
// models
// ---------------------------------------------------------------------------------------
struct DevVec { float *p = nullptr; };
static inline float *dv(const Blob &b, const std::string &name) { const BlobTensor &t = b.t(name); return upload_f(t.data, t.nelem); }

struct ModelCV {
    int conv_dim, embed, heads, ffn, run_layers, pos_k, pos_groups, out_dim;
    int conv_k[7], conv_s[7];
    ConvW conv[7], proj, pos, final_proj;
    float *gn_g, *gn_b, *ln0_g, *ln0_b, *encln_g, *encln_b;
    float *conv0_raw = nullptr;     // [conv_dim][conv_k0] row-major copy of the first conv (fused conv + GroupNorm + GELU kernel)
    // qkv_f / ff1_f: the same projections with the PRECEDING LayerNorm folded in (W' = W diag(g), b' = b + W beta, wsum = row sums of W'):
    // one-stream plans feed them the not-yet-normalised tensor and drop the LayerNorm launches (build_contentvec)
    struct Layer { ConvW qkv, o, ff1, ff2, qkv_f, ff1_f; float *qkv_wsum = nullptr, *ff1_wsum = nullptr; float *ln1_g, *ln1_b, *ln2_g, *ln2_b; };
    bool has_folded = false;
    ConvW proj_f; float *proj_wsum = nullptr;      // feature projection with the LayerNorm over the conv features folded in
    static ConvW fold_ln(const float *w, const float *bias, int M, int K, const float *g, const float *beta, float **wsum_dev);      // (model_cv.hip)
    std::vector<Layer> layers;
    std::vector<float *> owned;
    size_t weight_bytes = 0;
    explicit ModelCV(const Blob &b);
    ~ModelCV();
    int out_frames(size_t L) const
    {
        long long T = (long long)L;
        for (int i = 0; i < 7; i++) { if (T < conv_k[i]) return 0; T = (T - conv_k[i]) / conv_s[i] + 1; }
        return (int)T;
    }
};

struct ResBlockW {
    ConvW c1, c2, sc; bool has_sc = false; int ci = 0, co = 0; float *pair_bias = nullptr;      // pair_bias: [c1.bias; sc.bias] for the fused c1 + shortcut launch
    // rm_block_kernel (rmblock.hip.h; blocks with 16 / 32 / 64 output channels): the three weight panels in its fragment order
    // [tap][Cin16 / 4][Cout / 16][64 lanes] (lane (li, kq) = W[16 mt + li][4 c4 + kq][tap], zero beyond Cin), packed once at model load
    // (one allocation [w1 | w2 | wsc]: the kernel touches every 128-byte line of it once at its start -- the panels are cold in HBM at every chunk)
    float *f_w1 = nullptr, *f_w2 = nullptr, *f_sc = nullptr; int f_lines = 0;
};
// one ConvBlockRes from weights in PyTorch layout: w1 [co][ci][3][3], w2 [co][co][3][3], wsc [co][ci] (nullptr: identity shortcut), biases [co] (BatchNorm
// folded): the prepared convolutions, the pair bias of the c1 + shortcut launch and -- 16 / 32 output channels, at most 64 input channels -- rm_block_kernel's
// panels.  ModelRM builds its blocks with it, and so does rvc_debug_rm_block (debug.hip)
ResBlockW make_res_block(const float *w1, const float *b1, const float *w2, const float *b2, const float *wsc, const float *bsc, int ci, int co);
void free_res_block(ResBlockW &r);
// the recurrent weights of a bidirectional GRU (PyTorch weight_hh_l0 / _reverse, [3H][H] each, gates r, z, n) in the two layouts of the kernels:
// whhT [2][H][3H] (gru_kernel: lanes read consecutive rows) and whh [2][3H][H] row-major (gru_multi_kernel)
void gru_prep_whh(const float *const whh_dir[2], int H, std::vector<float> &whhT, std::vector<float> &whh);

struct ModelRM {
    int en_out, levels, n_blocks, inter_layers, n_mels, gru_hidden, n_out;
    float bn_scale, bn_shift;
    std::vector<std::vector<ResBlockW>> enc, inter, dec;
    std::vector<ConvW> up;
    ConvW cnn, gru_ih, fc;
    float *whhT = nullptr, *bhh = nullptr, *whh = nullptr;
    size_t weight_bytes = 0;
    static ResBlockW block(const Blob &b, const std::string &pre, int ci, int co);
    explicit ModelRM(const Blob &b);
    ~ModelRM();
};

// CREPE (model_crepe.hip): six convolutions (capacity `cap`: 32 = full, 4 = tiny), BatchNorm as per-channel scale and shift applied
// behind the ReLU, the classifier as a 1x1 convolution over the [4 * 16 cap] features (time major, channel minor), Hz per bin
struct ModelCR {
    int cap = 0;
    ConvW conv[6], fc;
    float *scale[6] = {}, *shift[6] = {}, *f0tab = nullptr;
    size_t weight_bytes = 0;
    explicit ModelCR(const Blob &b);
    ~ModelCR();
    ModelCR(const ModelCR &) = delete; ModelCR &operator=(const ModelCR &) = delete;
};

// FCPE (model_fcpe.hip): the input stack (two k = 3 convolutions around GroupNorm(4)), `layers` blocks of LayerNorm -> pointwise H -> 2 I ->
// GLU -> depthwise 31 -> SiLU -> pointwise I -> H, the final LayerNorm and the classifier (weight norm folded by the importer); its own Slaney filterbank for
// the mel front end (basis [128][513], band [128][2] as ints) and Hz per bin
struct ModelFC {
    int H = 0, I = 0, layers = 0;
    ConvW in0, in1, out;
    float *gn_g = nullptr, *gn_b = nullptr, *norm_g = nullptr, *norm_b = nullptr, *basis = nullptr, *f0tab = nullptr;
    int *band = nullptr;
    struct Layer { float *ln_g = nullptr, *ln_b = nullptr, *dw_w = nullptr, *dw_b = nullptr; ConvW pw1, pw2; };
    std::vector<Layer> ly;
    size_t weight_bytes = 0;
    explicit ModelFC(const Blob &b);
    ~ModelFC();
    ModelFC(const ModelFC &) = delete; ModelFC &operator=(const ModelFC &) = delete;
};

// GLU row packing of a WaveNet in-layer (igemm_common.hip.h glu_store): packed row f*16 + kq*4 + r <- model row f*8 + kq*2 + (r&1) of the tanh half (r < 2)
// or the sigmoid half (r >= 2, + H).  w: [2H][K] in model row order, bias: [2H]
template <typename T> void glu_pack_rows(const T *w, const float *bias, int H, size_t K, std::vector<float> &wp, std::vector<float> &bp);      // (model_synth.hip: float and double)
// ... the map itself, both ways (H a multiple of 8): the packed row that holds model row m of [2H], and the model row packed row p holds.  glu_pack_rows
// walks the second, speaker_fold_kernel (speaker.hip.h) stores through the first
__host__ __device__ static inline int glu_model_row(int p, int H) { const int f = p >> 4, kq = (p & 15) >> 2, rr = p & 3; return f * 8 + kq * 2 + (rr & 1) + (rr >= 2 ? H : 0); }
__host__ __device__ static inline int glu_packed_row(int m, int H) { const int hi = m >= H ? 1 : 0, q = m - hi * H; return (q >> 3) * 16 + ((q & 7) >> 1) * 4 + (q & 1) + 2 * hi; }

// Run-time speaker selection (speaker.hip.h).  The speaker enters the synthesizer as cond(g), a per-channel constant folded into the
// biases of the flows' in-layers and of dec_pre.  A blob with a speaker table (sy.emb_g [n_spk][gin]) keeps the table, every cond layer and the unfolded biases
// on the device; one launch of speaker_fold_kernel rewrites the live bias buffers in place for g = sum_i w_i emb_g[id_i].
constexpr int SPK_MAX_MIX = 8;
struct SpeakerMix { int n; int id[SPK_MAX_MIX]; float w[SPK_MAX_MIX]; };
// one conditioned layer: bias[r] = base_b[r] + cond_b[r] + cond_w[r][:] . g for its `rows` model rows (global rows row0 ..), stored to dst0 and -- when not
// null -- dst1, at the GLU-packed position of r (glu_h = the layer's H) or at r itself (glu_h = 0)
struct SpeakerLayer { const float *base_b, *cond_w, *cond_b; float *dst0, *dst1; int row0, rows, glu_h; };

struct ModelSY {
    int phone_dim, hidden, inter, filter, heads, enc_layers, enc_k, window, flow_n, wn_layers, wn_k, gin, up_init, n_ups, n_rb, n_rbd, sr;
    int up_rate[8], up_kernel[8], rb_k[8], rb_d[8];
    // has_f0 (config key f0, absent = 1): false = a model trained without pitch guidance (upstream's ..NSFsid_nono: no pitch embedding, a plain HiFi-GAN
    // decoder).  Its blob has no sy.enc.pitch_emb, sy.src, sy.dec.nc*: pitch_emb stays null, ncs empty; its plans have no pitch branch (engine.hip get_plan)
    bool has_f0 = true;
    ConvW phone, proj;
    float *pitch_emb = nullptr;
    // qkv_f: the projection with the previous layer's second LayerNorm folded in (ModelCV::fold_ln); proj_f likewise for the last layer.
    // (The first LayerNorm of a layer feeds a 3-tap convolution with zero padding: padded positions are zero AFTER the norm, so it stays.)
    struct Layer {
        ConvW qkv, o, ff1, ff2, qkv_f; float *qkv_wsum = nullptr; float *rel_k, *rel_v, *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    };
    ConvW proj_f; float *proj_wsum = nullptr; bool has_folded = false;
    std::vector<Layer> layers;
    struct Flow {
        ConvW pre, post; std::vector<ConvW> in, rs; bool flipped = false;
        // one stream: the WaveNet with its 1x1 res_skip layers composed into the following in-layers (compose_flows): host copies of the
        // layer weights in model order, and the composed panels
        std::vector<float> h_pre_w, h_pre_b, h_post_w, h_post_b;
        std::vector<std::vector<float>> h_in_w, h_in_b, h_rs_w, h_rs_b;
        ConvW pre1, postc, posth; std::vector<ConvW> inc; float *pair_bias = nullptr;      // postc: z_next rows, posth: the next flow's h0 rows
    };
    bool composed = false;
    std::vector<Flow> flows;
    ConvW dec_pre, dec_post;
    std::vector<ConvW> ups, ncs;
    std::vector<std::vector<std::vector<std::pair<ConvW, ConvW>>>> rbs;   // [stage][kernel][dilation] -> (c1, c2)
    float src_w = 0.f, src_b = 0.f;
    std::vector<float *> owned;
    size_t weight_bytes = 0;
    // run-time speaker selection: n_spk = rows of the blob's table (1 without one: the one speaker is sy.g, id 0, and nothing below is allocated).  The mix in
    // force is (mix_id, mix_w)[mix_n], weights normalised in double; spk_baked = the live biases are still the host fold of sy.g made at load (no set call has
    // been made, mix = {sid_g: 1}); spk_dirty = a set call (or a late compose_flows) has left the live biases behind the mix: the next chunk queues the fold.
    // The buffers the fold writes (F.in[j].bias, F.inc[j].bias, dec_pre.bias) belong to this ModelSY alone.
    int n_spk = 1, sid_g = 0;
    float *spk_emb = nullptr;                          // [n_spk][gin]
    std::vector<SpeakerLayer> spk_layers; SpeakerLayer *d_spk_layers = nullptr; int spk_rows = 0;
    SpeakerMix *d_spk_mix = nullptr, *h_spk_mix = nullptr;      // h: pinned ring of 8, one block per queued fold (its async copy reads the block later)
    unsigned spk_slot = 0; hipEvent_t spk_ev[8] = {}; bool spk_ev_used[8] = {};
    hipEvent_t spk_prof[2] = {nullptr, nullptr}; bool spk_prof_valid = false;      // around the last fold queued under rvc_set_profile
    int mix_n = 1; int32_t mix_id[SPK_MAX_MIX] = {}; double mix_w[SPK_MAX_MIX] = {1.0};
    bool spk_baked = true, spk_dirty = false;
    bool has_speaker_table() const { return spk_emb != nullptr; }
    void speaker_setup(const Blob &b);                                             // at load, when the blob has sy.emb_g
    void speaker_targets();                                                        // (re)point the layer table at the live bias buffers
    void set_speaker_mix(const int32_t *sid, const double *weight, size_t n);      // ShapeError on a bad mix, state unchanged
    void queue_speaker_fold(hipStream_t s, bool profile);                          // the one launch (+ the copy of the mix), only when spk_dirty
    void speaker_biases(bool composed_copy, std::vector<float> &out);              // the live folded biases in model row order (rvc_debug_speaker_biases)
    explicit ModelSY(const Blob &b);
    void compose_flows();      // (model_synth.hip)
    ~ModelSY();
    int upp() const { int u = 1; for (int i = 0; i < n_ups; i++) u *= up_rate[i]; return u; }
};

}  // namespace rvc

namespace rvc {
struct StreamSet; struct IndexBuild;
// The retrieval index as the engine owns it (retrieval.hip install_index is the one place that fills it): the row-major matrix, its device-side layouts (rowsT:
// [dim][n], built on demand by ensure_index_transposed; rowsF: MFMA fragment order; ynorm / nhn: |y|^2 and -|y|^2 / 2) and the IVF structure over its rows
// (rvc_set_index_ivf / rvc_train_index_ivf; ivf.hip.h): centroids, CSR offsets and the row permutation.  An empty `rows` = no index.
struct IvfLists { DevBuf<float> cent; DevBuf<int> offs, perm; size_t nlist = 0, longest = 0, empty = 0; };
struct RetrievalIndex {
    DevBuf<float> rows, rowsT, rowsF, ynorm, nhn; size_t n = 0, dim = 0;
    float prep_ms = 0.f;                              // device-side repack + norms of the load
    IvfLists ivf;
};
}  // namespace rvc
using namespace rvc;

struct rvc_engine {
    std::string data_path, err;
    int device = 0;
    // aux streams: 1 = f0 branch, 2 = side work (NSF source), 3 = ContentVec branch when the CUs are partitioned.  Four streams
    // in total: the runtime multiplexes streams onto 4 hardware queues, a fifth stream would share (and serialise with) another.
    hipStream_t stream = nullptr, aux[3] = {nullptr, nullptr, nullptr};
    struct rvc::StreamSet *sset = nullptr;             // the engine's streams are borrowed from a per-device pool (never destroyed)
    int cv_cus = 256;                                 // CUs the ContentVec branch (and the retrieval behind it) runs on: all, or all minus the f0 partition
    bool partition_ok = false, partitioned = false;   // CU-masked streams available / currently in use (n_streams <= 4)
    hipEvent_t ev_fork[3] = {nullptr, nullptr, nullptr}, ev_join[3] = {nullptr, nullptr, nullptr};
    std::unique_ptr<ModelCV> cv;
    std::unique_ptr<ModelRM> rm;
    int f0_method = 0;                                // 0 none, RVC_F0_RMVPE (rm is loaded), RVC_F0_YIN / RVC_F0_PM (no weights), RVC_F0_CREPE / _TINY (cr_full / cr_tiny); engine-wide (PlanKey)
    std::unique_ptr<ModelCR> cr_full, cr_tiny;        // each stays loaded once read: going back to it costs no file and keeps its plans
    std::unique_ptr<ModelFC> fc;                      // FCPE (RVC_F0_FCPE), kept once read like the CREPE presets
    int hybrid_n = 0, hybrid_m[rvc::HYBRID_MEMBERS_MAX] = {}, hybrid_mode = 0;      // f0_method == RVC_F0_HYBRID: the members (the lead first) and the mode (rvc_load_f0_hybrid); hybrid_n = 0 otherwise
    double fcpe_threshold = 0.006;                    // rvc_set_fcpe_threshold: f0 = 0 where the top posterior is at or below it; engine-wide (PlanKey)
    int crepe_decoder = 0;                            // rvc_set_crepe_decoder: 0 = Viterbi, 1 = arg-max; engine-wide (PlanKey)
    std::unique_ptr<ModelSY> sy;
    // constants for the mel front end
    float *d_window = nullptr, *d_twiddle = nullptr, *d_basis = nullptr; int *d_band = nullptr;
    // retrieval index: what is loaded (index) and the caller's preferences, which are no part of it.  index_nprobe: 0 = flat search, else the lists probed per
    // query; engine-wide (PlanKey); a new index or a dropped IVF structure resets it
    rvc::RetrievalIndex index;
    float index_rate = 0.f;
    int index_nprobe = 0;
    int index_k = KNN_K;                                        // neighbours blended per query (rvc_set_index_k: 4 or 8); the caller's preference, kept across index loads (PlanKey)
    // the last k-means training of an IVF structure (rvc_train_index_ivf; kmeans.hip.h): what rvc_index_ivf_train_info reports
    bool km_valid = false; int km_iters_run = 0; size_t km_moved_last = 0; std::vector<double> km_obj; double km_ms[3] = {0, 0, 0};
    rvc::IndexBuild *ib = nullptr;                              // an open index build (rvc_index_build_begin .. _finish / _abort; retrieval.hip); never touches `index` before finish
    double bcast_ms[3] = {0, 0, 0}; int bcast_ranks = 0;         // last rvc_index_broadcast: communicator set-up, broadcast, repack (ms); ranks the communicator reports
    // streams
    int n_streams = 1;
    StreamState *d_state = nullptr;
    StreamState *d_state_bucket = nullptr; int *d_bucket_idx = nullptr;      // rvc_infer_batch_g: the states of one geometry bucket, gathered contiguously, and their stream numbers
    CallParams *d_cp = nullptr, *h_cp = nullptr;   // h_cp: ring of 64 pinned blocks, one per call (an async copy reads its block later)
    unsigned cp_slot = 0; hipEvent_t ev_cp = nullptr;
    uint32_t seed = 0, stream_id0 = 0;
    // plans (keyed by PlanKey, least recently used first)
    std::vector<std::unique_ptr<Plan>> plans;
    Plan *last_plan = nullptr;
    int gemm_precision = 0;           // 0 = fp32 everywhere (the product), 1 = split-bf16 for ContentVec's 1x1 GEMMs at many streams (exploratory)
    int plan_cap = 8;                 // rvc_set_plan_cache
    int autotune = 1;                 // rvc_set_plan_autotune: 1 = plans of more than 4 streams pick among eligible kernels by timing them at plan build, 0 = the rules only
    double last_build_ms = 0;         // wall time of the last plan build (rvc_plan_autotune_info)
    int last_tuned = 0, last_changed = 0, last_hits = 0; double last_tune_ms = 0;
    long long knn_recoveries = 0;     // chunks whose retrieval was recomputed after a hand-off time-out (rvc_retrieval_info)
    long long plan_builds = 0;        // plans built since rvc_create (a miss = arena allocation + composed weights + a device synchronisation)
    int taps_on = 0;               // 0 off, 1 taps on the explicit plan, 2 taps on the production plan (rvc_enable_taps)
    bool profile_on = false, use_graph = false;
    // offline throughput mode: consecutive unsynchronised infer_device calls overlap chunk i+1's two front branches with chunk i's
    // synthesizer (two plan slots; the branch streams are ordered by events instead of forking from the main stream)
    bool pipeline = false, pipe_now = false; int pipe_slot = 0; hipEvent_t ev_in = nullptr; const void *pipe_input = nullptr; size_t pipe_input_bytes = 0;
    // per-stream controls (StreamCtl, state.hip.h): what the device holds (with the seed), and a pinned ring of 8 blocks of 4096, one block per strided copy that
    // changes them (the async copy reads its block later; ev_up: completion of the copy that last read a block).  engine.hip push_call_params
    std::vector<rvc::StreamCtl> pushed_ctl; uint32_t pushed_seed = 0; bool pushed_valid = false;
    rvc::StreamCtl *h_ctl = nullptr; unsigned up_slot = 0;
    hipEvent_t ev_up[8] = {}; bool ev_up_used[8] = {};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.f;
    size_t last_knn_rows = 0;
    // The settings behind the controls, per stream and the default of streams rvc_set_streams adds later (rvc_reset_state leaves them alone): formant shift in
    // semitones (rvc_set_formant_shift[_stream]), the pitch controls (f0cond.hip.h; rvc_set_pitch_semitones / f0_range / f0_median / f0_snap [_stream]) and consonant
    // protection ([0, 0.5], 0.5 = off; rvc_set_protect[_stream]).  What of them is a plan's identity is PlanKey's R2 / fstage and with_protect; the values travel in
    // StreamCtl (the transpose as a factor of the multiplier) and are not.
    struct PitchCtl { double semitones = 0.0; float lo = 0.f, hi = INFINITY; int radius = 0; uint32_t mask = 0; float strength = 0.f; };
    struct StreamSettings { double formant = 0.0; PitchCtl pitch; double protect = rvc::PROTECT_OFF; };
    std::vector<StreamSettings> settings; StreamSettings settings_default;
    // formant filter tables by ratio (o, n): device memory for the engine's life (a captured graph's descriptors point at them)
    std::map<std::pair<int, int>, rvc::FormantTable> ftabs;
    // the file converter (convert.hip.h): the high-pass taps on the device (uploaded by the first call that filters) and what
    // rvc_convert_info reports of the last completed convert
    rvc::DevBuf<float> hp_taps;
    struct ConvertInfo { bool valid = false; size_t windows = 0, batches = 0; std::vector<int32_t> offsets; double ms[4] = {0, 0, 0, 0}; } conv;
    // ... and rvc_convert_many_info of the last completed rvc_convert_many (convert_many.hip.h): offsets in global window order
    ConvertInfo many;
    // ... and rvc_convert_file_info of the last completed rvc_convert_file
    struct FileInfo { bool valid = false; double ms[7] = {0, 0, 0, 0, 0, 0, 0}; size_t rate_out = 0; float peak = 0.f; } file;
    // f0 from outside (f0_override.hip.h).  ov[s]: the pending override rows of stream s (empty = none), for the END of its next f0 window;
    // ov_hold: an override stays until cleared instead of being consumed by the next call of its stream.  d_ov: the device block a plan with the select reads
    // every chunk -- F0OvCall | count per stream | rows [streams][1024] -- allocated with the first such plan, freed with the stream states (alloc_state, which
    // drops the plans that bake its address); ov_dirty: the block is behind `ov`.  ov_ring: pinned blocks the block's copies are queued from, each reused only
    // after its copies have completed.  curve_*: the recording's curve for rvc_convert* (breakpoints in HBM) and, during a conversion that uses it, its grid
    std::vector<std::vector<float>> ov; bool ov_hold = false, ov_dirty = true;
    char *d_ov = nullptr; hipStream_t ov_stream = nullptr;
    struct OvBlock { char *p = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool used = false; } ov_ring[8]; unsigned ov_slot = 0;
    rvc::DevBuf<double> curve_t; rvc::DevBuf<float> curve_hz, curve_grid; size_t curve_n = 0;
    bool conv_curve = false; rvc::F0OvCall conv_call{};          // inside convert_run with a curve: the gather of the batch at hand
    std::vector<float> conv_f0; bool conv_f0_valid = false;      // the conditioned f0 of the last completed conversion on the 10 ms grid (rvc_convert_f0)
    // f0 analysis and auto-transpose (f0_analyze.hip.h, f0_select.hip.h).  sel_ws: the select's workspace, allocated by the first select.
    // at_*: rvc_set_auto_transpose (target 0 = off).  auto_mul: inside a conversion that transposes by a != 0 the factor (float)2^(a / 12) every stream's
    // multiplier takes behind its semitone factor (push_call_params), 0 = none -- set and removed by convert_run alone, so streaming calls never see it.
    // at_info: what rvc_auto_transpose_info reports of the last conversion that ran the analysis
    rvc::DevBuf<uint32_t> sel_ws;
    double at_target = 0.0; int at_step = 1; double at_limit = 12.0;
    float auto_mul = 0.f;
    struct AutoInfo { bool valid = false; float median = 0.f; size_t voiced = 0; double semitones = 0.0; double ms[2] = {0, 0}; } at_info;
    // per-file pitch of rvc_convert_many (f0_analyze_many.hip.h), read by rvc_convert_many alone and kept over model loads.
    // many_semitones: rvc_set_convert_many_pitch, one entry per file of the next call (empty = cleared); many_at_*: rvc_set_convert_many_auto_transpose
    // (target 0 = off).  many_mul: auto_mul per stream -- inside convert_many_run the factor (float)2^(t_f / 12) of the file whose window the stream holds in
    // the batch at hand, 0 = none, empty outside the call.  many_pitch: what rvc_convert_many_pitch_info reports of the last call that ran the pass
    std::vector<double> many_semitones;
    double many_at_target = 0.0; int many_at_step = 1; double many_at_limit = 12.0;
    std::vector<float> many_mul;
    struct ManyPitchInfo { bool valid = false; std::vector<float> median; std::vector<size_t> voiced; std::vector<double> a, t; double ms[2] = {0, 0}; } many_pitch;
    // the file converter's silence gate (silence.hip.h).  sil_db / sil_hang: rvc_set_convert_silence (at or below -60 dB = off), kept over
    // model loads.  sil_info: what rvc_convert_silence_info reports of the last completed call that ran with the gate
    double sil_db = -60.0; int sil_hang = 30;
    struct SilenceInfo { bool valid = false; size_t run = 0, skipped = 0, loud = 0, kept = 0; double ms = 0.0; } sil_info;
    int *h_status = nullptr;        // pinned, one word per stream (up to 4096)
    bool status_queued = false;     // an async copy of the status words is already in the stream in front of the caller's sync
};


namespace rvc {
static inline void set_device(rvc_engine *e) { HIPCHK(hipSetDevice(e->device)); }
template <typename Fn> static rvc_status guarded(rvc_engine *e, Fn fn)
{
    if (!e) return RVC_BACKEND;
    try {
        set_device(e);
        return fn();
    } catch (const ShapeError &x) { e->err = x.what(); return RVC_SHAPE; }
    catch (const PanicError &x) { e->err = x.what(); return RVC_PANIC; }
    catch (const std::exception &x) { e->err = x.what(); return RVC_BACKEND; }
}
// ---- model builders (model_*.hip) and the retrieval unit (retrieval.hip) ----
T1 build_contentvec(rvc_engine *e, Plan &pl, int B, size_t L);
T1 build_rmvpe(rvc_engine *e, Plan &pl, int B, size_t L, size_t frame16k, bool update_cache);
void build_pitch_post(rvc_engine *e, Plan &pl, int B, const T1 &sal, bool update_cache, size_t frame16k, size_t hubert_length, float **pitchf_out, int **pitch_out, const float *f0_in = nullptr);
float *build_yin(rvc_engine *e, Plan &pl, int B, size_t L, size_t frame16k);
// (method: the preset, RVC_F0_CREPE or RVC_F0_CREPE_TINY; pre: the prefix of its tap and stamp names -- a hybrid of both presets names the second one apart)
float *build_crepe(rvc_engine *e, Plan &pl, int B, size_t L, size_t frame16k, int method, const char *pre = "cr");
// CREPE's decoder alone (crepe_decode_kernel, crepe.hip.h): the plan's launch and rvc_debug_crepe_decode's (debug.hip).  prob [B][Tm][360]; bp: B * Tm * 360 bytes of
// back-pointers where crepe_backpointer_bytes says so (long windows; shorter ones keep them in LDS); bins / pd may be null
std::vector<float> crepe_f0_table();
size_t crepe_backpointer_bytes(int B, int Tm);
void launch_crepe_decode(hipStream_t s, int B, const float *prob, int Tm, int decoder, const float *f0tab, unsigned char *bp, float *f0, int *bins, float *pd);
float *build_fcpe(rvc_engine *e, Plan &pl, int B, size_t L, size_t frame16k);
// "pm", Praat's autocorrelation tracker (f0_pm.hip, pm.hip.h): build_yin's contract.  launch_pm_cand: the stream peaks and the candidates of
// every frame (gpk [B][2]; cn [B][Tm]; cf / cs / cd [B][Tm][15]); launch_pm_path: the Viterbi path over them (path, f0 [B][Tm]).  Both are rvc_debug_pm's launches
float *build_pm(rvc_engine *e, Plan &pl, int B, size_t L, size_t frame16k);
std::vector<float> pm_rw_table();
void launch_pm_cand(hipStream_t s, int B, const float *audio, long long audio_bs, int n, int frame, int Tm, const float *rw, float *gpk, int *cn, float *cf, float *cs, float *cd);
void launch_pm_path(hipStream_t s, int B, int Tm, const int *cn, const float *cf, const float *cd, int *path, float *f0);
// FCPE's decoder and its GLU + depthwise + SiLU kernel alone (fcpe.hip.h): the plan's launches and the debug entries' (debug.hip).  Decoder: logit [B][360][l_ld]
// (sigmoid applied, posteriors written to prob [B][Tm][360]) or, with logit null, the caller's posteriors prob_in; bins may be null.  Depthwise: z [B][2 I][z_ld] ->
// y [B][I][y_ld], w [I][31], bias [I]
std::vector<float> fcpe_f0_table();
float fcpe_cent_step();
void launch_fcpe_decode(hipStream_t s, int B, int Tm, const float *logit, int l_ld, long long l_bs, const float *prob_in, float *prob, const float *f0tab, double threshold, float *f0, int *bins);
void launch_fcpe_glu_dw(hipStream_t s, int B, int I, int T, const float *z, int z_ld, long long z_bs, const float *w, const float *bias, float *y, int y_ld, long long y_bs);
// hybrid f0 (f0_hybrid.hip.h): one launch that decodes RMVPE's salience sal [B][360][ld] to unshifted Hz when RMVPE is member rm_at (-1:
// not a member, sal unread) and combines the n member rows [B][Tm] (rows[0] the lead's; rows[rm_at] unread) into out [B][Tm].  launch_f0_hybrid: the plan's
// launch (add_f0_hybrid queues it and returns the combined row, which build_pitch_post takes as f0_in) and rvc_debug_f0_hybrid's (debug.hip).  rm_f0: RMVPE's
// decoded row, may be null
void launch_f0_hybrid(hipStream_t s, int B, int Tm, int n, int mode, const float *const *rows, int rm_at, const float *sal, int sal_cs, long long sal_bs, StreamState *st,
                      float *rm_f0, float *out);
float *add_f0_hybrid(rvc_engine *e, Plan &pl, int B, int n, int mode, const float *const *rows, int rm_at, const T1 &sal);
// f0 from outside (f0_override.hip.h), each launch as the engine queues it (engine.hip) and as rvc_debug_f0_override does (debug.hip).
// launch_f0_override: out [B][Tm] = the rows f [B][Tm] selected against the overrides `call` describes (cnt [streams], rows [streams][1024]; map: the engine stream of
// each plan stream, or null).  launch_f0_curve_grid: n breakpoints (device) -> grid [Nf].  launch_f0_export: the rows f0 [nw][Tm] of windows w0 .. of one recording onto
// its grid [Nf], through the windowed calls' export kernel on a one-file table (windows.hip.h); returns synchronised
void launch_f0_override(hipStream_t s, int B, int Tm, const float *f, float *out, const F0OvCall *call, const int *cnt, const float *rows, const int *map);
void launch_f0_curve_grid(hipStream_t s, const double *t, const float *hz, int n, float *grid, long long Nf);
void launch_f0_export(hipStream_t s, const float *f0, int Tm, int w0, int nw, int H, int C, float *grid, long long Nf);
T1 build_nsf_source(rvc_engine *e, Plan &pl, int B, float *d_pitchf);
// the head and the tail of the f0 branch and ContentVec's first layer as plan helpers: the builders above call them, and so does rvc_debug_front (debug.hip)
void add_conv0_front(Plan &pl, const ConvW &cw, const float *w_raw, const float *gn_g, const float *gn_b, int kt, int st, const T1 &x, const T1 &y);
void add_mel_frontend(rvc_engine *e, Plan &pl, int B, const float *audio, long long audio_bs, int n, int frame, int Tm, float *mel, const T2 &img, float bn_scale, float bn_shift);
void add_mel_frontend_tables(rvc_engine *e, Plan &pl, int B, const float *audio, long long audio_bs, int n, int frame, int Tm, float *mel, const T2 &img, float bn_scale,
                             float bn_shift, const float *basis, const int *band);      // the same launch on another filterbank (device tables)
void add_pitch_post(Plan &pl, int B, const T1 &sal, int Tm, StreamState *st, const CallParams *cp, float *f0, bool update, long long shift, long long cache_start,
                    long long read_start, int R, float *pitchf, int *pitch, const float *f0_in = nullptr);
// one ConvBlockRes of RMVPE as build_rmvpe queues it (model_rmvpe.hip; rvc_debug_rm_block calls the same three).  add_rm_block_fused: the block as ONE launch of
// rm_block_kernel when it is eligible (false = not taken; dry: eligibility only, nothing queued); add_res_block: that launch, or c1 + shortcut in one launch and c2
// ("pair"), or one launch per convolution ("plain"); add_avgpool2: AvgPool2d(2, 2) of x into p as a launch of its own
bool add_rm_block_fused(Plan &pl, const ResBlockW &w, const T2 &x, const T2 &out, const ResBlockW *next, const T2 *pool_src = nullptr, bool dry = false, const T2 *pool_dst = nullptr);
T2 add_res_block(Plan &pl, const ResBlockW &w, const T2 &x, const T2 &out, const ResBlockW *next = nullptr, const T2 *pool_src = nullptr, const T2 *pool_dst = nullptr);
void add_avgpool2(Plan &pl, const T2 &x, const T2 &p);
void add_nsf_source(Plan &pl, int B, const float *pitchf, const T1 &src, int R, int upp, float sr, float lin_w, float lin_b, const StreamState *st, const CallParams *cp,
                    int f0_num, int f0_den);
std::vector<T1> build_noise_convs(rvc_engine *e, Plan &pl, int B, const T1 &src);
// (a model without pitch guidance, ModelSY::has_f0 false: src, d_pitchf, d_pitch, nz are not looked at and src_join_sid is 0)
void build_synth(rvc_engine *e, Plan &pl, int B, const T1 &phone, const T1 &src, float *d_pitchf, int *d_pitch, int src_join_sid, const std::vector<T1> *nz = nullptr);
void build_retrieval(rvc_engine *e, Plan &pl, int B, int T, int C, uint32_t skip_head, uint32_t R, const T1 &phone);
// consonant protection on `phone` [B][C][R] against the ContentVec output `cv` [B][C][T] (protect_mix_kernel, protect.hip.h): the one launch of the plan op
// (engine.hip get_plan) and of rvc_debug_protect (debug.hip)
void launch_protect_mix(hipStream_t s, int B, const StreamState *st, const float *pitchf, const float *cv, int cv_cs, long long cv_bs, int C, int T, int skip_head, int R,
                        float *phone, int ph_cs, long long ph_bs);
// the caller-side post-processing (chunk.hip.h), the session's ring updates (session.hip.h) and one converter call of every stream (resample.hip.h), each launch
// as rvc_envelop_mixing / rvc_sola_step / rvc_session_process queue it (engine.hip) and as rvc_debug_post does (debug.hip).  B = streams; nf = RMS frames (the tracks are f64)
void launch_post_rms(hipStream_t s, int B, const float *y, int n, int frame, int hop, int nf, double *out, long long y_bs, long long out_bs);
void launch_post_mix(hipStream_t s, int B, float *out, int n, const double *r1, int n1, const double *r2, int n2, float mix_power, long long out_bs, long long r_bs, const float *mix_power_v);
void launch_post_sola_corr(hipStream_t s, int B, const float *output, const float *sola, int sola_len, int search, float *cor, long long out_bs, long long sola_bs, long long cor_bs);
void launch_post_sola(hipStream_t s, int B, float *output, float *sola, int sola_len, int search, int frame, float *frame_out, int *offset_out, const float *cor, long long out_bs,
                      long long sola_bs, long long frame_bs, long long cor_bs, const int *mode_v, int mode_all, float *pv_a, long long pva_bs);
void launch_ring_shift_append(hipStream_t s, int B, const float *in, float *out, int n, int f, const float *chunk);
void launch_ring16_update(hipStream_t s, int B, const float *in, float *out, int n, int f, const float *res, int skip, int copy_begin, long long res_bs);
// a converter of nb streams (rvc_session_create's; released with rvc_resampler_destroy) and its chunk sizes; one call of it queued on the engine's stream
rvc_status resampler_create_streams(rvc_engine *e, size_t rate_in, size_t rate_out, size_t chunk_size_in, int nb, rvc_resampler **out, int *fft_in, int *fft_out);
void launch_resampler(rvc_resampler *r, const float *d_in, float *d_out, long long in_bs, long long out_bs);
void install_index(rvc_engine *e, DevBuf<float> rows, size_t n, size_t dim);      // the one way a matrix becomes the engine's index (contract: retrieval.hip)
void ensure_index_transposed(rvc_engine *e);
// k-means training of an IVF structure (retrieval.hip, kmeans.hip.h): the device buffers of one training and its two steps, as rvc_train_index_ivf runs them and
// as rvc_debug_kmeans_step does (debug.hip).  assign[2]: the current and the previous assignment, swapped per step
struct KmeansWork {
    size_t n = 0, dim = 0, nlist = 0; int nwg = 0, nparts = 0;
    DevBuf<float> cent, dist; DevBuf<int> assign[2], moved_wg, counts, offs, perm;
    DevBuf<double> part, obj; DevBuf<long long> moved;
    DevTimer step; double ms_assign = 0, ms_update = 0;
    const float *rows = nullptr;          // the matrix trained on; null = the engine's loaded index
    void alloc(size_t n, size_t dim, size_t nlist, const float *rows = nullptr);
};
void kmeans_assign_step(rvc_engine *e, KmeansWork &w, const int *prev, int cur, double *objective, long long *moved);
void kmeans_update_step(rvc_engine *e, KmeansWork &w, int cur);
// The index builder (retrieval.hip, index_build.hip.h): the row store of one build and its device-side counters.  index_build_reserve
// grows the store to hold `need` rows (twice its size, or `need` if that is larger; the old allocation is retired until the stream has been synchronised);
// index_build_append queues index_append_kernel + index_compact_kernel for one window's ContentVec output cv [C][ld], T columns used, on the engine's stream.
// rvc_index_build_add runs them per window and so does rvc_debug_index_append (debug.hip).
struct IndexBuild {
    size_t window = 0, dim = 0, capacity = 0;
    size_t rows = 0, windows = 0, dropped = 0;      // as of the last add (the device counters are read once per add)
    DevBuf<float> store;                            // [capacity][dim] fp32
    DevBuf<int> d_cnt;                              // {rows, dropped} on the device
    DevBuf<int> d_bad; size_t bad_cap = 0;          // one word per frame of a window, zero between windows
    std::vector<DevBuf<char>> retired;              // allocations the store outgrew, freed behind the add's synchronisation
    std::vector<DevEvent> ev;                       // timing of an add's run w: 3 w = before its ContentVec run, 3 w + 1 = behind it, 3 w + 2 = behind its append
    double ms[3] = {0, 0, 0};                       // device milliseconds: ContentVec runs, appends, the reduction
    void alloc(size_t dim, size_t capacity);
};
void index_build_reserve(rvc_engine *e, IndexBuild &b, size_t upper, size_t need);
void index_build_append(rvc_engine *e, IndexBuild &b, const float *cv, int C, int T, int ld);
void index_build_abort(rvc_engine *e);
// engine.hip: the one-stream ContentVec-only plan of length L -- rvc_hubert's plan -- whatever rvc_set_streams says, and one run of it on the engine's stream
// over the samples already in pl.d_in; drop_plans: synchronise the device, then forget every cached plan (whoever changes what plans were built on calls it)
void drop_plans(rvc_engine *e);
Plan *hubert_plan(rvc_engine *e, size_t L);
void run_hubert_plan(rvc_engine *e, Plan &pl);
}  // namespace rvc
