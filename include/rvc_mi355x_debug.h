/*
 * rvc_mi355x_debug.h -- TEST HOOKS of librvc_mi355x.so.  Not part of the drop-in boundary (include/rvc_mi355x.h is): these entry
 * points exist so that the parity tests under tests/ and the profiling tools under tests/tools/ can force a code path the planner
 * would not pick for the geometry at hand, or look inside a plan.  A host (the `rvc` crate shim, rvc-rpc) never calls them, and none
 * of them is reachable through the environment.  Apart from rvc_* of the two headers the library exports nothing
 * (obs_rvc_amd/csrc/exports.map).
 */
#ifndef RVC_MI355X_DEBUG_H
#define RVC_MI355X_DEBUG_H
#include "rvc_mi355x.h"
#ifdef __cplusplus
extern "C" {
#endif

/* set (value != NULL) or clear one of the named planner hooks (obs_rvc_amd/csrc/plan.hip, kTestHooks: every one of them selects between
 * kernels / tiles / plan structures that compute the SAME result up to fp32 summation order); 0 = done, -1 = not a hook.  Plans built
 * before a hook changed are dropped. */
int rvc_debug_option(const char *name, const char *value);
/* device timestamps at section boundaries of the last call (hook RVC_STAMPS): "name us" lines; returns the number of stamps */
int rvc_debug_stamps(rvc_engine *e, char *buf, size_t cap);
/* launches (ops) of the last call's plan */
int rvc_debug_last_plan(rvc_engine *e, int *n_ops);
/* the named tap (rvc_enable_taps) of one stream of the last call, as rvc_get_tap returns stream 0's: plans built with taps on snapshot every stream of a
 * tapped tensor.  RVC_SHAPE for a stream the plan did not have (and for streams > 0 of the taps that hold the whole plan in one tensor: "pitchf",
 * "phone_prot", "phone_blend", "cv.out_all"); else as rvc_get_tap */
int rvc_debug_tap(rvc_engine *e, const char *name, int stream, float *out, size_t cap, size_t *n);
/* one line per profiled launch of the last call: "<us> <gflop> <description>" */
int rvc_debug_profile_dump(rvc_engine *e, char *buf, size_t cap);
/* one Conv1d / one Conv2d 3x3 or ConvTranspose2d 3x3 stride 2 / the folded-LayerNorm launch pair on deterministic data through whatever kernel
 * the planner (or a hook) picks, against a double-precision host evaluation: largest |gpu - host| / rms(host); negative on failure */
double rvc_debug_conv_check(rvc_engine *e, int M, int Cin, int KW, int dil, int N, int streams, int pre_act);
double rvc_debug_conv2d_check(rvc_engine *e, int M, int Cin, int H, int W, int streams, int kind, int residual);
double rvc_debug_ln_fold_check(rvc_engine *e, int M, int K, int N, float offset);
/* one convolution layer built with the planner calls and options the models use (prep_conv / prep_convT1d, merge_convs, add_conv1d /
 * add_convT1d / add_conv1d_multi / add_conv1d_two / add_conv2d), run once through whatever kernel the planner (or a hook) picks.
 * Weights and biases come in PyTorch layout (form: layout of w; bias):
 *   0 conv1d        [cout][cin / groups][kw]; [cout]      (glu: cout = 2H rows in model order, tanh half first; the output has H channels)
 *   1 convT1d       [cin][cout][kw]; [cout]               (stride = the upsampling factor, pad = (kw - stride) / 2)
 *   2 conv1d_multi  n blocks [cout][cin][kws[j]]; [n][cout] (phase j = conv j, y has n * cout rows)
 *   3 conv1d_two    two blocks [cout][cin]; [2][cout] (the pair bias); y has 3 cout + 16 rows, the first output at row 16, the second at row 16 + 2 cout
 *   4 conv2d 3x3    [cout][cin][3][3]; [cout]             (t_in = H, t_out = W; y_ws: the image written transposed into a [cout * W][H] 1-D tensor)
 * bias may be NULL (no bias).  x / y / r are the WHOLE allocations of the input, output and residual tensors (guard zones, halos, ld padding,
 * every stream): uploaded before the launch, downloaded after it.  geo[3][8] receives, for x, y, r: allocation size (floats), offset of element
 * (0, 0, 0) from the allocation's start, C, T (2-D: W), ld (row stride), bs (stream stride), cs (channel stride), H (1-D: 1).  With x == NULL only
 * geo is filled.  0 = done, else an rvc_status (rvc_last_error_message).  The plan is built under the engine's rvc_set_gemm_precision setting, as a
 * real plan is: in mode 1 a layer the split-bf16 rule takes runs on igemm_bf3_kernel (rvc_debug_last_kernel: "bf3"). */
typedef struct rvc_debug_layer_spec {
    int form, streams;
    int cin, cout, kw, stride, pad, dil, groups;
    int t_in, t_out, x_halo, y_halo, r_halo;
    int act; float slope; float scale; int accumulate;
    int pre_act; float pre_slope;
    int no_bias, final_out, glu;
    int res;                         /* 0 none; 1 a tensor of its own (multi: n * cout rows if res_grouped); 2 one row shared by every channel and stream (res_cs = res_bs = 0); 3 the output tensor; 4 the input tensor (1-D) */
    int n, kws[4], dils[4], pads[4];
    int x_grouped, res_grouped, y_ws;
} rvc_debug_layer_spec;
int rvc_debug_layer(rvc_engine *e, const rvc_debug_layer_spec *s, const float *w, const float *bias, float *x, float *y, float *r, long long *geo);
/* one transformer / recurrent op built with the helpers the models call (obs_rvc_amd/csrc/plan.hip add_attention, add_relpos_attention, add_layernorm,
 * add_gru, with their rules and forcing hooks) and run `reps` times eagerly, or -- graph != 0 -- captured once and the graph replayed `reps` times.
 * op: tensors x; y, weights w0; w1 in PyTorch layout (hd = E / heads):
 *   0 MHA (ContentVec)     qkv [3E][T] (q, k, v rows); out [E][T]                  -
 *   1 relative MHA (VITS)  qkv [3E][T]; out [E][T]                                 rel_k [2 window + 1][hd]; rel_v [2 window + 1][hd]
 *   2 LayerNorm            x [C][T], normalised in place (y unused)                gamma [C]; beta [C]
 *   3 bidirectional GRU    gi [6H][T]: gate pre-activations, b_ih included         weight_hh_l0 then weight_hh_l0_reverse, [2][3H][H];
 *                          (forward r, z, n, then reverse r, z, n); out [2H][T]    bias_hh_l0 then _reverse, [2][3H]
 * T is the length (R of the synthesizer, Tm of RMVPE).  x / y are the WHOLE allocations, as for rvc_debug_layer; geo[2][8] receives their geometry
 * (x, y) as there.  status (GRU): receives every stream's status word, int[streams] (0 = fine).  With x == NULL only geo is filled.  0 = done, else
 * an rvc_status (rvc_last_error_message); rvc_debug_last_kernel then names the variant ("attn_mfma2_qloop", "relpos_small", "ln_strip12", "gru_multi"). */
typedef struct rvc_debug_op_spec {
    int op, streams;
    int E, heads, T, window, C, H;
    int x_halo, y_halo;
    int reps, graph;
} rvc_debug_op_spec;
int rvc_debug_op(rvc_engine *e, const rvc_debug_op_spec *s, const float *w0, const float *w1, float *x, float *y, int *status, long long *geo);
/* the head and the tail of the f0 branch and ContentVec's first layer, each built with the plan helper the models call (add_mel_frontend, add_conv0_front,
 * add_pitch_post, add_nsf_source: model_rmvpe.hip, model_cv.hip, model_synth.hip) and run once eagerly, or -- graph != 0 -- captured and the graph launched once.
 * op: tensors buf[0..3] (each the WHOLE allocation, uploaded before the launch and downloaded after it; geo[4][8] as for rvc_debug_layer, zeros for an unused
 * slot); weights w0; w1:
 *   4 mel front end   buf0 audio [streams][n] (the last `frame` samples of each stream are analysed; 64 floats of slack behind the last stream, as the
 *                     plan's input buffer has); buf1 log-mel [streams][128][Tm]; buf2 the RMVPE input image [streams][1][Tm + 2][128 + 2] (geo: C = 1,
 *                     T = W = 128, H = Tm), = log-mel * scale + shift.  The engine's own window / twiddle / mel tables are used.
 *   5 conv0           buf0 audio [streams][L] (+ 64); buf1 out [streams][C][To], To = (L - 10) / 5 + 1.  Conv1d(1 -> C, 10 taps, stride 5, no bias) +
 *                     GroupNorm(C groups) + GELU.  w0 = weight [C][10], w1 = gamma [C] then beta [C].  rvc_debug_last_kernel names the path ("conv0_multi4",
 *                     "conv0_multi8", "conv0_one8|16|32", "conv0_generic"); hook RVC_CONV0_KERNEL = multi | one | generic.
 *   6 pitch decode    buf0 salience [streams][360][Tm] (a plan tensor: ld padding, guards); buf1 f0 [streams][Tm]; update != 0: buf2 pitchf [streams][R], buf3 the
 *                     coarse pitch [streams][R] as int32 in the floats' place; the cache moves by `shift`, takes f0[3 .. Tm - 1) from cache_start on, and R values are
 *                     read from read_start on (out-of-range values: RVC_PANIC, as the chunk would).  Threshold 0.03.
 *   7 NSF source      buf0 pitchf [streams][T]; buf1 src [streams][1][T upp] with a halo of x_halo columns per side.  sr, lin_w, lin_b, f0_num / f0_den as given;
 *                     T > 512: RVC_SHAPE.
 * state[streams]: what the kernels read of a stream's state and of the call (uppower, stream_id, chunk, cache) goes in, status and the updated cache come back;
 * seed is the call's noise seed.  With buf == NULL only geo is filled.  0 = done, else an rvc_status (rvc_last_error_message). */
typedef struct rvc_debug_stream_state {
    float uppower; unsigned stream_id, chunk; int status;
    float cache_pitchf[1024];
} rvc_debug_stream_state;
typedef struct rvc_debug_front_spec {
    int op, streams, graph;
    int n, frame;                                    /* 4: samples per stream, analysed samples (frame = 160 (Tm - 1) rounded as the engine does: Tm = 1 + frame / 160) */
    float bn_scale, bn_shift;
    int C, L;                                        /* 5 */
    int Tm, update, shift, cache_start, read_start, R;   /* 6 */
    int T, upp, x_halo, f0_num, f0_den;              /* 7 */
    float sr, lin_w, lin_b;
    unsigned seed;
} rvc_debug_front_spec;
int rvc_debug_front(rvc_engine *e, const rvc_debug_front_spec *s, const float *w0, const float *w1, float *const *buf, rvc_debug_stream_state *state, long long *geo);
/* protect_mix_kernel alone (obs_rvc_amd/csrc/protect.hip.h; DESIGN.md "Consonant protection"), launched as a plan launches it: phone [streams][C][ph_ld]
 * (R rows used; uploaded, mixed in place, downloaded whole: the padding comes back as it went in), cv [streams][C][cv_ld] (T columns used: the ContentVec
 * output, channel-major), pitchf [streams][R], protect [streams] in [0, 0.5] (stored as float, as rvc_set_protect_stream stores it).  Needs ph_ld >= R,
 * cv_ld >= T and skip_head + R <= 2 T + 1 (RVC_SHAPE otherwise).  graph != 0: captured and the graph launched once.  0 = done, else an rvc_status. */
typedef struct rvc_debug_protect_spec {
    int streams, C, R, T, skip_head, ph_ld, cv_ld, graph;
} rvc_debug_protect_spec;
int rvc_debug_protect(rvc_engine *e, const rvc_debug_protect_spec *s, float *phone, const float *cv, const float *pitchf, const double *protect);
/* crepe_decode_kernel alone (obs_rvc_amd/csrc/crepe.hip.h; DESIGN.md "CREPE pitch"), launched as a CREPE plan launches it, on the caller's posteriors prob
 * [B][Tm][360]: decoder 0 = Viterbi, 1 = arg-max.  f0_out [B][Tm] is what the plan hands to the pitch tail (Hz, filtered, 0 = unvoiced); bins_out [B][Tm] the
 * decoded path and pd_out [B][Tm] its periodicity prob[t][bin[t]] before the median filter (either may be NULL).  Needs no weights.  B in [1, 64], Tm in
 * [2, 1024] (RVC_SHAPE otherwise).  0 = done, else an rvc_status. */
int rvc_debug_crepe_decode(rvc_engine *e, const float *prob, int B, int Tm, int decoder, float *f0_out, int *bins_out, float *pd_out);
/* fcpe_decode_kernel alone (obs_rvc_amd/csrc/fcpe.hip.h; DESIGN.md "FCPE pitch"), launched as an FCPE plan launches it but on the caller's posteriors prob
 * [B][Tm][360] (no sigmoid), under the engine's threshold (rvc_set_fcpe_threshold).  f0_out [B][Tm] is what the plan hands to the pitch tail (Hz, 0 = unvoiced);
 * bins_out [B][Tm] the arg-max bins (may be NULL).  Needs no weights.  B in [1, 64], Tm in [1, 1024] (RVC_SHAPE otherwise).  0 = done, else an rvc_status. */
int rvc_debug_fcpe_decode(rvc_engine *e, const float *prob, int B, int Tm, float *f0_out, int *bins_out);
/* fcpe_glu_dw_silu_kernel alone, launched as an FCPE plan launches it, on contiguous arrays: z [B][2 I][T] (value rows, then gate rows), w [I][31], bias [I]
 * -> y_out [B][I][T] = silu(bias + depthwise31(z[:I] * sigmoid(z[I:])), zero padding 15).  B in [1, 64], I and T in [1, 4096].  0 = done, else an rvc_status. */
int rvc_debug_fcpe_dw(rvc_engine *e, const float *z, const float *w, const float *bias, int B, int I, int T, float *y_out);
/* f0_hybrid_kernel alone (obs_rvc_amd/csrc/f0_hybrid.hip.h; DESIGN.md "Hybrid f0"), launched as a hybrid plan launches it, on the caller's member rows
 * rows [n][B][Tm] (Hz, lead first; mode RVC_HYBRID_VOTE / RVC_HYBRID_MEDIAN) -> out [B][Tm], the row a plan hands to the pitch tail.  sal (may be NULL): a salience
 * [B][360][Tm] that the launch decodes as RMVPE's in place of member rm_at (rows[rm_at] is then not read; rm_f0_out [B][Tm], may be NULL, gets the decoded row);
 * with sal NULL rm_at must be -1.  ms_out (may be NULL): the launch's time between two HIP events.  Reads no weights and no state but the status word of streams
 * 0 .. B - 1 (a decode that runs off the salience raises ST_PANIC there, as in a plan).  n in [1, 4], B in [1, the engine's streams], Tm in [1, 1024] (RVC_SHAPE
 * otherwise).  0 = done, else an rvc_status. */
int rvc_debug_f0_hybrid(rvc_engine *e, const float *rows, int n, int B, int Tm, int mode, const float *sal, int rm_at, float *out, float *rm_f0_out, float *ms_out);
/* The kernels of the PM f0 method alone (obs_rvc_amd/csrc/pm.hip.h; DESIGN.md "PM pitch"), launched as a PM plan launches them.  Candidate arrays: cand_n [B][Tm]
 * (0 .. 14 voiced candidates), cand_f / cand_s / cand_delta [B][Tm][15] (frequency in Hz, strength, local score; entry 0 is the unvoiced candidate, 1 .. n the
 * voiced ones in ascending lag).
 *   (a) audio != NULL: pm_peak_kernel + pm_cand_kernel on audio [B][n], whose last `frame` samples are the f0 window (Tm = 1 + frame / 160); the candidate arrays
 *       are written.  With path_out and f0_out given the path kernel runs on them as well.
 *   (b) audio == NULL: pm_path_kernel on the caller's cand_n / cand_f / cand_delta (cand_s may be NULL; n and frame are not looked at); path_out [B][Tm] takes the
 *       chosen candidate of every frame and f0_out [B][Tm] its frequency (0 = unvoiced).
 * B in [1, 64], Tm in [1, 1024]. */
int rvc_debug_pm(rvc_engine *e, const float *audio, int B, int n, int frame, int Tm, int *cand_n, float *cand_f, float *cand_s, float *cand_delta, int *path_out, float *f0_out);
/* The kernels of "f0 from outside" alone (obs_rvc_amd/csrc/f0_override.hip.h; DESIGN.md "f0 from outside"), through the launches the engine uses.  geo is
 * {Nf, w0, nw, H, C}: grid frames, the window of stream 0, real windows of the batch, hop and context in frames.
 *   op 0  select against row buffers: rows [B][Tm], ov [B][1024] (stream b's ov_n[b] rows from its entry 0 on, aligned to the END of the window), out [B][Tm]
 *   op 1  select against a conversion's grid: rows [B][Tm], ov = the grid [Nf], geo; stream b is window w0 + b (b < nw), its row t grid row (w0 + b) H - C + t
 *   op 2  f0_curve_grid_kernel: t [n_bp] seconds, ov = hz [n_bp], geo[0] = Nf, out [Nf]
 *   op 3  f0_export_many_kernel, the f0 export of every conversion, on a one-file table as rvc_convert runs it: rows = the window rows [B][Tm] (B = nw windows
 *         from w0 on), geo, out [Nf] -- read first, so frames the launch does not write keep the caller's value
 * B in [1, 64], Tm in [1, 1024], Nf in [1, 2^24]; everything is checked on the host before a launch. */
int rvc_debug_f0_override(rvc_engine *e, int op, const float *rows, int B, int Tm, const float *ov, const int *ov_n, const long long *geo, const double *t, int n_bp, float *out);
/* the caller-side post-processing, the session's ring updates and a converter of several streams (obs_rvc_amd/csrc/chunk.hip.h, session.hip.h, resample.hip.h;
 * DESIGN.md "Post-processing and resamplers: what is tested"), each launch queued as rvc_session_process queues it, on the caller's arrays with the caller's
 * stream strides.  op: buffers buf[0..3] (each the WHOLE allocation, [streams][stride] floats, uploaded before the launches and downloaded after them: the
 * padding comes back as it went in):
 *   0 envelope mixing   buf0 input [in_bs] (n used); buf1 model output [out_bs] (n used, mixed in place); buf2 [r_bs]: the RMS track of the input (nf values) and,
 *                       from nf on, that of the output, nf = (n + 2 (frame / 2) - frame) / hop + 1; mix_power [streams]: the exponent 1 - mix_rate per stream.  (The tracks are f64 on the device: buf2 is widened going up and rounded to float coming back.)
 *   1 SOLA step, linear buf0 output [out_bs] (search + frame + sola_len used; blended in place); buf1 the saved tail [sola_bs] (sola_len; replaced); buf2 the
 *                       frame [frame_bs]; buf3 the search + 1 normalised correlations [cor_bs]; offsets [streams]
 *   2 ring_shift_append buf0 ring in [n]; buf1 ring out [n]; buf2 chunk [f]                       (contiguous: the kernel takes no strides)
 *   3 ring16_update     buf0 ring in [n]; buf1 ring out [n]; buf2 the converter's output [x_bs]   (rings contiguous); skip, copy_begin as the session passes them
 *   4 converter         a converter of `streams` streams for (rate_in, rate_out, chunk), `chunks` calls, destroyed before the hook returns:
 *                       buf0 [chunks][streams][x_bs] (input_frames_next used), buf1 [chunks][streams][out_bs] (output_frames_max written)
 * graph != 0: the launches are captured and the graph launched once.  RVC_SHAPE for a stride smaller than the row it strides over, search > 1023 and sizes
 * out of range; nothing is queued then.  0 = done, else an rvc_status (rvc_last_error_message). */
typedef struct rvc_debug_post_spec {
    int op, streams, graph;
    int n, frame, hop;                       /* 0 (n: samples); 1: frame; 2, 3: n = ring length */
    int sola_len, search;                    /* 1 */
    int f, skip, copy_begin;                 /* 2, 3 */
    int rate_in, rate_out, chunk, chunks;    /* 4 */
    long long in_bs, out_bs, r_bs, sola_bs, frame_bs, cor_bs, x_bs;
} rvc_debug_post_spec;
int rvc_debug_post(rvc_engine *e, const rvc_debug_post_spec *s, float *const *buf, const float *mix_power, int *offsets);
/* one ConvBlockRes of RMVPE (conv3x3 + ReLU, conv3x3 + ReLU, + 1x1 shortcut or the input) queued as build_rmvpe queues it (obs_rvc_amd/csrc/model_rmvpe.hip:
 * make_res_block, add_rm_block_fused, add_res_block, add_avgpool2) and run `reps` times eagerly, or -- graph != 0 -- captured once and the graph replayed `reps`
 * times.  Weights in PyTorch layout: w1 [cout][cin][3][3], w2 [cout][cout][3][3], wsc [cout][cin] or NULL (identity shortcut: cin = cout), biases [cout].
 *   pool_in   x is [cin][2 H][2 W] and the block sees its AvgPool2d(2, 2): staged by the fused block itself when a dry run says so (hook RVC_RM_FUSE = 3: never),
 *             else a pooling launch into a tensor of the aid's own in front of the block
 *   pool_out  p [cout][H / 2][W / 2] = AvgPool2d(2, 2) of the result: a second output of the fused block when a dry run says so, else a pooling launch behind it
 *   y_in_cat  y has 2 cout channels and the block writes channels [cout, 2 cout) (where an encoder level's last block writes)
 *   next      1: the launch is given a second block's panels to warm (the fused kernel's extra workgroup)
 *   rm_fuse   Plan::rm_fuse (build_rmvpe: the f0 branch has its own partition and there are at most four streams); hook RVC_RM_FUSE applies on top
 * x / y / p are the WHOLE allocations, as for rvc_debug_layer (p may be NULL without pool_out); geo[3][8] receives their geometry (x, y, p) as there, zeros for
 * an unused p.  With x == NULL only geo is filled.  0 = done, else an rvc_status (rvc_last_error_message); rvc_debug_last_kernel then names what ran: "rmb_1_3_2" /
 * "rmb_2_2_1" (rm_block_kernel<MT, NT1, NT2>, + "+pool_in" / "+pool_out" for a pooling folded into it), "pair" (c1 + shortcut in one launch, then c2) or "plain". */
typedef struct rvc_debug_rm_block_spec {
    int streams, cin, cout, H, W;
    int pool_in, pool_out, y_in_cat, next, rm_fuse;
    int graph, reps;
} rvc_debug_rm_block_spec;
int rvc_debug_rm_block(rvc_engine *e, const rvc_debug_rm_block_spec *s, const float *w1, const float *b1, const float *w2, const float *b2, const float *wsc,
                       const float *bsc, float *x, float *y, float *p, long long *geo);
/* the retrieval section of an infer plan alone (obs_rvc_amd/csrc/retrieval.hip build_retrieval; DESIGN.md "Retrieval: what is tested") on an engine that has an
 * index loaded (rvc_load_index on a bare rvc_create engine is enough): cv [streams][C][cv_ld], the ContentVec output in channel-major layout with T columns
 * used; phone [streams][C][ph_ld], R columns written; idx / dist [streams][R][k], k = rvc_index_k (the plan the aid builds carries it, as it carries nprobe); overflow [streams], the many-stream path's flag word per stream (zeros on the
 * other paths).  cv and phone are uploaded, the ops run `reps` times eagerly, or -- graph != 0 -- captured once and the graph replayed `reps` times, and both come
 * back whole: the padding as it went in.  path 0: the planner's choice; 1: the plan's row-major exhaustive list (what a chunk runs after a hand-off time-out;
 * RVC_SHAPE when the plan has none).  The other paths are forced with the hooks RVC_KNN_EXHAUSTIVE and RVC_KNN_NO_GEMM, the one-launch form's grid with
 * RVC_KNN_WGS; rvc_debug_last_kernel then names what was queued: "knn_fused", "knn_gemm", "knn_exhaustive" or "knn_fallback".  Needs ph_ld >= R, cv_ld >= T,
 * skip_head + R <= 2 T + 1, C = the index dimension, rate in [0, 1] (RVC_SHAPE otherwise).  RVC_BACKEND when a stream's status word was raised or the one-launch
 * form left its ticket words non-zero.  0 = done, else an rvc_status. */
typedef struct rvc_debug_retrieval_spec {
    int streams, C, T, cv_ld, skip_head, R, ph_ld;
    float rate;
    int path, reps, graph;
} rvc_debug_retrieval_spec;
int rvc_debug_retrieval(rvc_engine *e, const rvc_debug_retrieval_spec *s, float *cv, float *phone, int *idx, float *dist, int *overflow);
/* the device-side copies of the loaded index besides the row-major matrix: bit 0 = MFMA-fragment order, bit 1 = the transposed copy (built by the first plan that
 * needs it; while it is absent, the exhaustive scan of a fallback list walks the row-major matrix), bit 2 = an IVF structure is attached; 0 without an index */
int rvc_debug_index_layouts(rvc_engine *e);
/* one assign step and one update step of the k-means training (obs_rvc_amd/csrc/kmeans.hip.h) on the loaded index, from the caller's
 * centroids [nlist][dim]: assign_out / dist_out [n] and objective_out are the assign step's, moved_out its rows whose list differs from prev_assign_or_null (all n
 * when that is null), centroids_out [nlist][dim] the update step's means over assign_out.  Nothing is attached and the engine's structure stays.  RVC_SHAPE
 * without an index or with nlist outside [1, min(n, 65536)].  0 = done, else an rvc_status. */
int rvc_debug_kmeans_step(rvc_engine *e, const float *centroids_in, size_t nlist, const int32_t *prev_assign_or_null, int32_t *assign_out, float *dist_out,
                          float *centroids_out, double *objective_out, long long *moved_out);
/* one append of the index builder (obs_rvc_amd/csrc/index_build.hip.h) on a store of its own: cv [C][ld] is a window's ContentVec output
 * in channel-major layout with T columns used; the store starts with `capacity` rows of room and `cursor` rows in it (head_rows [cursor][C], may be null when
 * cursor is 0).  The aid reserves room for cursor + T rows as rvc_index_build_add does (so a capacity below that grows the store), runs index_append_kernel and
 * index_compact_kernel, and returns the store's rows [*rows_out][C] in store_out (cap_rows >= cursor + T), the row count and the rows dropped for a NaN or an
 * Inf.  The engine's own build, if one is open, is not touched.  0 = done, else an rvc_status. */
int rvc_debug_index_append(rvc_engine *e, const float *cv, int C, int T, int ld, size_t cursor, size_t capacity, const float *head_rows, float *store_out,
                           size_t cap_rows, size_t *rows_out, size_t *dropped_out);
/* run-time speaker selection (obs_rvc_amd/csrc/speaker.hip.h), read only: the live speaker-conditioned biases of the loaded synthesizer in
 * model row order -- flow 0 in-layer 0 [2 hidden], flow 0 in-layer 1, ..., the last flow's last in-layer, dec_pre [up_init]; the in-layers un-packed from their
 * GLU row order.  composed = 0: the plain in-layers' buffers; 1: the composed twins' (RVC_SHAPE while the flows are not composed); dec_pre is the same buffer
 * either way.  *n = the count, flow_n wn_layers 2 hidden + up_init; RVC_SHAPE when cap is smaller.  Synchronises the device.  0 = done, else an rvc_status. */
int rvc_debug_speaker_biases(rvc_engine *e, int composed, float *out, size_t cap, size_t *n);
/* milliseconds of the last speaker_fold_kernel launch that was queued while rvc_set_profile was on (HIP events around the launch alone); -1 before one.
 * Synchronises the device. */
float rvc_debug_speaker_fold_ms(rvc_engine *e);
/* the autotuner's decisions of this process, one line each ("<layer signature> -> [choice] <kernel description> | <us> (<candidates>)"); returns the number of
 * entries.  reset forgets them (the next plan build measures again). */
int rvc_debug_autotune_dump(char *buf, size_t cap);
void rvc_debug_autotune_reset(void);
/* weight slabs alive on a device: count and bytes (obs_rvc_amd/csrc/plan.hip, wmalloc) */
int rvc_debug_weight_slabs(int device, int *count, size_t *bytes);
/* the kernel the planner chose for this thread's last rvc_debug_conv*_check / rvc_debug_layer launch ("reg", "g32", "c32s", ...), or the variant of
 * its last rvc_debug_op */
const char *rvc_debug_last_kernel(void);
/* the whole description of this thread's last implicit-GEMM launch queued, as rvc_debug_profile_dump prints it ("reg M=20 N=37 K=16384 ... split=2": split > 1
 * is the two-stage grid-level split-K, partial sums finished by splitk_epilogue_kernel) */
const char *rvc_debug_last_desc(void);
/* host only: the formant resampler's full filter table h[n][K] (o -> n, K = 2 w + o; obs_rvc_amd/csrc/formant.hip.h) as fp32.  *width = K;
 * returns 0, 1 when cap < n K (nothing written to out), -1 for bad arguments */
int rvc_debug_formant_table(size_t o, size_t n, float *out, size_t cap, size_t *width);
/* enable != 0: every later rvc_session_process records HIP events around its SOLA stage (offset search, blend, tail save; with the phase-vocoder
 * crossfade its analysis and synthesis launches); returns the milliseconds of the last chunk processed with the events on (0 before one) */
float rvc_debug_session_sola_ms(rvc_session *s, int enable);
/* the same around the session's two noise-reduction stages (rvc_session_set_noise_reduction): the milliseconds of both sides added, of the last chunk
 * processed with the events on while a side was in use (0 before one) */
float rvc_debug_session_denoise_ms(rvc_session *s, int enable);

#ifdef __cplusplus
}
#endif
#endif
