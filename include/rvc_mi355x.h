/*
 * rvc_mi355x.h -- C ABI of the MI355X-native RVC streaming inference engine.
 *
 * Drop-in boundary for the `rvc` crate of RVC-Project/obs-rvc: every entry point below
 * replaces one method of `rvc::RvcInfer` (reference: rvc/src/rvc.rs:30-220) or one
 * variant of `rvc_common::errors::RvcInferError` (rvc-common/src/errors.rs:2-8).  Plain
 * pointers and sizes only; one handle = one engine bound to one GPU; a handle is NOT
 * re-entrant (the reference methods take `&mut self`, rvc.rs:133-134).
 *
 * Reference method                                  -> C entry point
 *   RvcInfer::new(data_path)            rvc.rs:30-44   rvc_create
 *   (Drop)                                             rvc_destroy
 *   load_contentvec(RvcModelVersion)    rvc.rs:46-54   rvc_load_contentvec
 *   load_model(model_path)              rvc.rs:56-60   rvc_load_model
 *   load_f0(PitchAlgorithm)             rvc.rs:62-75   rvc_load_f0
 *   unload_model()                      rvc.rs:77-79   rvc_unload_model
 *   hubert(input) -> (1,C,T)            rvc.rs:81-97   rvc_hubert
 *   extract_feature(input) -> (1,2T+1,C) rvc.rs:99-109 rvc_extract_feature
 *   pitch(input, shift, frame) -> f0    rvc.rs:111-131 rvc_pitch
 *   infer(input, frame, shift, skip_head, return_length) rvc.rs:133-220  rvc_infer
 *
 * File naming follows rvc/src/models.rs:58-61,72 with the native extension:
 *   <data>/contentvec/vec-{256,768}-layer-{9,12}.rvcw, <data>/f0/rmvpe.rvcw, <model>.rvcw
 * (a path ending in ".onnx" is mapped to its ".rvcw" sibling).
 */
#ifndef RVC_MI355X_H
#define RVC_MI355X_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* RvcInferError (rvc-common/src/errors.rs:2-8) + RVC_PANIC for inputs on which the reference
 * panics instead of returning an error (e.g. rmvpe.rs:124 out-of-bounds gather). */
typedef enum {
    RVC_OK = 0,
    RVC_MODEL_NOT_LOADED = 1,
    RVC_CONTENTVEC_NOT_LOADED = 2,
    RVC_F0_NOT_LOADED = 3,
    RVC_BACKEND = 4,          /* Ort(..) in the reference: load / device / kernel failure */
    RVC_SHAPE = 5,            /* NdarrayShapeError(..): bad sizes, output buffer too small */
    RVC_PANIC = 6
} rvc_status;

/* RvcModelVersion / PitchAlgorithm as the i64 conversions of rvc-common/src/enums.rs:32-48,96-110 */
#define RVC_VERSION_V1 1
#define RVC_VERSION_V2 2
#define RVC_PITCH_RMVPE 1

typedef struct rvc_engine rvc_engine;

/* Process environment: when the library is loaded it plants GPU_MAX_HW_QUEUES=16 unless the variable is already set (the HIP runtime
 * maps a process's streams onto 4 hardware queues by default; the engine runs 4 streams per chunk, and a second engine or an RCCL
 * communicator in the same process would share queues with them: +5-20 % per-chunk latency).  The runtime reads
 * the variable when IT initialises, so load this library before the first HIP call or set the variable yourself; set
 * RVC_NO_RUNTIME_DEFAULTS=1 to have the library leave the environment alone. */

/* RvcInfer::new.  device = HIP device ordinal (-1: current / LOCAL_RANK default 0). */
rvc_status rvc_create(const char *data_path, int device, rvc_engine **out);
void rvc_destroy(rvc_engine *e);
rvc_status rvc_load_contentvec(rvc_engine *e, int model_version);
rvc_status rvc_load_model(rvc_engine *e, const char *model_path);
rvc_status rvc_load_f0(rvc_engine *e, int pitch_algorithm);
void rvc_unload_model(rvc_engine *e);

/* Caller-owned buffers.  On RVC_SHAPE the required element count is still written to dims / out_len. */
rvc_status rvc_hubert(rvc_engine *e, const float *input, size_t n, float *out, size_t cap, size_t dims[3]);
rvc_status rvc_extract_feature(rvc_engine *e, const float *input, size_t n, float *out, size_t cap, size_t dims[3]);
rvc_status rvc_pitch(rvc_engine *e, const float *input, size_t n, int32_t pitch_shift, size_t sample_frame_16k_size,
                     float *out, size_t cap, size_t *out_len);
/* has_pitch_shift = 0 mirrors Option::None (rvc.rs:163) */
rvc_status rvc_infer(rvc_engine *e, const float *input, size_t n, size_t sample_frame_16k_size, int has_pitch_shift,
                     int32_t pitch_shift, uint32_t skip_head, uint32_t return_length, float *out, size_t cap, size_t *out_len);
const char *rvc_last_error_message(rvc_engine *e);

/* ---- f0 methods: RMVPE (the reference's only one), or YIN, a time-domain tracker that needs no weight file ---- */
/* rvc_load_f0 keeps the reference's one-variant PitchAlgorithm (every value loads RMVPE); the engine's method is chosen here by constants of
 * its own.  YIN (de Cheveigne & Kawahara 2002; DESIGN.md "YIN pitch") reads the frames RMVPE's front end reads -- the same number of f0 rows
 * with the same meaning -- in one kernel, needs no <data>/f0/rmvpe.rvcw, and feeds the same pitch shift, pitch cache and get_f0_post; 0 Hz =
 * unvoiced.  The method is engine-wide (not per stream), may be changed between calls, and is part of a plan's identity. */
#define RVC_F0_RMVPE 1
#define RVC_F0_YIN   2     /* weight-free; DESIGN.md "YIN pitch" */
/* CREPE (Kim et al. 2018; DESIGN.md "CREPE pitch"): the six-layer 1-D conv net on the same frame grid, decoded as upstream decodes it -- Viterbi over the 360
 * bins -- and fed to the same pitch tail.  Full (capacity 32) reads <data>/f0/crepe-full.rvcw, tiny (capacity 4) <data>/f0/crepe-tiny.rvcw
 * (python -m obs_rvc_amd.importers crepe writes them); a missing file gives what a missing rmvpe.rvcw gives (RVC_BACKEND) and leaves the method as it was.
 * A preset is read once per engine: going back to it reads no file and finds its plans.  The value 3 is not a method: it stays the unknown value it was.
 * Limits: every frame of every stream is in flight at once, so streams x frames of the f0 window may not exceed 65535 (RVC_SHAPE beyond), and a plan holds
 * about 1.9 MB of activations per frame at full capacity (0.24 MB tiny): 60 MB at the 32 frames of a 160 ms chunk, 2 GB per stream at 1024 frames. */
#define RVC_F0_CREPE      4
#define RVC_F0_CREPE_TINY 5
/* FCPE (torchfcpe's CFNaiveMelPE, convolutions only; DESIGN.md "FCPE pitch"): a light network tracker on the same frame grid -- 128 Slaney mels, an input stack,
 * N blocks of LayerNorm -> pointwise -> GLU -> depthwise 31 -> SiLU -> pointwise with a residual, 360 posteriors per frame -- decoded by upstream's
 * local_argmax (the arg-max bin and its four neighbours either side) and fed to the same pitch tail.  Reads <data>/f0/fcpe.rvcw once per engine
 * (python -m obs_rvc_amd.importers fcpe writes it; the sizes come from the blob); a missing file gives what a missing rmvpe.rvcw gives (RVC_BACKEND) and leaves
 * the method as it was.  The values 3 and 6 are not methods. */
#define RVC_F0_FCPE       7
/* PM (upstream's f0_method "pm": Praat's to_pitch_ac, Boersma 1993; DESIGN.md "PM pitch"): the second weight-free tracker, on YIN's frames.  Per frame the
 * autocorrelation of the Hanning-windowed 60 ms window divided by the window's own, up to 14 interpolated peak candidates and an unvoiced one; one Viterbi path
 * through the candidates of the whole f0 window under Praat's octave-jump and voiced / unvoiced transition costs, so a frame is decided with its neighbours and
 * not alone as YIN decides it.  Floor 50 Hz, ceiling 1100 Hz, voicing threshold 0.6 (upstream's call), Praat's defaults otherwise; no setter.  Needs no file. */
#define RVC_F0_PM         9
rvc_status rvc_load_f0_method(rvc_engine *e, int method);   /* RMVPE: same as rvc_load_f0; YIN, PM: need no file; CREPE, CREPE_TINY, FCPE: see above; other values: RVC_SHAPE */
int rvc_f0_method(rvc_engine *e);                           /* 0 = none loaded */
/* CREPE's decoder: 0 = Viterbi (the default, upstream's), 1 = arg-max (the same decoder without the transition term).  Engine-wide, may be changed between
 * calls, part of a CREPE plan's identity; other values: RVC_SHAPE. */
#define RVC_CREPE_VITERBI 0
#define RVC_CREPE_ARGMAX  1
rvc_status rvc_set_crepe_decoder(rvc_engine *e, int decoder);
int rvc_crepe_decoder(rvc_engine *e);
/* FCPE's voicing threshold: f0 = 0 on a frame whose largest posterior is at or below it.  Default 0.006 (what upstream's real-time client passes).  Engine-wide,
 * may be changed between calls and holds from the next call on (part of an FCPE plan's identity); values outside [0, 1) and NaN: RVC_SHAPE. */
rvc_status rvc_set_fcpe_threshold(rvc_engine *e, double threshold);
double rvc_fcpe_threshold(rvc_engine *e);
/* Hybrid f0 (the forks' `hybrid[rmvpe+fcpe]`; DESIGN.md "Hybrid f0"): 1 to 4 distinct members out of the six methods above run on the same audio, one after
 * another on the f0 branch, and their unshifted f0 rows are combined per stream and frame; the combined row takes the pitch tail every method takes (shift, pitch
 * controls, cache, get_f0_post).  methods[0] is the LEAD.  A member is voiced on a frame iff its value is > 0.  With n members of which v are voiced:
 *   RVC_HYBRID_VOTE   (the default of the front ends) voiced iff 2 v > n, or 2 v == n and the lead is voiced; an unvoiced frame gives 0, a voiced one the median
 *                     of the v voiced values
 *   RVC_HYBRID_MEDIAN the median of all n values, unvoiced ones entering as 0: the forks' plain median, kept for parity -- it halves f0 where two members
 *                     disagree on voicing, which is why it is not the default
 * (median of an even count: 0.5f * (a + b) of the two middle values).  A hybrid of one member is that method, bit for bit.  Each member keeps its engine-wide
 * settings (rvc_set_crepe_decoder, rvc_set_fcpe_threshold, RMVPE's 0.03) and its own limits and refusals (CREPE: streams x frames <= 65535).
 * rvc_load_f0_hybrid loads every member as rvc_load_f0_method would (same files, read once and kept where that holds) and makes the hybrid the engine's method:
 * rvc_f0_method then returns RVC_F0_HYBRID; rvc_load_f0_method / rvc_load_f0 go back to a single method.  All or nothing: a member's missing file (RVC_BACKEND),
 * n outside 1..4, a repeated member, a value that is no single method, a mode other than 0 / 1 (RVC_SHAPE with a message) leave the method, the members and the
 * loaded weights as they were.  rvc_load_f0_method(e, RVC_F0_HYBRID) is RVC_SHAPE: it names no members.  Engine-wide, part of a plan's identity (the ordered
 * members and the mode).  rvc_f0_hybrid writes the members in order (at most cap) and the mode (either pointer may be null) and returns n, 0 when the
 * method is no hybrid. */
#define RVC_F0_HYBRID 8
#define RVC_HYBRID_VOTE   0
#define RVC_HYBRID_MEDIAN 1
rvc_status rvc_load_f0_hybrid(rvc_engine *e, const int *methods, int n, int mode);
int rvc_f0_hybrid(rvc_engine *e, int *methods, int cap, int *mode);
/* Models trained without pitch guidance (upstream's SynthesizerTrnMs{256,768}NSFsid_nono, `f0: 0` in the checkpoint; blob config key f0 = 0; DESIGN.md
 * section 22): 1 = the loaded model has pitch guidance, 0 = it has none, -1 = no model loaded.  On a no-f0 model no call of the infer family (rvc_infer*,
 * rvc_session_process, rvc_convert*, rvc_convert_file*) needs an f0 method or runs one that is loaded: pitch_shift / has_pitch_shift, the pitch controls
 * (rvc_set_pitch_semitones, _f0_range, _f0_median, _f0_snap), rvc_set_protect, the f0 method and the CREPE decoder are ignored and no part of a plan's identity,
 * the pitch cache is not written, the chunk counter advances.  Formant shift, the index, graph replay and every other setting apply; chunk pipelining
 * (rvc_set_pipeline) has no front pair to overlap there: an infer call with it on returns RVC_SHAPE with a message.  rvc_pitch is the tracker's and unchanged. */
int rvc_model_has_f0(rvc_engine *e);
/* Speakers of a multi-speaker voice model, selected and blended at run time (upstream's `sid` of every vc_single call and `n_spk` of get_vc; DESIGN.md
 * section 24).  A synthesizer blob may carry the speaker table sy.emb_g [n_spk][gin] (python -m obs_rvc_amd.importers synth ... --speakers all|N); one without
 * has the one speaker 0, the row baked into it.  The setting is engine-wide (every stream), is the loaded model's (rvc_load_model / rvc_unload_model put it back
 * to the blob's baked speaker) and may change between any two chunks: a set call only records the mix, the next chunk queues one small launch on the engine's
 * stream in front of its synthesizer that rewrites the speaker-conditioned biases in place -- no host synchronisation, no plan rebuilt, no plan key changed;
 * unsynchronised (sync = 0), pipelined and graph-replayed chunks see it in order.  Until the first set call nothing differs from a baked blob, bit for bit.
 *   rvc_model_speakers   rows of the table; 1 without one; 0 = no model loaded
 *   rvc_set_speaker      the speaker by id
 *   rvc_set_speaker_mix  g = sum_i weight[i] emb_g[sid[i]] over 1 <= n <= 8 distinct ids; weights >= 0, finite, not all zero, normalised to sum 1 in double
 *   rvc_speaker_mix      the mix in force (normalised weights); *n = its length, RVC_SHAPE when cap is smaller (nothing written but *n)
 * RVC_SHAPE (state unchanged): an id outside [0, n_spk), n = 0 or n > 8, a repeated id, a negative or non-finite weight, a weight sum of 0.
 * RVC_MODEL_NOT_LOADED without a model.  On a blob without a table rvc_set_speaker(e, 0) succeeds, launches nothing and leaves the output bit for bit. */
int rvc_model_speakers(rvc_engine *e);
rvc_status rvc_set_speaker(rvc_engine *e, int sid);
rvc_status rvc_set_speaker_mix(rvc_engine *e, const int32_t *sid, const double *weight, size_t n);
rvc_status rvc_speaker_mix(rvc_engine *e, int32_t *sid, double *weight, size_t cap, size_t *n);

/* ---- capabilities the reference plumbs through but never implements / bakes into its export ---- */
/* flat-L2 retrieval index (index_path / index_rate settings, obs-rvc/src/lib.rs:78,81; rvc.rs:159 TODO).  A load that fails behind its argument checks
   (RVC_BACKEND: no device memory, a failed copy) leaves the engine with no index at all -- rvc_index_device_ptr returns NULL, k and the index rate are kept. */
rvc_status rvc_load_index(rvc_engine *e, const float *vectors, size_t n, size_t dim);
rvc_status rvc_load_index_device(rvc_engine *e, const void *d_vectors, size_t n, size_t dim);  /* already in HBM (RCCL-broadcast) */
void rvc_set_index_rate(rvc_engine *e, float rate);
/* kNN hits of the last infer: idx[rows][k], squared distances [rows][k], k = the rvc_index_k the last plan was built with (4 unless rvc_set_index_k changed it:
   size the arrays for cap_rows * rvc_index_k(e) entries); rows = return_length for stream 0, followed (stream-major) by the rows of as many
   further streams of a batched call as cap_rows holds whole.  After rvc_infer_batch_g (streams bucketed by geometry) no rows are reported: *rows = 0. */
rvc_status rvc_get_knn(rvc_engine *e, int32_t *idx, float *dist, size_t cap_rows, size_t *rows);
/* Neighbours blended per query: 4 (the default) or 8, what every upstream RVC pipeline searches its index with.  The hits are the k
   smallest by (exact fp32 distance, row number), the weights (1/d)^2 normalised over the k; the first four of the eight are the k = 4 hits.  Engine-wide, part of
   a plan's identity, and a preference of the caller rather than a property of the index: it may be set before or after an index is loaded and survives
   rvc_load_index*, rvc_index_broadcast, rvc_set_index_ivf and rvc_train_index_ivf.  The index needs at least k rows.  RVC_SHAPE: k other than 4 or 8; k = 8 on
   a loaded index of fewer than 8 rows (and loading or broadcasting an index of fewer than k rows: the engine keeps what it had). */
rvc_status rvc_set_index_k(rvc_engine *e, int k);
int rvc_index_k(rvc_engine *e);                               /* 4 on a fresh engine */
/* The one-launch retrieval (up to 11 streams) hands its partial lists from workgroup to workgroup inside the launch; if a workgroup does not arrive
   in time (a GPU shared with another process), the engine recomputes that chunk's retrieval through the exhaustive scan and the rest of the chunk,
   and the call still returns RVC_OK with the same hits.  This counts such chunks (0 on a GPU of one's own).  Unsynchronised calls (sync = 0) cannot
   be recomputed in order: there the time-out is reported by rvc_synchronize as RVC_BACKEND. */
long long rvc_retrieval_recoveries(rvc_engine *e);
/* IVF-probed retrieval: search the index as upstream searches its IndexIVFFlat files -- the nprobe nearest lists, then exact L2 inside
   them -- instead of scanning every row.  rvc_set_index_ivf attaches the structure (coarse centroids [nlist][dim] and the list number of every row) to the index
   the engine holds, after rvc_load_index / rvc_load_index_device / rvc_index_broadcast; both arrays are copied.  Rows keep their numbers: the ids of rvc_get_knn
   mean what they mean for the flat search.  Fewer than k rows (rvc_index_k: four, or eight) in the probed lists: the missing hits are idx -1 / dist +inf and that frame is not blended.
   RVC_SHAPE: no index loaded, dim or n different from the index, nlist 0 or above 65536, an assignment outside [0, nlist), a non-finite centroid, nprobe outside
   [0, 64], nprobe >= 1 without a structure.  Loading or broadcasting a new index drops the structure and returns nprobe to 0.  nprobe is engine-wide (not per
   stream) and part of a plan's identity. */
rvc_status rvc_set_index_ivf(rvc_engine *e, const float *centroids, size_t nlist, size_t dim, const int32_t *assign, size_t n);
rvc_status rvc_set_index_nprobe(rvc_engine *e, int nprobe);   /* 0 = flat search (default); 1..64 = probe that many lists, clamped to nlist */
int rvc_index_nprobe(rvc_engine *e);                          /* 0 = flat */
rvc_status rvc_index_ivf_info(rvc_engine *e, size_t *nlist, size_t *longest_list, size_t *empty_lists);
/* Train an IVF structure for the loaded index on the device: Lloyd's k-means over the rows in HBM -- c_j starts as row init_rows[j], an
   assign step (every row to the list with the smallest (d, j), d the exact distance of the probe) and then up to `iters` update steps (the fp64 mean of a list's
   rows, rounded once; an empty list keeps its centroid: no splitting, no reseeding), each followed by an assign step; it stops early behind an assign step that
   moved no row.  The result is attached exactly as rvc_set_index_ivf would (same CSR build, plans cleared, nprobe back to 0).  nlist 0 = upstream's rule
   min(floor(16 sqrt(n)), n / 39) clamped to [1, 65536]; iters 0..100; init_rows NULL = the seeded sample (the nlist rows with the smallest (h(seed, i), i), in
   ascending row number).  The same index and arguments give the same bits on every run and every rank.  RVC_SHAPE, the engine keeping the structure it had: no
   index loaded, nlist above n or 65536, iters outside [0, 100], an initial row out of range or named twice, a row of the index that holds a NaN or an Inf (the
   message names the first).  A failure behind these checks leaves the engine with no structure and a flat search. */
rvc_status rvc_train_index_ivf(rvc_engine *e, size_t nlist, int iters, const int32_t *init_rows, uint32_t seed);
/* of the last training on this engine: update steps done, rows moved by the last assign step, the objectives of the assign steps
   (up to cap of them; *n_obj = how many there are), device milliseconds {assign, update, total}; RVC_SHAPE before a training has completed */
rvc_status rvc_index_ivf_train_info(rvc_engine *e, int *iters_run, size_t *moved_last, double *objective, size_t cap, size_t *n_obj, double ms[3]);
/* read the attached structure back, trained or set (export, tests): RVC_SHAPE when none is attached or a capacity is short */
rvc_status rvc_get_index_ivf(rvc_engine *e, float *centroids, size_t cap_centroid_floats, int32_t *assign, size_t cap_rows);
/* Build a voice's index from its recordings on the device: upstream's "train feature index" with this engine's own ContentVec, so that
   the rows and the queries that will search them come from the same arithmetic.  begin opens a build, add appends the ContentVec frames of one recording to a
   row store in HBM, finish installs the store as the engine's index; the rows never visit the host.
   begin: needs ContentVec (RVC_CONTENTVEC_NOT_LOADED).  window = samples at 16 kHz per ContentVec run, 0 = 48 000 (3 s); the run is rvc_hubert's one-stream plan
   of that length whatever rvc_set_streams says, so the rows are rvc_hubert's rows bit for bit; a window ContentVec yields no frame for: RVC_SHAPE.
   capacity_hint = rows the store [capacity][dim] (fp32, one device allocation) starts with, 0 = 4096; an append that would overflow it grows it to twice its
   size, or to the needed size if that is larger, with a device-to-device copy.  A second begin while a build is open: RVC_SHAPE.
   add / add_device (host / device samples): the recording is cut into consecutive windows, no overlap, no padding; every full window contributes its T frames
   as T rows, the tail runs at its own length and is dropped silently when it is shorter than ContentVec's receptive field (where rvc_hubert says "input too
   short").  The rows of one add are exactly the frames rvc_hubert returns for each of these slices, in time order; nothing carries from one add to the next.
   A row that holds a NaN or an Inf is not stored but counted (dropped_nonfinite); *rows_added excludes such rows.  One synchronisation per add.  Without begin:
   RVC_SHAPE.  The engine's loaded index keeps serving rvc_infer while a build is open: nothing before finish touches it.
   finish: rows > max_rows: Lloyd's k-means with reduce_to centres over the store -- the trainer of rvc_train_index_ivf (same seeded sample, assign and update
   steps, early stop; iters 0..100), deterministic bit for bit -- and the centres in centre order become the rows.  max_rows = 0 and reduce_to = 0 select
   upstream's rule: above 200 000 rows, 10 000 centres.  The result is installed as rvc_load_index_device installs a matrix (auxiliary layouts rebuilt, plans
   cleared, any IVF structure dropped, nprobe back to 0) and the build is closed; no IVF structure is trained (rvc_train_index_ivf does that).  RVC_SHAPE, the
   build staying open and the engine keeping its index: fewer rows than rvc_index_k(e) to install, reduce_to above the rows held or above 65536, iters out of
   range.
   abort frees the store; rvc_destroy aborts an open build.  info: rows stored, the store's capacity, ContentVec runs so far, rows dropped, device milliseconds
   {ContentVec runs, appends, reduction}; RVC_SHAPE when no build is open. */
rvc_status rvc_index_build_begin(rvc_engine *e, size_t window, size_t capacity_hint);
rvc_status rvc_index_build_add(rvc_engine *e, const float *pcm16k, size_t n, size_t *rows_added);
rvc_status rvc_index_build_add_device(rvc_engine *e, const void *d_pcm16k, size_t n, size_t *rows_added);
rvc_status rvc_index_build_info(rvc_engine *e, size_t *rows, size_t *capacity, size_t *windows, size_t *dropped_nonfinite, double ms[3]);
rvc_status rvc_index_build_finish(rvc_engine *e, size_t max_rows, size_t reduce_to, int iters, uint32_t seed);
void       rvc_index_build_abort(rvc_engine *e);
/* the synthesizer's two noise inputs are explicit counter-based (Philox4x32-10) streams */
void rvc_set_noise_seed(rvc_engine *e, uint32_t seed, uint32_t stream_id);
void rvc_reset_state(rvc_engine *e);     /* zero the 1024-entry pitch cache and the chunk counter */

/* ---- formant shift: the plugin's resonance shift (obs-rvc/src/lib.rs:80,103,176,369-375,446-451), semitones in [-5, 5] ---- */
/* Moves the formants (the timbre) and keeps the pitch: with f = 2^(phi / 12), the latent and the harmonic source are stretched to
 * R2 = ceil(R f) frames (the source's f0 scaled by R2 / R), the decoder runs on them, and its output is resampled from upp_res =
 * floor(f sr / 100) to sr / 100 samples per frame; the f0 the pitch cache keeps is multiplied by (float)2^(-phi / 12).  The output
 * is always R sr / 100 samples; phi = 0 is the plain path (same plan, same output).  Per stream, like pitch_shift: rvc_set_formant_shift
 * sets every stream and the default of streams rvc_set_streams adds later (existing streams keep theirs); rvc_reset_state leaves the
 * values alone.  Out of range or NaN: RVC_SHAPE.  Streams whose values give different R2 run one bucket per R2 (synchronously; not with
 * graph replay or chunk pipelining: RVC_SHAPE).  DESIGN.md "Formant shift" has the definition. */
rvc_status rvc_set_formant_shift(rvc_engine *e, double semitones);
rvc_status rvc_set_formant_shift_stream(rvc_engine *e, int stream, double semitones);
/* host only, pure: out = {R2, upp_res} of a return_length, a model sample rate (a multiple of 100) and a shift */
rvc_status rvc_formant_geometry(size_t return_length, size_t sample_rate, double semitones, size_t out[2]);

/* ---- pitch controls: transpose in semitones, voiced range, f0 median filter, snap to a scale (DESIGN.md "Pitch controls") ---- */
/* The integer pitch_shift arguments of rvc_pitch / rvc_infer* / rvc_session_* keep the reference's meaning bit for bit: 2^(pitch_shift / 12) with
 * Rust's truncating division (rvc.rs:121), i.e. whole octaves only -- pitch_shift = 7 shifts nothing.  rvc_set_pitch_semitones is the real
 * transpose.  Per stream and per chunk, on the f0 rows of the window (0 Hz = unvoiced), from either f0 method, in this order:
 *   1. f *= 2^(pitch_shift / 12) [* the formant factor on infer calls] * (float)2^(semitones / 12); semitones = 0 multiplies by nothing
 *   2. range gate: a voiced row with f < lo_hz or f > hi_hz becomes unvoiced; lo_hz = 0 and hi_hz = +inf = off
 *   3. median filter of radius 0..7 (window 2 r + 1, rows outside the window are 0, unvoiced zeros take part): scipy.signal.medfilt
 *   4. scale snap: bit k of pitch_class_mask allows pitch class k (C = 0; MIDI note n is allowed iff bit n mod 12 is set); with
 *      n = 69 + 12 log2(f / 440) and target = the nearest allowed note (a tie goes to the lower one), f *= 2^(strength (target - n) / 12);
 *      mask = 0 or strength = 0 = off; mask bits above bit 11, strength outside [0, 1]: RVC_SHAPE
 * The conditioned rows are what rvc_pitch returns, what the "f0" tap shows and what the pitch cache and the synthesizer get.  Semantics as
 * rvc_set_formant_shift[_stream]: the engine-wide call sets every stream and the default of streams rvc_set_streams adds later,
 * rvc_reset_state leaves the values alone, a bad stream number gives RVC_SHAPE with a message.  Unlike the formant shift the values are no
 * part of a plan's identity: changing them between chunks builds no plan, and they hold under graph replay, chunk pipelining,
 * rvc_infer_batch_g and the session. */
rvc_status rvc_set_pitch_semitones(rvc_engine *e, double semitones);                   /* [-24, 24]; NaN / out of range: RVC_SHAPE */
rvc_status rvc_set_pitch_semitones_stream(rvc_engine *e, int stream, double semitones);
rvc_status rvc_set_f0_range(rvc_engine *e, double lo_hz, double hi_hz);                /* 0, +inf = off; lo > hi, negative, NaN: RVC_SHAPE */
rvc_status rvc_set_f0_range_stream(rvc_engine *e, int stream, double lo_hz, double hi_hz);
rvc_status rvc_set_f0_median(rvc_engine *e, int radius);                               /* 0..7 */
rvc_status rvc_set_f0_median_stream(rvc_engine *e, int stream, int radius);
rvc_status rvc_set_f0_snap(rvc_engine *e, uint32_t pitch_class_mask, double strength);
rvc_status rvc_set_f0_snap_stream(rvc_engine *e, int stream, uint32_t pitch_class_mask, double strength);

/* ---- consonant protection: upstream RVC's `protect`, next to the index rate (DESIGN.md "Consonant protection") ---- */
/* With the index rate up, breaths and voiceless consonants are pulled towards index vectors as well, and they have no pitch for the synthesizer to hang them
 * on ("tearing": buzzing on s, t, f).  Per stream, protect is a double in [0, 0.5]; 0.5 = off, the default (upstream: `protect < 0.5` enables it).  On an infer
 * call whose plan uses the index (an index is loaded and the index rate is > 0), after the retrieval has blended and with the pitchf rows the synthesizer
 * gets (pitch shift, pitch controls and the cache update done): a row r with pitchf[r] < 1.0f is unvoiced, and on unvoiced rows every channel becomes
 *   phone[c][r] = p * phone[c][r] + (1 - p) * raw[c][r],   p = (float)protect, 1 - p in float, raw = the ContentVec feature the row had before the retrieval.
 * Voiced rows, streams at 0.5 and calls without an index keep their bits; p = 0 gives the raw row.  rvc_get_knn's hits, rvc_hubert, rvc_extract_feature,
 * rvc_pitch and the pitch cache are unaffected.  Semantics as rvc_set_pitch_semitones[_stream]: the engine-wide call sets every stream and the default of
 * streams rvc_set_streams adds later, rvc_reset_state leaves the values alone, a bad stream number gives RVC_SHAPE with a message.  Whether ANY stream of
 * a call is below 0.5 is part of a plan's identity (the first such call builds a plan, as the first call with an index does); the values are not: changing
 * 0.33 to 0.2 between chunks builds nothing, and they hold under graph replay, chunk pipelining, rvc_infer_batch_g and the session. */
rvc_status rvc_set_protect(rvc_engine *e, double protect);                 /* [0, 0.5]; 0.5 = off; NaN / out of range: RVC_SHAPE */
rvc_status rvc_set_protect_stream(rvc_engine *e, int stream, double protect);

/* ---- f0 from outside: a per-chunk override of a stream's f0 rows, and upstream RVC's "f0 curve file" for a whole recording (DESIGN.md "f0 from outside") ---- */
/* Override rows: a stream may bring n <= 1024 rows in Hz for the END of its next f0 window (row i of n is window row Tm - n + i; the window's Tm is that of the
 * consuming call, 1 + f0 frame / 160).  A NaN row keeps the tracker's value, 0 is unvoiced, anything else is a finite value in (0, 20000].  The rows REPLACE the
 * f0 method's rows in front of everything else: the multiplier (pitch_shift, formant factor, rvc_set_pitch_semitones), range gate, median, snap, the pitch cache
 * and protect apply to them as to the tracker's.  So -- unlike upstream, which pastes its curve behind its transpose -- an override and a curve are transposed like
 * any f0: for absolute values call with pitch_shift = 0 and rvc_set_pitch_semitones(e, 0).  The tracker still runs, and an f0 method must be loaded; a model
 * without pitch guidance ignores overrides and curve.
 *   rvc_set_f0_override_stream: hz == NULL or n == 0 clears.  RVC_SHAPE (state unchanged): a bad stream number, n > 1024, a negative or infinite value or one above
 *     20000.  n greater than the window's Tm is refused (RVC_SHAPE, nothing run, the override stays) by the call that would consume it.
 *   rvc_set_f0_override_hold: 0 (default): an override is consumed by the next infer call of its stream (rvc_infer*, rvc_infer_batch_g, the session; rvc_pitch
 *     honours and consumes stream 0's); 1: it stays until cleared.  rvc_reset_state and rvc_set_streams clear pending overrides.
 * Whether ANY stream of a call has an override is part of a plan's identity (the first such call builds a plan); the values are not: they travel in front of the
 * chunk and hold under graph replay, chunk pipelining, rvc_infer_batch_g and the session.  Calls without an override run the launches they always ran.
 * The curve: n >= 1 breakpoints (t seconds strictly increasing and finite, hz 0 or in (0, 20000]) of ONE recording, used by rvc_convert* / rvc_convert_file* only
 * (they clear the streams' overrides first; streaming calls never read the curve; model loads leave it alone).  Grid row j stands for j / 100 s: between two voiced
 * breakpoints linear, next to a 0 the nearer breakpoint's value (a tie goes to the earlier), on the last breakpoint its value, NaN outside [t_0, t_n-1].
 *   rvc_set_f0_curve: n == 0 clears; RVC_SHAPE and the old curve kept on bad input.  rvc_f0_curve_grid: the first n_frames rows of the grid as the device builds
 *     it (all NaN without a curve); cap < n_frames: RVC_SHAPE.
 *   rvc_convert_f0: the conditioned f0 (what the synthesizer got) of the last completed conversion, one value per 10 ms frame of the recording; RVC_SHAPE before
 *     a conversion has completed, for a model without pitch guidance, or with cap short (*n_frames is still written). */
rvc_status rvc_set_f0_override_stream(rvc_engine *e, int stream, const float *hz, size_t n);
rvc_status rvc_set_f0_override_hold(rvc_engine *e, int hold);
rvc_status rvc_set_f0_curve(rvc_engine *e, const double *t_sec, const float *hz, size_t n);
rvc_status rvc_f0_curve_grid(rvc_engine *e, size_t n_frames, float *out, size_t cap);
rvc_status rvc_convert_f0(rvc_engine *e, float *hz, size_t cap, size_t *n_frames);

/* ---- multi-GPU (BASELINE configs[4]; no counterpart in the reference: one RvcInfer per process, rvc.rs:133-134) ---- */
/* Streams shard across GPUs with NO per-chunk collective: one process + one engine per GPU, stream s on rank s mod world.  The one
 * exchange step is at load: the shared retrieval index travels from rank 0 into every rank's HBM with ONE ncclBroadcast over
 * RCCL / xGMI.  Rank 0 calls rvc_rccl_unique_id and hands the 128 bytes to the other ranks by any host-side means (pipe, file,
 * TCP store); then EVERY rank calls rvc_index_broadcast with the same id.  Rank 0 passes the (n, dim) fp32 matrix (or NULL to
 * send the index its engine already holds); the other ranks pass vectors = NULL and n = dim = 0 (or the shape they expect, which
 * is then checked).  librccl is loaded lazily (dlopen; RVC_RCCL_LIB overrides the name): single-GPU use never touches it. */
#define RVC_RCCL_UNIQUE_ID_BYTES 128
rvc_status rvc_rccl_unique_id(void *id128);
rvc_status rvc_index_broadcast(rvc_engine *e, const void *unique_id128, int rank, int world, const float *vectors, size_t n, size_t dim);
/* RVC_OK when librccl can be loaded in this process (creates no communicator).  Hosts agree on it across ranks BEFORE calling
 * rvc_index_broadcast, so that a rank without the library cannot leave the others waiting in the communicator set-up.  Inside
 * rvc_index_broadcast nothing a single rank finds wrong with its own arguments makes it leave alone: rank 0 sends an empty header when
 * its index is unusable, every rank checks the header against what it expects, and ONE all-reduce of the verdicts precedes the payload
 * broadcast -- the ranks return the error together (tests/test_gpu_multi.py runs this with two ranks). */
rvc_status rvc_rccl_available(void);
/* the engine's last rvc_index_broadcast: ms[0] communicator set-up, ms[1] header + agreement + payload broadcast, ms[2] device-side
 * repack of the index (MFMA-fragment order + norms; the matrix never returns to the host); *ranks = ncclCommCount */
rvc_status rvc_index_broadcast_info(rvc_engine *e, double ms[3], int *ranks);

/* ---- many concurrent streams on one GPU (BASELINE configs 4-5) ---- */
/* The engine then holds n_streams independent stream states (pitch cache, noise counters) that share weights. */
rvc_status rvc_set_streams(rvc_engine *e, int n_streams);
/* input [n_streams][n], out [n_streams][cap_per_stream]; all streams use the same geometry */
rvc_status rvc_infer_batch(rvc_engine *e, const float *input, size_t n, size_t sample_frame_16k_size, int32_t pitch_shift,
                           uint32_t skip_head, uint32_t return_length, float *out, size_t cap_per_stream, size_t *out_len);
/* device-resident variant (input/out are HIP device pointers on the engine's device; no host copy, no sync
 * unless sync != 0).  Used by the throughput bench so that the timed region starts with inputs in HBM. */
rvc_status rvc_infer_device(rvc_engine *e, const void *d_input, size_t n, size_t sample_frame_16k_size, int32_t pitch_shift,
                            uint32_t skip_head, uint32_t return_length, void *d_out, size_t cap_per_stream, size_t *out_len, int sync);
/* the same with one pitch shift PER STREAM (pitch_shift[n_streams]): every stream of a batch is a caller of its own with its own
 * settings, as every stream is its own process in the reference (obs-rvc/src/lib.rs:701-707) */
rvc_status rvc_infer_batch_v(rvc_engine *e, const float *input, size_t n, size_t sample_frame_16k_size, const int32_t *pitch_shift,
                             uint32_t skip_head, uint32_t return_length, float *out, size_t cap_per_stream, size_t *out_len);
rvc_status rvc_infer_device_v(rvc_engine *e, const void *d_input, size_t n, size_t sample_frame_16k_size, const int32_t *pitch_shift,
                              uint32_t skip_head, uint32_t return_length, void *d_out, size_t cap_per_stream, size_t *out_len, int sync);
/* many streams, every stream with ITS OWN geometry (in the reference every stream is a process with its own chunk length, crossfade and
 * extra context: obs-rvc/src/lib.rs:200-227, 694).  All arrays have n_streams entries (inputs / outs: host pointers per stream;
 * pitch_shift may be NULL = 0 for every stream).  Streams with equal (n, sample_frame_16k_size, skip_head, return_length) run as one
 * batch; a server can mix 160 ms and 300 ms callers in one call.  At most as many different geometries per call as the plan cache holds
 * (8 unless rvc_set_plan_cache raised it). */
rvc_status rvc_infer_batch_g(rvc_engine *e, const float *const *inputs, const size_t *n, const size_t *sample_frame_16k_size, const int32_t *pitch_shift,
                             const uint32_t *skip_head, const uint32_t *return_length, float *const *outs, const size_t *caps, size_t *out_lens);
rvc_status rvc_synchronize(rvc_engine *e);
void rvc_set_use_graph(rvc_engine *e, int on);    /* replay the per-chunk launch sequence from a hipGraph */
/* Plan cache.  The engine keeps one "plan" per call geometry (n, sample_frame_16k_size, skip_head, return_length, stream count, retrieval on/off):
 * its activation arena, plan-time weight copies and launch list.  Every plugin instance has its own geometry (obs-rvc/src/lib.rs:200-227), so a
 * server sees as many plans as it has distinct caller settings.  The cache holds n_plans of them (default 8, 2..256), least recently used evicted
 * first.  A MISS costs a plan build: arena allocation (tens of MB at one stream, GBs at 64), composed weights and a device synchronisation --
 * tens of milliseconds; a server that rotates through more geometries than the cache holds pays that on every call.  rvc_plan_cache_info reports
 * capacity, plans currently cached and plans built since rvc_create (-> 1 on a valid engine). */
rvc_status rvc_set_plan_cache(rvc_engine *e, int n_plans);
/* Plan-time selection by measurement.  The planner's kernel / tile rules are thresholds measured on one box at a handful of stream counts and one geometry;
 * every plugin instance has its own geometry (obs-rvc/src/lib.rs:200-227) and GPUs of one pool differ.  With on = 1 (the default) a plan of MORE THAN 4 STREAMS
 * times, while it is built and on the engine's own device, the eligible kernels / tiles of every layer that has more than one (the rule-based choice and its
 * neighbours across the nearest thresholds: a warm-up and 1-3 timed launches each) and keeps the fastest; results are cached per process by (device, layer
 * signature, stream count).  All candidates are parity-tested kernels: the choice affects fp32 summation order only.  A first plan build at 64 streams takes
 * ~0.1-0.3 s longer, later builds of the same layers nothing.  on = 0: the rules only (results then do not depend on timing).  rvc_plan_autotune_info reports
 * the engine's LAST plan build: layers tuned by trials, layers whose choice differs from the rules, layers served from the cache, ms in trials, ms in all. */
rvc_status rvc_set_plan_autotune(rvc_engine *e, int on);
rvc_status rvc_plan_autotune_info(rvc_engine *e, int *tuned, int *changed, int *cache_hits, double *tune_ms, double *build_ms);
/* EXPLORATORY (no counterpart in the reference, off by default, never used for the headline figure): mode 1 = the 1-D layers with >= 128 output rows (ContentVec's projections and stem, the decoder's wide stages) run every
 * fp32 product as three bf16 matrix-core products (a_hi b_hi + a_hi b_lo + a_lo b_hi, fp32 accumulate) in launches of >= 250 workgroups of 128 x 128 (many
 * streams); ~2^-16 relative per product instead of fp32 rounding.  mode 0 = fp32 everywhere, the reference's arithmetic. */
rvc_status rvc_set_gemm_precision(rvc_engine *e, int mode);
int rvc_plan_cache_info(rvc_engine *e, int *capacity, int *cached, long long *builds);
/* Offline throughput mode (no counterpart in the reference, whose protocol is one request at a time): with on != 0, consecutive
 * rvc_infer_device(..., sync = 0) calls overlap chunk i+1's ContentVec / f0 branches with chunk i's synthesizer (two plan slots).
 * Results are identical to the serial order; every call needs its own output buffer until rvc_synchronize. */
void rvc_set_pipeline(rvc_engine *e, int on);

/* ---- caller-side post-processing of the plugin, same host-buffer convention ---- */
/* envelop_mixing (obs-rvc/src/rt_utils.rs:119-132): output[i] *= (rms(input)/max(rms(output),1e-3))^(1-mix_rate) */
rvc_status rvc_envelop_mixing(rvc_engine *e, const float *input, float *output, size_t output_len, size_t sample_rate, double mix_rate);
/* get_sola_offset (rt_utils.rs:60-90) + crossfade / tail save / frame extraction (obs-rvc/src/lib.rs:768-794).
 * output needs sola_len + search + frame valid samples; sola_buffer (sola_len) is updated in place. */
rvc_status rvc_sola_step(rvc_engine *e, float *output, size_t output_len, float *sola_buffer, size_t sola_len, size_t search,
                         size_t frame, float *frame_out, size_t *sola_offset);
/* The same step with a choice of crossfade (no counterpart in the plugin; DESIGN.md "Phase-vocoder crossfade and input gate").  LINEAR is
 * rvc_sola_step bit for bit.  PHASE_VOCODER replaces the sin^2 blend of output[offset .. offset + sola_len) by the blend of the upstream
 * real-time client's "phase vocoder" switch: the magnitudes of the two windowed spectra are added and every bin's phase glides from the saved
 * tail's to the new segment's along the seam; offset search, saved tail and frame extraction are unchanged.  sola_len < 2 blends linearly;
 * sola_len > 4096 or an unknown mode: RVC_SHAPE. */
enum { RVC_CROSSFADE_LINEAR = 0, RVC_CROSSFADE_PHASE_VOCODER = 1 };
rvc_status rvc_sola_step_x(rvc_engine *e, float *output, size_t output_len, float *sola_buffer, size_t sola_len, size_t search,
                           size_t frame, float *frame_out, size_t *sola_offset, int crossfade);
/* Input gate of the session on host buffers (the upstream client's response threshold, restated causally).  zc = sample_rate / 100, n a multiple
 * of zc, x = concat(hist3zc, chunk): block i (zc samples) of `out` is zero when 20 log10(max(rms(x[i zc .. i zc + 4 zc)), 1e-5)) < threshold_db
 * and the chunk's samples otherwise; hist_out = the last 3 zc samples of x (ungated).  threshold_db <= -60 = off (out = chunk); NaN: RVC_SHAPE. */
rvc_status rvc_input_gate(rvc_engine *e, const float *hist3zc, const float *chunk, size_t n, size_t sample_rate, double threshold_db,
                          float *out, float *hist_out);

/* ---- the plugin's two sample-rate converters ---- */
/* rubato::FftFixedInOut::<f32>::new(rate_in, rate_out, chunk_size_in, 1) at obs-rvc/src/lib.rs:236-242 (host rate -> 16 kHz in front
 * of infer, model rate -> host rate behind it); one channel.  The converter runs on the engine's device and stream and must be
 * destroyed before the engine. */
typedef struct rvc_resampler rvc_resampler;
rvc_status rvc_resampler_create(rvc_engine *e, size_t rate_in, size_t rate_out, size_t chunk_size_in, rvc_resampler **out);
void rvc_resampler_destroy(rvc_resampler *r);
size_t rvc_resampler_input_frames_next(rvc_resampler *r);    /* Resampler::input_frames_next: frames one process call consumes */
size_t rvc_resampler_output_frames_max(rvc_resampler *r);    /* Resampler::output_frames_max (lib.rs:244): frames it produces */
void rvc_resampler_reset(rvc_resampler *r);                  /* Resampler::reset */
/* Resampler::process (lib.rs:675) / process_into_buffer (lib.rs:747-749).  n_in must equal input_frames_next(), otherwise
 * RVC_SHAPE (rubato: ResampleError::WrongNumberOfInputFrames, on which the plugin panics); *n_out = output_frames_max(). */
rvc_status rvc_resampler_process(rvc_resampler *r, const float *in, size_t n_in, float *out, size_t cap, size_t *n_out);
/* device-resident variant (HIP device pointers, engine's stream; no sync unless sync != 0) */
rvc_status rvc_resampler_process_device(rvc_resampler *r, const void *d_in, void *d_out, int sync);

/* ---- streaming spectral-gate noise reduction (the upstream real-time client's input / output noise reduction; DESIGN.md "Spectral-gate noise reduction") ---- */
/* No counterpart in the plugin.  Causal, no look-ahead, 10 ms delay.  Per stream at sample_rate (a multiple of 100, at most 192000: the frame must fit
 * the kernels' LDS budget, N <= 3840): zc = sample_rate / 100 is the hop, N = 2 zc the frame (50 Hz bins), K = zc + 1 bins, w[j] = sin(pi (j + 0.5) / N)
 * the analysis and synthesis window (w[j]^2 + w[j + zc]^2 = 1: an all-ones mask reconstructs the input).  Input = hop blocks x_0, x_1, ... with x_{-1} = 0,
 * frame m = concat(x_{m-1}, x_m); state per stream: S[k] = 0, g[k] = 0, the previous block, the previous frame's synthesis tail.  Frame m, bin k:
 *   1. X[k] = sum_j w[j] frame[j] exp(-2 pi i k j / N), M = |X[k]|
 *   2. slope = (M - S[k]) / max(S[k], 1e-8), then S[k] = a S[k] + (1 - a) M, a = (float)exp(-10 / 200)        (200 ms noise floor)
 *   3. g0[k] = 1 / (1 + exp(-(slope - threshold) / 0.1))
 *   4. g1[k] = sum_{|d| <= 10, 0 <= k + d < K} t[d] g0[k + d] / sum_{same d} t[d], t[d] = 11 - |d|             (+-500 Hz triangle)
 *   5. g[k] = max(g1[k], b g[k]), b = (float)exp(-10 / 50)                                                     (50 ms release hold)
 *   6. Y[k] = (strength g[k] + (1 - strength)) X[k]
 *   7. f = w . irfft_N(Y); output block m = f_{m-1}[zc:] + f_m[:zc] = the gated x_{m-1}: the input delayed by zc samples.
 * strength in [0, 1], 0 = off and the default: that stream is copied UNDELAYED, bit for bit, and its state is left alone; threshold in [0, 16], default 2.
 * NaN / out of range, a stream out of range, n not a positive multiple of zc (or more than 4096 hops), an unsupported sample_rate: RVC_SHAPE with a message.  A stream's result
 * depends neither on the other streams nor on how its signal is cut into calls.  The denoiser runs on the engine's device and stream and must be
 * destroyed before the engine. */
typedef struct rvc_denoiser rvc_denoiser;
rvc_status rvc_denoiser_create(rvc_engine *e, size_t sample_rate, int n_streams, rvc_denoiser **out);
void rvc_denoiser_destroy(rvc_denoiser *d);
void rvc_denoiser_reset(rvc_denoiser *d);                      /* zero every stream's state; the settings stay */
rvc_status rvc_denoiser_set(rvc_denoiser *d, int stream /* -1 = all */, double strength, double threshold);
size_t rvc_denoiser_latency(rvc_denoiser *d);                  /* zc: samples of delay of a stream whose strength is > 0 */
/* host buffers in [n_streams][n], out [n_streams][n] */
rvc_status rvc_denoiser_process(rvc_denoiser *d, const float *in, size_t n, float *out);
/* device-resident variant (HIP device pointers, stream b at d_in + b in_stride / d_out + b out_stride floats; engine's stream; no sync unless sync != 0);
 * d_in == d_out with equal strides is allowed */
rvc_status rvc_denoiser_process_device(rvc_denoiser *d, const void *d_in, void *d_out, size_t n, size_t in_stride, size_t out_stride, int sync);

/* ---- the plugin's per-chunk state machine as one call (SURVEY.md section 8 rows f1-f3 chained, all buffers resident in HBM) ---- */
/* `create`/`update` + `process_one_frame` of the filter (obs-rvc/src/lib.rs:181-260, 659-795): host-rate ring, 16 kHz ring, both
 * resamplers, RvcInfer::infer, RMS envelope mixing and SOLA.  One H2D copy (the new chunk), one D2H copy (the finished frame) and
 * one synchronisation per chunk (with the phase-vocoder crossfade and the input gate as well).  Lengths in seconds as in the plugin's settings; skip_inference != 0 = pass-through mode
 * (lib.rs:224-227).  The session covers every stream of the engine (rvc_set_streams before rvc_session_create): process then takes
 * input [streams][n] and writes output [streams][cap], sola_offset [streams].  Destroy the session before the engine.  The session has no
 * formant setting, no pitch controls and no consonant protection of its own: it honours the engine's per-stream values (rvc_set_formant_shift[_stream],
 * rvc_set_pitch_semitones / rvc_set_f0_range / rvc_set_f0_median / rvc_set_f0_snap [_stream], rvc_set_protect[_stream]). */
typedef struct rvc_session rvc_session;
rvc_status rvc_session_create(rvc_engine *e, size_t sample_rate, double sample_length, double crossfade_length, double extra_inference_time,
                              size_t model_output_sample_rate, int32_t pitch_shift, double rms_mix_rate, int skip_inference, rvc_session **out);
void rvc_session_destroy(rvc_session *s);
size_t rvc_session_frame_size(rvc_session *s);                 /* sample_frame_size: samples per process call, in and out */
void rvc_session_set_params(rvc_session *s, int32_t pitch_shift, double rms_mix_rate);      /* every stream */
/* one stream's pitch shift and RMS mix rate (the plugin's per-instance settings, obs-rvc/src/lib.rs:174-185); the others keep theirs */
rvc_status rvc_session_set_params_stream(rvc_session *s, int stream, int32_t pitch_shift, double rms_mix_rate);
/* Crossfade of the SOLA seam (RVC_CROSSFADE_*; LINEAR at creation), every stream or one; a session whose streams use both serves them in the
 * same call.  Unknown mode, stream out of range, PHASE_VOCODER with sola_buffer_frame_size > 4096: RVC_SHAPE with a message. */
rvc_status rvc_session_set_crossfade(rvc_session *s, int mode);
rvc_status rvc_session_set_crossfade_stream(rvc_session *s, int stream, int mode);
/* Input gate (rvc_input_gate) in front of the host-rate ring, every stream or one: the resampler, the model and the RMS-mix input see the gated
 * signal, in pass-through mode too.  Off at creation and at threshold_db <= -60 (the chunk passes bit for bit).  The 30 ms history is that of the
 * ungated input; it is kept from the first time any stream's gate is switched on (zeros before).  NaN, stream out of range: RVC_SHAPE. */
rvc_status rvc_session_set_input_gate(rvc_session *s, double threshold_db);
rvc_status rvc_session_set_input_gate_stream(rvc_session *s, int stream, double threshold_db);
/* Spectral-gate noise reduction (rvc_denoiser above) inside the session, per side and per stream, every stream or one; strength 0 (the default) = off.
 * RVC_DENOISE_INPUT sits between the input gate and the host-rate ring: the resampler, the model and the RMS-mix input see the denoised chunk, in
 * pass-through mode too.  RVC_DENOISE_OUTPUT runs on the finished frame behind SOLA and the crossfade, at the host rate.  Each side's denoiser is created the
 * first time a stream switches the side on and is not launched before that; streams at strength 0 keep their bits.  Switching a side on adds zc samples
 * (10 ms) of delay on that side for that stream from that chunk on; delay and state survive rvc_session_set_params.  The chunk keeps its one H2D copy, one
 * D2H copy and one synchronisation (the chunk after a setter call uploads the settings with one more of each).  NaN / out of range, unknown side, stream
 * out of range, a session above 192000 Hz: RVC_SHAPE with a message. */
enum { RVC_DENOISE_INPUT = 0, RVC_DENOISE_OUTPUT = 1 };
rvc_status rvc_session_set_noise_reduction(rvc_session *s, int side, double strength, double threshold);
rvc_status rvc_session_set_noise_reduction_stream(rvc_session *s, int stream, int side, double strength, double threshold);
void rvc_session_geometry(rvc_session *s, int32_t out[10]);   /* the derived sizes of lib.rs:200-227 (see session.hip.h) */
rvc_status rvc_session_process(rvc_session *s, const float *input_sample, size_t n, float *output, size_t cap, size_t *sola_offset);

/* ---- conversion of a whole recording (upstream's "model inference" tab, vc_single) ---- */
/* A 16 kHz signal of any length -> the voice's audio at the model's rate.  The recording is cut into windows of ONE geometry, so one plan serves the whole
 * file; the windows run S = rvc_set_streams at a time through the batched infer path (window w = i S + s on stream s in batch i) and are stitched on the
 * device by the plugin's SOLA step in its LINEAR crossfade, chained over the windows.  In frames of 10 ms (160 samples at 16 kHz, zc = rate / 100 at the
 * model's rate), with k the window size in [2, 32], C the context on each side, >= 3, X the crossfade, >= 1, Q = 1 the SOLA search; 0 selects k = 14,
 * C = 48, X = 5 (14: the longest window whose return_length, 351 with C = 48, the synthesizer's LDS-resident attention takes at RVC's head size; a longer
 * one fails at the plan build with that kernel's message):
 *   F = 32 k - 1 frames per window, n = 160 F samples, sample_frame_16k_size = 5120 (k - 1), skip_head = C, hop H = F - 2 C - X - Q (H >= X),
 *   return_length = H + X + Q;   Nf = ceil(N / 160), W = ceil(Nf / H) windows, window w = samples [160 (w H - C), + n), zero outside [0, N).
 * A short last batch is padded with all-zero windows whose outputs are dropped.  Stitch: sola_len = X zc, search = Q zc, frame = H zc, the tail starts as
 * zeros; the output is the W frames in order, cut to Nf zc samples.  With C >= 3 every pitch row a window uses is computed from that window alone.
 * The call BEGINS WITH WHAT rvc_reset_state DOES (pitch caches and chunk counters zeroed): the result depends on the recording and the settings, not on what
 * the engine ran before.  Every batch is one batched infer call with the integer pitch_shift (whole octaves, as everywhere): every per-stream setting
 * (formant shift, pitch controls, protect, noise seeds), the index (rate, k, nprobe), the f0 method and graph replay apply as to any infer call;
 * rvc_set_pipeline is ignored.  highpass != 0 (upstream filters every file it converts): the 48 Hz high-pass of rvc_highpass in front.
 * RVC_MODEL_NOT_LOADED / RVC_CONTENTVEC_NOT_LOADED / RVC_F0_NOT_LOADED as for rvc_infer, before any argument is looked at.  RVC_SHAPE with a message: n = 0; a
 * synthesizer whose rate is not a multiple of 100; k, C or X out of range; H < X; Q zc > 1023 (the SOLA kernels' limit); cap short (*out_len is written). */
/* host only, pure: out = {windows, n, sample_frame_16k_size, skip_head, return_length, hop, zc, output samples} */
rvc_status rvc_convert_geometry(size_t n16k, size_t sample_rate, size_t k, size_t context, size_t crossfade, size_t out[8]);
rvc_status rvc_convert(rvc_engine *e, const float *pcm16k, size_t n, size_t k, size_t context, size_t crossfade, int32_t pitch_shift,
                       int highpass, float *out, size_t cap, size_t *out_len);
/* device-resident variant (HIP device pointers on the engine's device); returns synchronised */
rvc_status rvc_convert_device(rvc_engine *e, const void *d_pcm16k, size_t n, size_t k, size_t context, size_t crossfade, int32_t pitch_shift,
                              int highpass, void *d_out, size_t cap, size_t *out_len);
/* of the last completed convert: windows, batches, the SOLA offset of every window (the first cap_offsets of them), device ms = {high-pass, gather + model,
   stitch, total}; any pointer may be NULL.  RVC_SHAPE before one has completed */
rvc_status rvc_convert_info(rvc_engine *e, size_t *windows, size_t *batches, int32_t *offsets, size_t cap_offsets, double ms[4]);
/* the chained LINEAR rvc_sola_step over windows [n_windows][window_len], tail = zeros at the start: out [n_windows][frame], offsets [n_windows] (may be NULL);
   offsets and samples are rvc_sola_step's, bit for bit.  frame >= sola_len >= 1, search <= 1023, window_len >= search + frame + sola_len, else RVC_SHAPE */
rvc_status rvc_sola_stitch(rvc_engine *e, const float *windows, size_t n_windows, size_t window_len, size_t sola_len, size_t search, size_t frame,
                           float *out, int32_t *offsets);
/* 48 Hz zero-phase high-pass at 16 kHz, a direct FIR of 2 M + 1 taps, M = 1024, over the zero-extended signal; out [n].  In fp64, rounded once to fp32:
   lp[j] = 2 fc sinc(2 fc (j - M)) (0.42 - 0.5 cos(2 pi j / 2M) + 0.08 cos(4 pi j / 2M)), fc = 48 / 16000, scaled to sum 1; h = delta[j - M] - lp;
   y[i] = sum_j h[j] x[i + M - j], accumulated in fp32 in the order j = 0 .. 2M.  n = 0: RVC_SHAPE */
rvc_status rvc_highpass(rvc_engine *e, const float *pcm16k, size_t n, float *out);

/* ---- a file at any rate, with the volume envelope ---- */
/* One-shot sample-rate conversion of a whole signal: a windowed-sinc polyphase converter with the formant stage's filter (Hann-windowed sinc, width 6,
 * rolloff 0.99; torchaudio.functional.resample at its defaults), NOT the streaming converter above.  g = gcd(rate_in, rate_out), o = rate_in / g,
 * n = rate_out / g, b = 0.99 min(o, n), w = ceil(6 o / b), K = 2 w + o; the taps h[j][k], j < n, k < K, are evaluated in fp64 and rounded once to fp32;
 *   N_out = ceil(N_in n / o),   y[i n + j] = sum_{k = 0 .. K-1} h[j][k] x[i o + k - w],   x = 0 outside [0, N_in).
 * Each output is one fp32 fma chain over ascending k; o == n is a copy, bit for bit.  RVC_SHAPE with a message: a rate of 0; o or n above 2048; N_in = 0
 * (or above 2^40); cap short (*n_out is written). */
/* host only, pure: out = {o, n, w, N_out} */
rvc_status rvc_resample_geometry(size_t rate_in, size_t rate_out, size_t n_in, size_t out[4]);
rvc_status rvc_resample(rvc_engine *e, const float *in, size_t n_in, size_t rate_in, size_t rate_out, float *out, size_t cap, size_t *n_out);
/* device-resident variant (HIP device pointers on the engine's device); returns synchronised */
rvc_status rvc_resample_device(rvc_engine *e, const void *d_in, size_t n_in, size_t rate_in, size_t rate_out, void *d_out, size_t cap, size_t *n_out);
/* The whole-file volume envelope (upstream's rms_mix_rate / change_rms; not rvc_envelop_mixing, the plugin's streaming form): y [n_y] at rate_y is rewritten
 * in place; src [n_src] at rate_src is the signal whose envelope it takes on.  For signal s in {1 = src, 2 = y}: L_s = 2 (rate_s / 2), hop_s = rate_s / 2,
 * F_s = 1 + N_s / hop_s, r_s[f] = sqrt(mean(xpad[f hop_s .. f hop_s + L_s)^2)) over the signal zero-padded by L_s / 2 on both sides; both tracks are brought
 * to N_2 points by linear interpolation with half-pixel centres (u = max((i + 0.5) F_s / N_2 - 0.5, 0), i0 = floor(u), i1 = min(i0 + 1, F_s - 1));
 *   out[i] = y[i] R_1[i]^(1 - rate) max(R_2[i], 1e-6)^(rate - 1),
 * the tracks and the product in fp64, rounded once at the store.  rate = 1 leaves y untouched.  RVC_SHAPE: rate outside [0, 1] or NaN; a sample rate below 2
 * (or above 2^20); n_src = 0 or n_y = 0 (or above 2^30). */
rvc_status rvc_change_rms(rvc_engine *e, const float *src, size_t n_src, size_t rate_src, float *y, size_t n_y, size_t rate_y, double rate);
/* A recording at rate_in -> the voice at rate_out (0 = the model's), all on the device: rvc_resample rate_in -> 16 000 (skipped when equal); everything
 * rvc_convert does on that signal; rvc_change_rms with the 16 kHz signal the model saw as the source (behind the high-pass when it is on; skipped at
 * rms_mix_rate = 1); rvc_resample model rate -> rate_out (skipped when equal); a max-abs reduction.  The result is that composition of the public calls,
 * bit for bit.  Statuses: the three *_NOT_LOADED as for rvc_convert, before any argument is looked at; then the RVC_SHAPE cases of each stage in that
 * order; cap short (*out_len is written).  rvc_convert_info reports the windows and offsets of the inner conversion. */
rvc_status rvc_convert_file(rvc_engine *e, const float *pcm, size_t n, size_t rate_in, size_t k, size_t context, size_t crossfade, int32_t pitch_shift,
                            int highpass, double rms_mix_rate, size_t rate_out, float *out, size_t cap, size_t *out_len);
/* device-resident variant; returns synchronised */
rvc_status rvc_convert_file_device(rvc_engine *e, const void *d_pcm, size_t n, size_t rate_in, size_t k, size_t context, size_t crossfade, int32_t pitch_shift,
                                   int highpass, double rms_mix_rate, size_t rate_out, void *d_out, size_t cap, size_t *out_len);
/* of the last completed rvc_convert_file: device ms = {resample in, high-pass, gather + model, stitch, envelope, resample out, total}, the output rate,
   peak = max |out| (exact); any pointer may be NULL.  RVC_SHAPE before one has completed */
rvc_status rvc_convert_file_info(rvc_engine *e, double ms[7], size_t *rate_out, float *peak);

/* ---- f0 analysis, order statistics and auto-transpose (the forks' "proposed pitch") ---- */
/* rvc_analyze_f0: the f0 of a whole 16 kHz recording on the 10 ms grid, Nf = ceil(n / 160) rows in Hz with 0 = unvoiced, without the synthesizer.  The windows
 * are rvc_convert's (same geometry and defaults for k, context, crossfade = 0; same gather; S = rvc_set_streams windows per batch, a short last batch
 * zero-padded); each batch runs the pitch-only plan of that geometry at S streams, and the hop rows of each window go onto the grid.  A row is the f0 method's
 * own, single or hybrid: what rvc_pitch returns for that window with pitch_shift = 0, every pitch control neutral and no override -- the multiplier, range gate,
 * median, snap and formant factor do not apply whatever the streams' settings are (the tail runs under a neutral control block; the settings are not touched).
 * The call begins with what rvc_reset_state does and leaves the state that way.  Needs an f0 method (RVC_F0_NOT_LOADED), neither a voice model nor
 * ContentVec.  highpass != 0: rvc_highpass first.  RVC_SHAPE with a message: n = 0, a bad geometry (the converter's checks), cap short (*n_frames is written);
 * each member of a hybrid keeps its own limits (CREPE: streams x frames <= 65535). */
rvc_status rvc_analyze_f0(rvc_engine *e, const float *pcm16k, size_t n, size_t k, size_t context, size_t crossfade, int highpass, float *hz, size_t cap,
                          size_t *n_frames);
/* device-resident variant (HIP device pointers on the engine's device); returns synchronised */
rvc_status rvc_analyze_f0_device(rvc_engine *e, const void *d_pcm16k, size_t n, size_t k, size_t context, size_t crossfade, int highpass, void *d_hz, size_t cap,
                                 size_t *n_frames);
/* Exact order statistics of the voiced rows.  A row is voiced iff it is finite and > 0.  With the v voiced rows sorted ascending as s[0 .. v), quantile p in
 * [0, 1] gives s[floor(p (v - 1))], the product in double: p = 0.5 is the lower median; the result is an element of the input, bit for bit -- no interpolation,
 * no averaging.  v = 0: every out_hz is 0 and *voiced = 0.  A radix select on the IEEE bit pattern on the device; only the nq values and v come back.
 * rvc_f0_stats takes n host rows; rvc_f0_stats_stream the 1024-row pitch cache of a stream where it lies.  The pitch cache holds CONDITIONED f0 -- behind
 * pitch_shift, the semitone transpose and the pitch controls: a host that wants the raw median of a live stream reads it while its transpose is 0.
 * RVC_SHAPE: n = 0 or above 2^30, nq outside [1, 8], a quantile outside [0, 1] or NaN, a bad stream number. */
rvc_status rvc_f0_stats(rvc_engine *e, const float *hz, size_t n, const double *quantile, size_t nq, float *out_hz, size_t *voiced);
rvc_status rvc_f0_stats_stream(rvc_engine *e, int stream, const double *quantile, size_t nq, float *out_hz, size_t *voiced);
/* Auto-transpose of the file converter.  target_hz = 0 (the default) = off, else in (0, 20000]; step 0 = exact, 1 = whole semitones, 12 = whole octaves;
 * limit in [0, 24] semitones (the front ends default to 12).  Anything else: RVC_SHAPE, state unchanged.  With a target set and a model with pitch guidance,
 * rvc_convert* and rvc_convert_file* run, in front of their first batch, rvc_analyze_f0 on the signal the model will see (16 kHz, behind the high-pass when it
 * is on) with the call's own k, context and crossfade; merge the f0 curve in when one is in force (row = isnan(curve) ? tracked : curve); take the lower
 * median m; a = 12 log2(target / m) in double, rounded to the step (ties to even), clamped to [-limit, limit], 0 when no row is voiced.  For the duration of
 * the call every stream's multiplier takes the factor (float)2^(a / 12) behind the rvc_set_pitch_semitones factor (a = 0 multiplies by nothing); it is no
 * part of a plan's identity and is gone on every way out of the call.  pitch_shift and the semitones compose with it; a model without pitch guidance skips
 * all of it; streaming calls never read the setting.  The conversion proper starts from the same reset state as with the setting off.
 * rvc_auto_transpose_info: of the last conversion that ran the analysis -- the median, the voiced rows, a, device ms {analysis, merge + select}; RVC_SHAPE
 * before one has. */
rvc_status rvc_set_auto_transpose(rvc_engine *e, double target_hz, int step, double limit);
rvc_status rvc_auto_transpose(rvc_engine *e, double *target_hz, int *step, double *limit);
rvc_status rvc_auto_transpose_info(rvc_engine *e, float *median_hz, size_t *voiced, double *semitones, double ms[2]);

/* ---- many recordings in one call (upstream's "model inference" tab, vc_multi) ---- */
/* F recordings at 16 kHz, one geometry and one set of settings for all of them: what rvc_convert does to each, with the windows of all files laid end to end
 * and run S = rvc_set_streams at a time, so that a batch holds windows of several files.  File f with N_f >= 1 samples has the windows rvc_convert_geometry
 * gives it: Nf_f = ceil(N_f / 160), W_f = ceil(Nf_f / H), out_f = Nf_f zc.  Global window g = P_f + w with P_f = W_0 + ... + W_{f-1}, 0 <= w < W_f; files
 * stay in the order given and windows in order, nothing is sorted; Wtot = P_F.  Batch i runs globals [i S, min((i + 1) S, Wtot)) on streams 0 ..; only the
 * last batch is padded with all-zero windows.  Window w of file f reads samples [160 (w H - C), + n) of THAT file, zero outside [0, N_f).  The stitch is
 * rvc_convert's per file: the tail in front of a file's first window is zeros, a file that continues in the next batch takes the tail it left behind.
 * Limits: 1 <= F <= 65536, every N_f >= 1, Wtot <= 2^30, sum of out_f <= 2^40; anything else is RVC_SHAPE with a message.
 * rvc_convert_many BEGINS WITH WHAT rvc_reset_state DOES.  All signals go up once, with highpass != 0 each file is filtered on its own (rvc_highpass's bits,
 * the zero extension per file), the outputs come down once; every per-stream setting, the index, the f0 method and graph replay apply as to any infer
 * call; rvc_set_pipeline is ignored.  out[f] takes out_f samples; out_len [F] (may be NULL) is written.  So the result is, bit for bit, the composition:
 * gather per file, rvc_reset_state, rvc_infer_batch per batch in the packed order, rvc_sola_stitch per file; with one file it is rvc_convert's.
 * Statuses, in this order: the three *_NOT_LOADED as for rvc_convert, before any argument is looked at; RVC_SHAPE with a message for F out of range, n NULL,
 * an empty recording, the geometry errors of rvc_convert, the totals above; for auto-transpose in force (rvc_set_auto_transpose: it would take one
 * multiplier per file) and for an f0 curve set (rvc_set_f0_curve: a curve belongs to one recording); then every out_len[f] is written; a short cap[f] (or
 * cap NULL); a NULL pointer among pcm16k, out and their entries.  Nothing is launched on a refused call.  After a completed call rvc_convert_info and
 * rvc_convert_f0 answer as before any conversion has completed. */
/* host only, pure: windows [F] and out_samples [F] per file, totals = {Wtot, sum of out_samples}; any of the three may be NULL */
rvc_status rvc_convert_many_geometry(const size_t *n16k, size_t n_files, size_t sample_rate, size_t k, size_t context, size_t crossfade, size_t *windows,
                                     size_t *out_samples, size_t totals[2]);
rvc_status rvc_convert_many(rvc_engine *e, const float *const *pcm16k, const size_t *n, size_t n_files, size_t k, size_t context, size_t crossfade,
                            int32_t pitch_shift, int highpass, float *const *out, const size_t *cap, size_t *out_len);
/* of the last completed rvc_convert_many: Wtot, the batches, the SOLA offset of every window in global window order (the first cap_offsets of them), device
   ms = {high-pass, gather + model, stitch, total} as rvc_convert_info's; any pointer may be NULL.  RVC_SHAPE before one has completed */
rvc_status rvc_convert_many_info(rvc_engine *e, size_t *windows_total, size_t *batches, int32_t *offsets, size_t cap_offsets, double ms[4]);
/* rvc_sola_stitch for several files at once, the stitch kernels of rvc_convert_many on host buffers: windows [Wtot][window_len] laid end to end, file f
   holding windows_per_file[f] >= 1 of them, every file's tail starting as zeros: out [Wtot][frame], offsets [Wtot] (may be NULL).  Equal to rvc_sola_stitch
   of each file's windows, bit for bit.  rvc_sola_stitch's limits; 1 <= n_files <= 65536, Wtot <= 2^24, else RVC_SHAPE */
rvc_status rvc_sola_stitch_many(rvc_engine *e, const float *windows, const size_t *windows_per_file, size_t n_files, size_t window_len, size_t sola_len,
                                size_t search, size_t frame, float *out, int32_t *offsets);

/* ---- a pitch per recording for rvc_convert_many (Applio's batch mode proposes a pitch per file) ---- */
/* rvc_analyze_f0_many: rvc_analyze_f0 of F recordings in one call.  hz[f] takes exactly the rows rvc_analyze_f0 gives file f alone, Nf_f = ceil(N_f / 160),
 * bit for bit; n_frames [F] (may be NULL) is written.  The windows of all files are packed as rvc_convert_many packs them -- global window order, S =
 * rvc_set_streams per batch through ONE pitch-only plan, only the last batch padded -- all signals go up once, highpass != 0 filters each file on its own, and
 * with the silence gate on the active windows of all files are compacted; the rows of skipped windows are 0.  The call begins and ends with what
 * rvc_reset_state does.  Needs an f0 method only.  Statuses in rvc_convert_many's order: RVC_F0_NOT_LOADED before any argument is looked at; RVC_SHAPE with a
 * message for F out of range, n NULL, an empty recording, a bad geometry, the totals; then n_frames is written; a short cap[f] (or cap NULL); a NULL pointer
 * among pcm16k, hz and their entries.  Nothing is launched on a refused call. */
rvc_status rvc_analyze_f0_many(rvc_engine *e, const float *const *pcm16k, const size_t *n, size_t n_files, size_t k, size_t context, size_t crossfade,
                               int highpass, float *const *hz, const size_t *cap, size_t *n_frames);
/* rvc_f0_stats_many: rvc_f0_stats of every file's rows, bit for bit, in one launch.  hz holds the files' rows end to end, rows_per_file [F] their counts;
 * out_hz [F][nq], voiced [F] (may be NULL).  One workgroup per file runs the radix select with its histograms in LDS; only integers are summed.
 * RVC_SHAPE: F outside [1, 65536], a file without rows, more than 2^30 rows in all, rvc_f0_stats's limits for nq and the quantiles, a NULL buffer. */
rvc_status rvc_f0_stats_many(rvc_engine *e, const float *hz, const size_t *rows_per_file, size_t n_files, const double *quantile, size_t nq, float *out_hz,
                             size_t *voiced);
/* Two engine-wide settings, kept over model loads and read by rvc_convert_many ONLY (rvc_set_auto_transpose keeps its meaning, and rvc_convert_many stays
 * refused while it is in force).  rvc_set_convert_many_pitch: one transpose per file of the next calls, each finite and in [-24, 24] semitones (else RVC_SHAPE,
 * state unchanged); NULL or n_files = 0 clears the list.  A list whose length differs from a call's n_files makes that call RVC_SHAPE with a message; nothing is
 * launched.  rvc_set_convert_many_auto_transpose: rvc_set_auto_transpose's arguments and checks, target_hz = 0 (the default) = off.
 * With either on and a model with pitch guidance, rvc_convert_many runs, behind the high-pass and the silence gate and in front of its first batch, the
 * analysis of rvc_analyze_f0_many on the signals the model will see with the call's own k, context and crossfade; takes the lower median m_f and the voiced
 * count v_f of every file in one launch (rvc_f0_stats_many at p = 0.5) and brings them down in one copy; computes on the host in double
 * a_f = 12 log2(target / m_f) rounded to the step (ties to even) and clamped to [-limit, limit] -- 0 with the target off or v_f = 0 -- and
 * t_f = semitones[f] + a_f; and starts the conversion proper from the reset state.  In every batch a stream that holds a window of file f (under the silence
 * gate: the window the compaction put there) takes the factor (float)2^(t_f / 12) behind its own rvc_set_pitch_semitones factor; t_f = 0 multiplies by
 * nothing, padded streams take nothing.  The factor is no part of a plan's identity and is gone on every way out of the call.  So with the engine's own
 * semitones at 0 the result is, bit for bit, rvc_convert_many's composition with rvc_set_pitch_semitones_stream(s, t_f(s)) (0 for a padded stream) in front
 * of each rvc_infer_batch.  A model without pitch guidance skips all of it.  rvc_convert_many_info's total includes the pass.
 * rvc_convert_many_pitch_info: of the last rvc_convert_many that ran the pass, per file (the first cap_files of them) m_f, v_f, a_f, t_f, and device
 * ms = {analysis, select}; any pointer may be NULL; RVC_SHAPE before one has. */
rvc_status rvc_set_convert_many_pitch(rvc_engine *e, const double *semitones, size_t n_files);
rvc_status rvc_set_convert_many_auto_transpose(rvc_engine *e, double target_hz, int step, double limit);
rvc_status rvc_convert_many_auto_transpose(rvc_engine *e, double *target_hz, int *step, double *limit);
rvc_status rvc_convert_many_pitch_info(rvc_engine *e, float *median_hz, size_t *voiced, double *auto_semitones, double *total_semitones, size_t cap_files,
                                       double ms[2]);

/* ---- the file converter's silence gate (the upstream client's response threshold, slicer2's job) ---- */
/* Off by default.  With a threshold set, rvc_convert*, rvc_convert_file* (on the resampled and filtered signal), rvc_convert_many, rvc_analyze_f0* and the
 * analysis pass of auto-transpose measure the signal the model will see and run only the windows that hold something.  In 10 ms frames of 160 samples, the
 * signal x zero-extended beyond [0, N), Nf = ceil(N / 160):
 *   frame i is LOUD iff 20 log10(max(rms(x[160 i, 160 i + 640)), 1e-5)) >= threshold_db -- rvc_session_set_input_gate's measure --, decided as
 *       sumsq >= 640 max(10^(threshold_db / 10), 1e-10) with the sum in fp64 in a fixed order;
 *   frame i is KEPT iff a loud frame j has |i - j| <= hang_frames;
 *   window w is ACTIVE iff a kept frame lies in [w H, w H + H + X + Q) n [0, Nf), the frames its return_length covers.
 * The active windows are compacted in order: the j-th of them runs on stream j % S of batch j / S -- across files, in global window order, for
 * rvc_convert_many -- and only the last batch is padded with all-zero windows.  A skipped window is neither gathered nor inferred: return_length zc exact zeros
 * take its place in the unchanged stitch chain, and its f0 rows are 0 in rvc_convert_f0, rvc_analyze_f0 and the auto-transpose analysis.  The result is, bit
 * for bit, the composition: gather, rvc_reset_state, rvc_infer_batch per compacted batch, zero windows inserted at the skipped positions, rvc_sola_stitch (per
 * file: rvc_sola_stitch_many).  Noise counters follow the place, so this is NOT the ungated output with holes.  rvc_convert_info / rvc_convert_many_info report
 * every window (offsets of skipped ones included) and the batches actually run; a call without an active window runs no batch and no model kernel and returns
 * zeros with RVC_OK.  An f0 curve acts on the windows that run, by absolute frame.  The streaming session and the index builder never read the setting.
 * rvc_set_convert_silence: engine-wide, kept over model loads; threshold_db <= -60 = off (the session gate's convention), hang_frames in [0, 1000]; NaN or a
 * hang out of range: RVC_SHAPE, state unchanged.  rvc_convert_silence reads the setting back.  rvc_convert_silence_info: of the last completed call that ran
 * with the gate (rvc_silence_map included) -- windows run and skipped, loud and kept frames, device ms of the gate's own kernels; RVC_SHAPE before one has.
 * rvc_silence_map: the analysis alone on host buffers, with its own threshold (applied as given) and hang; needs no model; sample_rate only enters the
 * geometry check (a multiple of 100).  frame_loud / frame_kept [Nf] (cap_frames), window_active [W] and window_place [W] (cap_windows; place = the window's
 * rank among the active ones, -1 = skipped); any of the four may be NULL; RVC_SHAPE for n = 0, NaN, a bad hang or geometry, a short cap of a given buffer. */
rvc_status rvc_set_convert_silence(rvc_engine *e, double threshold_db, int hang_frames);
rvc_status rvc_convert_silence(rvc_engine *e, double *threshold_db, int *hang_frames);
rvc_status rvc_convert_silence_info(rvc_engine *e, size_t *windows_run, size_t *windows_skipped, size_t *frames_loud, size_t *frames_kept, double *ms_analysis);
rvc_status rvc_silence_map(rvc_engine *e, const float *pcm16k, size_t n, double threshold_db, int hang_frames, size_t k, size_t context, size_t crossfade,
                           size_t sample_rate, uint8_t *frame_loud, uint8_t *frame_kept, size_t cap_frames, uint8_t *window_active, int32_t *window_place,
                           size_t cap_windows);

/* ---- what THIS GPU sustains, measured in-run (bench.py; boxes of one pool differ by ~10 % on matrix-core-bound work) ---- */
/* rvc_calibrate: ~50 ms of device time.  A bare v_mfma_f32_32x32x2_f32 stream on every SIMD (four waves per SIMD, non-zero operands) -> fp32 matrix-core
 * TFLOP/s actually reached and the shader clock it ran at (s_memtime cycles per s_memrealtime tick); a float4 read stream over 1 GiB -> HBM TB/s. */
typedef struct {
    double mfma_f32_tflops, mfma_sclk_mhz, mfma_ms;
    double hbm_read_tbs, hbm_sclk_mhz;
    double ms_total;
    int compute_units;
} rvc_calibration;
rvc_status rvc_calibrate(int device, rvc_calibration *out);
/* Effective shader clock WHILE other work runs: start leaves eight sleeping one-wave workgroups (one per XCD) on a stream of their own that count shader
 * cycles against the 100 MHz real-time counter; stop ends them and reports the mean / minimum over the XCDs and the seconds observed.  The waves leave
 * by themselves after 20 s (do not run it under a profiler that serialises dispatches).  One monitor per device. */
rvc_status rvc_clock_monitor_start(int device);
rvc_status rvc_clock_monitor_stop(int device, double *sclk_mhz_mean, double *sclk_mhz_min, double *seconds);

/* ---- measurement / debugging ---- */
/* total milliseconds of the last infer measured with HIP events on the engine's stream */
float rvc_last_gpu_ms(rvc_engine *e);
/* HIP-event timing of the dominant (implicit-GEMM) kernel class over the last infer call:
 * number of launches, summed milliseconds, summed algorithmic FLOPs (2*M*N*K per launch) */
rvc_status rvc_profile_last(rvc_engine *e, int *launches, double *kernel_ms, double *flops);
/* same for the HBM-bound retrieval launch (knn_scan_select_kernel: scan, select, exact re-rank and blend in one launch): launches, summed ms, summed algorithmic bytes (index size per pass) */
rvc_status rvc_profile_last_knn(rvc_engine *e, int *launches, double *kernel_ms, double *bytes);
void rvc_set_profile(rvc_engine *e, int on);
/* named intermediate tensor of stream 0 of the last call, contiguous row-major (tests).  on = 1: taps on the EXPLICIT plan (every
 * LayerNorm its own launch, WaveNets layer by layer: each tap has the oracle's meaning); on = 2: taps on the PRODUCTION plan (folded
 * LayerNorms, composed WaveNets: tensors that are not yet normalised there carry a ".raw" suffix); 0 = off */
void rvc_enable_taps(rvc_engine *e, int on);
rvc_status rvc_get_tap(rvc_engine *e, const char *name, float *out, size_t cap, size_t *n);
void rvc_get_pitch_cache(rvc_engine *e, int stream, float *out1024);
/* raw device pointer of the engine's weights/index for RCCL broadcast at load (config 5) */
void *rvc_index_device_ptr(rvc_engine *e, size_t *bytes);
int rvc_device(rvc_engine *e);
const char *rvc_version(void);

#ifdef __cplusplus
}
#endif
#endif
