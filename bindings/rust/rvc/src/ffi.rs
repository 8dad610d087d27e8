//! `extern "C"` declarations for `include/rvc_mi355x.h` (hand-written; `bindgen include/rvc_mi355x.h` gives the same items).
//! Names, argument order and integer widths follow the header one to one: `size_t` = `usize`, `int` = `c_int`,
//! `rvc_status` = `c_int` (0 ok, 1 ModelNotLoaded, 2 ContentvecNotLoaded, 3 F0NotLoaded, 4 Backend, 5 Shape, 6 Panic).
#![allow(dead_code)]
use std::os::raw::{c_char, c_double, c_float, c_int, c_longlong, c_void};

#[repr(C)]
pub struct RvcEngine {
    _private: [u8; 0],
}
#[repr(C)]
pub struct RvcResampler {
    _private: [u8; 0],
}
#[repr(C)]
pub struct RvcDenoiser {
    _private: [u8; 0],
}
#[repr(C)]
pub struct RvcSession {
    _private: [u8; 0],
}
/// rvc_calibration (include/rvc_mi355x.h)
#[repr(C)]
pub struct RvcCalibration {
    pub mfma_f32_tflops: c_double,
    pub mfma_sclk_mhz: c_double,
    pub mfma_ms: c_double,
    pub hbm_read_tbs: c_double,
    pub hbm_sclk_mhz: c_double,
    pub ms_total: c_double,
    pub compute_units: c_int,
}

pub const RVC_OK: c_int = 0;
pub const RVC_MODEL_NOT_LOADED: c_int = 1;
pub const RVC_CONTENTVEC_NOT_LOADED: c_int = 2;
pub const RVC_F0_NOT_LOADED: c_int = 3;
pub const RVC_BACKEND: c_int = 4;
pub const RVC_SHAPE: c_int = 5;
pub const RVC_PANIC: c_int = 6;
pub const RVC_RCCL_UNIQUE_ID_BYTES: usize = 128;
pub const RVC_F0_RMVPE: c_int = 1;
pub const RVC_F0_YIN: c_int = 2;
pub const RVC_F0_CREPE: c_int = 4;
pub const RVC_F0_CREPE_TINY: c_int = 5;
pub const RVC_F0_FCPE: c_int = 7;
pub const RVC_F0_HYBRID: c_int = 8;
pub const RVC_F0_PM: c_int = 9;
pub const RVC_HYBRID_VOTE: c_int = 0;
pub const RVC_HYBRID_MEDIAN: c_int = 1;
pub const RVC_CREPE_VITERBI: c_int = 0;
pub const RVC_CREPE_ARGMAX: c_int = 1;
pub const RVC_DENOISE_INPUT: c_int = 0;
pub const RVC_DENOISE_OUTPUT: c_int = 1;

extern "C" {
    // ---- RvcInfer (rvc/src/rvc.rs:30-220)
    pub fn rvc_create(data_path: *const c_char, device: c_int, out: *mut *mut RvcEngine) -> c_int;
    pub fn rvc_destroy(e: *mut RvcEngine);
    pub fn rvc_load_contentvec(e: *mut RvcEngine, model_version: c_int) -> c_int;
    pub fn rvc_load_model(e: *mut RvcEngine, model_path: *const c_char) -> c_int;
    pub fn rvc_load_f0(e: *mut RvcEngine, pitch_algorithm: c_int) -> c_int;
    pub fn rvc_unload_model(e: *mut RvcEngine);
    pub fn rvc_hubert(e: *mut RvcEngine, input: *const c_float, n: usize, out: *mut c_float, cap: usize, dims: *mut usize) -> c_int;
    pub fn rvc_extract_feature(e: *mut RvcEngine, input: *const c_float, n: usize, out: *mut c_float, cap: usize, dims: *mut usize) -> c_int;
    pub fn rvc_pitch(e: *mut RvcEngine, input: *const c_float, n: usize, pitch_shift: i32, sample_frame_16k_size: usize,
                     out: *mut c_float, cap: usize, out_len: *mut usize) -> c_int;
    pub fn rvc_infer(e: *mut RvcEngine, input: *const c_float, n: usize, sample_frame_16k_size: usize, has_pitch_shift: c_int,
                     pitch_shift: i32, skip_head: u32, return_length: u32, out: *mut c_float, cap: usize, out_len: *mut usize) -> c_int;
    pub fn rvc_last_error_message(e: *mut RvcEngine) -> *const c_char;
    // ---- f0 method: RVC_F0_RMVPE (= rvc_load_f0), RVC_F0_YIN or RVC_F0_PM (no weight file)
    pub fn rvc_load_f0_method(e: *mut RvcEngine, method: c_int) -> c_int;
    pub fn rvc_f0_method(e: *mut RvcEngine) -> c_int;
    pub fn rvc_model_has_f0(e: *mut RvcEngine) -> c_int;
    // ---- speakers of a multi-speaker model: the table's rows, the speaker by id, a blend of up to 8 ids, the mix in force
    pub fn rvc_model_speakers(e: *mut RvcEngine) -> c_int;
    pub fn rvc_set_speaker(e: *mut RvcEngine, sid: c_int) -> c_int;
    pub fn rvc_set_speaker_mix(e: *mut RvcEngine, sid: *const i32, weight: *const f64, n: usize) -> c_int;
    pub fn rvc_speaker_mix(e: *mut RvcEngine, sid: *mut i32, weight: *mut f64, cap: usize, n: *mut usize) -> c_int;
    // ---- CREPE (RVC_F0_CREPE / RVC_F0_CREPE_TINY: <data>/f0/crepe-full.rvcw / crepe-tiny.rvcw): its decoder, RVC_CREPE_VITERBI (default) or RVC_CREPE_ARGMAX
    pub fn rvc_set_crepe_decoder(e: *mut RvcEngine, decoder: c_int) -> c_int;
    pub fn rvc_crepe_decoder(e: *mut RvcEngine) -> c_int;
    // ---- FCPE (RVC_F0_FCPE: <data>/f0/fcpe.rvcw): its voicing threshold in [0, 1), default 0.006
    pub fn rvc_set_fcpe_threshold(e: *mut RvcEngine, threshold: c_double) -> c_int;
    pub fn rvc_fcpe_threshold(e: *mut RvcEngine) -> c_double;
    // ---- hybrid f0 (RVC_F0_HYBRID): 1 to 4 distinct members, the first the lead, combined per frame under RVC_HYBRID_VOTE (default) or RVC_HYBRID_MEDIAN
    pub fn rvc_load_f0_hybrid(e: *mut RvcEngine, methods: *const c_int, n: c_int, mode: c_int) -> c_int;
    pub fn rvc_f0_hybrid(e: *mut RvcEngine, methods: *mut c_int, cap: c_int, mode: *mut c_int) -> c_int;

    // ---- retrieval index, noise seed, state
    pub fn rvc_load_index(e: *mut RvcEngine, vectors: *const c_float, n: usize, dim: usize) -> c_int;
    pub fn rvc_load_index_device(e: *mut RvcEngine, d_vectors: *const c_void, n: usize, dim: usize) -> c_int;
    pub fn rvc_set_index_rate(e: *mut RvcEngine, rate: c_float);
    pub fn rvc_get_knn(e: *mut RvcEngine, idx: *mut i32, dist: *mut c_float, cap_rows: usize, rows: *mut usize) -> c_int;
    // IVF-probed retrieval: the structure of an IndexIVFFlat file over the loaded index, and how many lists a query probes (0 = flat search)
    pub fn rvc_set_index_ivf(e: *mut RvcEngine, centroids: *const c_float, nlist: usize, dim: usize, assign: *const i32, n: usize) -> c_int;
    pub fn rvc_set_index_nprobe(e: *mut RvcEngine, nprobe: c_int) -> c_int;
    pub fn rvc_index_nprobe(e: *mut RvcEngine) -> c_int;
    // neighbours blended per query: 4 (default) or upstream's 8; rvc_get_knn then writes idx / dist [rows][k]
    pub fn rvc_set_index_k(e: *mut RvcEngine, k: c_int) -> c_int;
    pub fn rvc_index_k(e: *mut RvcEngine) -> c_int;
    pub fn rvc_index_ivf_info(e: *mut RvcEngine, nlist: *mut usize, longest_list: *mut usize, empty_lists: *mut usize) -> c_int;
    // k-means training of an IVF structure for the loaded index, its report, and the attached structure read back
    pub fn rvc_train_index_ivf(e: *mut RvcEngine, nlist: usize, iters: c_int, init_rows: *const i32, seed: u32) -> c_int;
    pub fn rvc_index_ivf_train_info(e: *mut RvcEngine, iters_run: *mut c_int, moved_last: *mut usize, objective: *mut f64, cap: usize, n_obj: *mut usize, ms: *mut f64) -> c_int;
    pub fn rvc_get_index_ivf(e: *mut RvcEngine, centroids: *mut c_float, cap_centroid_floats: usize, assign: *mut i32, cap_rows: usize) -> c_int;
    // index builder: ContentVec frames of a voice's recordings into a row store on the device (window 0 = 48 000 samples, capacity_hint 0 = 4096 rows),
    // then installed as the engine's index (max_rows = reduce_to = 0: above 200 000 rows, 10 000 k-means centres)
    pub fn rvc_index_build_begin(e: *mut RvcEngine, window: usize, capacity_hint: usize) -> c_int;
    pub fn rvc_index_build_add(e: *mut RvcEngine, pcm16k: *const c_float, n: usize, rows_added: *mut usize) -> c_int;
    pub fn rvc_index_build_add_device(e: *mut RvcEngine, d_pcm16k: *const c_void, n: usize, rows_added: *mut usize) -> c_int;
    pub fn rvc_index_build_info(e: *mut RvcEngine, rows: *mut usize, capacity: *mut usize, windows: *mut usize, dropped_nonfinite: *mut usize, ms: *mut f64) -> c_int;
    pub fn rvc_index_build_finish(e: *mut RvcEngine, max_rows: usize, reduce_to: usize, iters: c_int, seed: u32) -> c_int;
    pub fn rvc_index_build_abort(e: *mut RvcEngine);
    // whole-recording conversion: windows of one geometry through the batched infer path, SOLA-stitched on the device (k, context, crossfade: 0 = 14 / 48 / 5
    // frames); geometry out[8] = {windows, n, sample_frame_16k_size, skip_head, return_length, hop, zc, output samples}; info ms[4] = {high-pass, gather + model,
    // stitch, total}
    pub fn rvc_convert_geometry(n16k: usize, sample_rate: usize, k: usize, context: usize, crossfade: usize, out: *mut usize) -> c_int;
    pub fn rvc_convert(e: *mut RvcEngine, pcm16k: *const c_float, n: usize, k: usize, context: usize, crossfade: usize, pitch_shift: i32, highpass: c_int,
                       out: *mut c_float, cap: usize, out_len: *mut usize) -> c_int;
    pub fn rvc_convert_device(e: *mut RvcEngine, d_pcm16k: *const c_void, n: usize, k: usize, context: usize, crossfade: usize, pitch_shift: i32, highpass: c_int,
                              d_out: *mut c_void, cap: usize, out_len: *mut usize) -> c_int;
    pub fn rvc_convert_info(e: *mut RvcEngine, windows: *mut usize, batches: *mut usize, offsets: *mut i32, cap_offsets: usize, ms: *mut f64) -> c_int;
    pub fn rvc_sola_stitch(e: *mut RvcEngine, windows: *const c_float, n_windows: usize, window_len: usize, sola_len: usize, search: usize, frame: usize,
                           out: *mut c_float, offsets: *mut i32) -> c_int;
    pub fn rvc_highpass(e: *mut RvcEngine, pcm16k: *const c_float, n: usize, out: *mut c_float) -> c_int;
    // a file at any rate, with the volume envelope: geometry out[4] = {o, n, w, N_out}; info ms[7] = {resample in, high-pass,
    // gather + model, stitch, envelope, resample out, total}
    pub fn rvc_resample_geometry(rate_in: usize, rate_out: usize, n_in: usize, out: *mut usize) -> c_int;
    pub fn rvc_resample(e: *mut RvcEngine, input: *const c_float, n_in: usize, rate_in: usize, rate_out: usize, out: *mut c_float, cap: usize, n_out: *mut usize) -> c_int;
    pub fn rvc_resample_device(e: *mut RvcEngine, d_in: *const c_void, n_in: usize, rate_in: usize, rate_out: usize, d_out: *mut c_void, cap: usize,
                               n_out: *mut usize) -> c_int;
    pub fn rvc_change_rms(e: *mut RvcEngine, src: *const c_float, n_src: usize, rate_src: usize, y: *mut c_float, n_y: usize, rate_y: usize, rate: f64) -> c_int;
    pub fn rvc_convert_file(e: *mut RvcEngine, pcm: *const c_float, n: usize, rate_in: usize, k: usize, context: usize, crossfade: usize, pitch_shift: i32,
                            highpass: c_int, rms_mix_rate: f64, rate_out: usize, out: *mut c_float, cap: usize, out_len: *mut usize) -> c_int;
    pub fn rvc_convert_file_device(e: *mut RvcEngine, d_pcm: *const c_void, n: usize, rate_in: usize, k: usize, context: usize, crossfade: usize, pitch_shift: i32,
                                   highpass: c_int, rms_mix_rate: f64, rate_out: usize, d_out: *mut c_void, cap: usize, out_len: *mut usize) -> c_int;
    pub fn rvc_convert_file_info(e: *mut RvcEngine, ms: *mut f64, rate_out: *mut usize, peak: *mut c_float) -> c_int;
    // many recordings in one call: declared for the header's sake, the shim has no method for them yet
    pub fn rvc_convert_many_geometry(n16k: *const usize, n_files: usize, sample_rate: usize, k: usize, context: usize, crossfade: usize, windows: *mut usize,
                                     out_samples: *mut usize, totals: *mut usize) -> c_int;
    pub fn rvc_convert_many(e: *mut RvcEngine, pcm16k: *const *const c_float, n: *const usize, n_files: usize, k: usize, context: usize, crossfade: usize,
                            pitch_shift: i32, highpass: c_int, out: *const *mut c_float, cap: *const usize, out_len: *mut usize) -> c_int;
    pub fn rvc_convert_many_info(e: *mut RvcEngine, windows_total: *mut usize, batches: *mut usize, offsets: *mut i32, cap_offsets: usize, ms: *mut f64) -> c_int;
    pub fn rvc_sola_stitch_many(e: *mut RvcEngine, windows: *const c_float, windows_per_file: *const usize, n_files: usize, window_len: usize, sola_len: usize,
                                search: usize, frame: usize, out: *mut c_float, offsets: *mut i32) -> c_int;
    // a pitch per recording for rvc_convert_many: the packed analysis, the segmented select, a transpose list and an auto-transpose
    // target read by rvc_convert_many alone; declared for the header's sake
    pub fn rvc_analyze_f0_many(e: *mut RvcEngine, pcm16k: *const *const c_float, n: *const usize, n_files: usize, k: usize, context: usize, crossfade: usize,
                               highpass: c_int, hz: *const *mut c_float, cap: *const usize, n_frames: *mut usize) -> c_int;
    pub fn rvc_f0_stats_many(e: *mut RvcEngine, hz: *const c_float, rows_per_file: *const usize, n_files: usize, quantile: *const c_double, nq: usize,
                             out_hz: *mut c_float, voiced: *mut usize) -> c_int;
    pub fn rvc_set_convert_many_pitch(e: *mut RvcEngine, semitones: *const c_double, n_files: usize) -> c_int;
    pub fn rvc_set_convert_many_auto_transpose(e: *mut RvcEngine, target_hz: c_double, step: c_int, limit: c_double) -> c_int;
    pub fn rvc_convert_many_auto_transpose(e: *mut RvcEngine, target_hz: *mut c_double, step: *mut c_int, limit: *mut c_double) -> c_int;
    pub fn rvc_convert_many_pitch_info(e: *mut RvcEngine, median_hz: *mut c_float, voiced: *mut usize, auto_semitones: *mut c_double,
                                       total_semitones: *mut c_double, cap_files: usize, ms: *mut c_double) -> c_int;
    // the file converter's silence gate: threshold <= -60 dB = off, hang 0..1000 frames; declared for the header's sake
    pub fn rvc_set_convert_silence(e: *mut RvcEngine, threshold_db: c_double, hang_frames: c_int) -> c_int;
    pub fn rvc_convert_silence(e: *mut RvcEngine, threshold_db: *mut c_double, hang_frames: *mut c_int) -> c_int;
    pub fn rvc_convert_silence_info(e: *mut RvcEngine, windows_run: *mut usize, windows_skipped: *mut usize, frames_loud: *mut usize, frames_kept: *mut usize,
                                    ms_analysis: *mut c_double) -> c_int;
    pub fn rvc_silence_map(e: *mut RvcEngine, pcm16k: *const c_float, n: usize, threshold_db: c_double, hang_frames: c_int, k: usize, context: usize, crossfade: usize,
                           sample_rate: usize, frame_loud: *mut u8, frame_kept: *mut u8, cap_frames: usize, window_active: *mut u8, window_place: *mut i32,
                           cap_windows: usize) -> c_int;
    pub fn rvc_set_noise_seed(e: *mut RvcEngine, seed: u32, stream_id: u32);
    pub fn rvc_reset_state(e: *mut RvcEngine);

    // ---- formant shift (the plugin's resonance shift), semitones in [-5, 5]
    pub fn rvc_set_formant_shift(e: *mut RvcEngine, semitones: f64) -> c_int;
    pub fn rvc_set_formant_shift_stream(e: *mut RvcEngine, stream: c_int, semitones: f64) -> c_int;
    pub fn rvc_formant_geometry(return_length: usize, sample_rate: usize, semitones: f64, out: *mut usize) -> c_int;
    // ---- pitch controls: transpose in semitones [-24, 24], voiced range in Hz, f0 median radius 0..7, snap to a 12-bit pitch-class mask
    pub fn rvc_set_pitch_semitones(e: *mut RvcEngine, semitones: f64) -> c_int;
    pub fn rvc_set_pitch_semitones_stream(e: *mut RvcEngine, stream: c_int, semitones: f64) -> c_int;
    pub fn rvc_set_f0_range(e: *mut RvcEngine, lo_hz: f64, hi_hz: f64) -> c_int;
    pub fn rvc_set_f0_range_stream(e: *mut RvcEngine, stream: c_int, lo_hz: f64, hi_hz: f64) -> c_int;
    pub fn rvc_set_f0_median(e: *mut RvcEngine, radius: c_int) -> c_int;
    pub fn rvc_set_f0_median_stream(e: *mut RvcEngine, stream: c_int, radius: c_int) -> c_int;
    pub fn rvc_set_f0_snap(e: *mut RvcEngine, pitch_class_mask: u32, strength: f64) -> c_int;
    pub fn rvc_set_f0_snap_stream(e: *mut RvcEngine, stream: c_int, pitch_class_mask: u32, strength: f64) -> c_int;
    // ---- consonant protection (upstream's `protect`): [0, 0.5], 0.5 = off; unvoiced rows are mixed back towards the raw ContentVec features
    pub fn rvc_set_protect(e: *mut RvcEngine, protect: f64) -> c_int;
    pub fn rvc_set_protect_stream(e: *mut RvcEngine, stream: c_int, protect: f64) -> c_int;
    pub fn rvc_set_f0_override_stream(e: *mut RvcEngine, stream: c_int, hz: *const c_float, n: usize) -> c_int;
    pub fn rvc_set_f0_override_hold(e: *mut RvcEngine, hold: c_int) -> c_int;
    pub fn rvc_set_f0_curve(e: *mut RvcEngine, t_sec: *const f64, hz: *const c_float, n: usize) -> c_int;
    pub fn rvc_f0_curve_grid(e: *mut RvcEngine, n_frames: usize, out: *mut c_float, cap: usize) -> c_int;
    pub fn rvc_convert_f0(e: *mut RvcEngine, hz: *mut c_float, cap: usize, n_frames: *mut usize) -> c_int;
    // f0 analysis of a whole recording (no synthesizer), exact order statistics of the voiced rows, auto-transpose of the file converter (target 0 = off;
    // step 0 / 1 / 12; limit 0..24 semitones)
    pub fn rvc_analyze_f0(e: *mut RvcEngine, pcm16k: *const c_float, n: usize, k: usize, context: usize, crossfade: usize, highpass: c_int, hz: *mut c_float,
                          cap: usize, n_frames: *mut usize) -> c_int;
    pub fn rvc_analyze_f0_device(e: *mut RvcEngine, d_pcm16k: *const c_void, n: usize, k: usize, context: usize, crossfade: usize, highpass: c_int,
                                 d_hz: *mut c_void, cap: usize, n_frames: *mut usize) -> c_int;
    pub fn rvc_f0_stats(e: *mut RvcEngine, hz: *const c_float, n: usize, quantile: *const c_double, nq: usize, out_hz: *mut c_float, voiced: *mut usize) -> c_int;
    pub fn rvc_f0_stats_stream(e: *mut RvcEngine, stream: c_int, quantile: *const c_double, nq: usize, out_hz: *mut c_float, voiced: *mut usize) -> c_int;
    pub fn rvc_set_auto_transpose(e: *mut RvcEngine, target_hz: c_double, step: c_int, limit: c_double) -> c_int;
    pub fn rvc_auto_transpose(e: *mut RvcEngine, target_hz: *mut c_double, step: *mut c_int, limit: *mut c_double) -> c_int;
    pub fn rvc_auto_transpose_info(e: *mut RvcEngine, median_hz: *mut c_float, voiced: *mut usize, semitones: *mut c_double, ms: *mut c_double) -> c_int;

    // ---- multi-GPU: the one collective (index broadcast at load, RCCL over xGMI)
    pub fn rvc_rccl_unique_id(id128: *mut c_void) -> c_int;
    pub fn rvc_index_broadcast(e: *mut RvcEngine, unique_id128: *const c_void, rank: c_int, world: c_int,
                               vectors: *const c_float, n: usize, dim: usize) -> c_int;
    pub fn rvc_rccl_available() -> c_int;
    pub fn rvc_index_broadcast_info(e: *mut RvcEngine, ms: *mut f64, ranks: *mut c_int) -> c_int;

    // ---- many streams per GPU
    pub fn rvc_set_streams(e: *mut RvcEngine, n_streams: c_int) -> c_int;
    pub fn rvc_infer_batch(e: *mut RvcEngine, input: *const c_float, n: usize, sample_frame_16k_size: usize, pitch_shift: i32,
                           skip_head: u32, return_length: u32, out: *mut c_float, cap_per_stream: usize, out_len: *mut usize) -> c_int;
    pub fn rvc_infer_batch_v(e: *mut RvcEngine, input: *const c_float, n: usize, sample_frame_16k_size: usize, pitch_shift: *const i32,
                             skip_head: u32, return_length: u32, out: *mut c_float, cap_per_stream: usize, out_len: *mut usize) -> c_int;
    pub fn rvc_infer_device_v(e: *mut RvcEngine, d_input: *const c_void, n: usize, sample_frame_16k_size: usize, pitch_shift: *const i32,
                              skip_head: u32, return_length: u32, d_out: *mut c_void, cap_per_stream: usize, out_len: *mut usize, sync: c_int) -> c_int;
    pub fn rvc_infer_batch_g(e: *mut RvcEngine, inputs: *const *const c_float, n: *const usize, sample_frame_16k_size: *const usize, pitch_shift: *const i32,
                             skip_head: *const u32, return_length: *const u32, outs: *const *mut c_float, caps: *const usize, out_lens: *mut usize) -> c_int;
    pub fn rvc_infer_device(e: *mut RvcEngine, d_input: *const c_void, n: usize, sample_frame_16k_size: usize, pitch_shift: i32,
                            skip_head: u32, return_length: u32, d_out: *mut c_void, cap_per_stream: usize, out_len: *mut usize,
                            sync: c_int) -> c_int;
    pub fn rvc_synchronize(e: *mut RvcEngine) -> c_int;
    pub fn rvc_set_use_graph(e: *mut RvcEngine, on: c_int);
    pub fn rvc_set_pipeline(e: *mut RvcEngine, on: c_int);
    // plan cache (one plan per call geometry; LRU) and the retrieval's recovered hand-off time-outs
    pub fn rvc_set_plan_cache(e: *mut RvcEngine, n_plans: c_int) -> c_int;
    pub fn rvc_plan_cache_info(e: *mut RvcEngine, capacity: *mut c_int, cached: *mut c_int, builds: *mut c_longlong) -> c_int;
    pub fn rvc_retrieval_recoveries(e: *mut RvcEngine) -> c_longlong;
    pub fn rvc_set_gemm_precision(e: *mut RvcEngine, mode: c_int) -> c_int;
    // plan-time selection among eligible kernels / tiles by measurement (default on above 4 streams)
    pub fn rvc_set_plan_autotune(e: *mut RvcEngine, on: c_int) -> c_int;
    pub fn rvc_plan_autotune_info(e: *mut RvcEngine, tuned: *mut c_int, changed: *mut c_int, cache_hits: *mut c_int, tune_ms: *mut c_double,
                                  build_ms: *mut c_double) -> c_int;
    // what this GPU sustains, measured in-run (bare fp32-MFMA stream, HBM read stream), and the effective shader clock while other work runs
    pub fn rvc_calibrate(device: c_int, out: *mut RvcCalibration) -> c_int;
    pub fn rvc_clock_monitor_start(device: c_int) -> c_int;
    pub fn rvc_clock_monitor_stop(device: c_int, sclk_mhz_mean: *mut c_double, sclk_mhz_min: *mut c_double, seconds: *mut c_double) -> c_int;

    // ---- caller-side steps of the plugin (obs-rvc/src/rt_utils.rs, obs-rvc/src/lib.rs:236-260,659-795)
    pub fn rvc_envelop_mixing(e: *mut RvcEngine, input: *const c_float, output: *mut c_float, output_len: usize, sample_rate: usize,
                              mix_rate: c_double) -> c_int;
    pub fn rvc_sola_step(e: *mut RvcEngine, output: *mut c_float, output_len: usize, sola_buffer: *mut c_float, sola_len: usize,
                         search: usize, frame: usize, frame_out: *mut c_float, sola_offset: *mut usize) -> c_int;
    // the same step with a choice of crossfade (0 = linear, 1 = phase vocoder) and the session's input gate on host buffers
    pub fn rvc_sola_step_x(e: *mut RvcEngine, output: *mut c_float, output_len: usize, sola_buffer: *mut c_float, sola_len: usize,
                           search: usize, frame: usize, frame_out: *mut c_float, sola_offset: *mut usize, crossfade: c_int) -> c_int;
    pub fn rvc_input_gate(e: *mut RvcEngine, hist3zc: *const c_float, chunk: *const c_float, n: usize, sample_rate: usize,
                          threshold_db: c_double, out: *mut c_float, hist_out: *mut c_float) -> c_int;
    pub fn rvc_resampler_create(e: *mut RvcEngine, rate_in: usize, rate_out: usize, chunk_size_in: usize, out: *mut *mut RvcResampler) -> c_int;
    pub fn rvc_resampler_destroy(r: *mut RvcResampler);
    pub fn rvc_resampler_input_frames_next(r: *mut RvcResampler) -> usize;
    pub fn rvc_resampler_output_frames_max(r: *mut RvcResampler) -> usize;
    pub fn rvc_resampler_reset(r: *mut RvcResampler);
    pub fn rvc_resampler_process(r: *mut RvcResampler, input: *const c_float, n_in: usize, out: *mut c_float, cap: usize, n_out: *mut usize) -> c_int;
    pub fn rvc_resampler_process_device(r: *mut RvcResampler, d_in: *const c_void, d_out: *mut c_void, sync: c_int) -> c_int;
    // streaming spectral-gate noise reduction: strength in [0, 1] (0 = off, undelayed), threshold in [0, 16]; 10 ms delay; stream -1 = all
    pub fn rvc_denoiser_create(e: *mut RvcEngine, sample_rate: usize, n_streams: c_int, out: *mut *mut RvcDenoiser) -> c_int;
    pub fn rvc_denoiser_destroy(d: *mut RvcDenoiser);
    pub fn rvc_denoiser_reset(d: *mut RvcDenoiser);
    pub fn rvc_denoiser_set(d: *mut RvcDenoiser, stream: c_int, strength: c_double, threshold: c_double) -> c_int;
    pub fn rvc_denoiser_latency(d: *mut RvcDenoiser) -> usize;
    pub fn rvc_denoiser_process(d: *mut RvcDenoiser, input: *const c_float, n: usize, out: *mut c_float) -> c_int;
    pub fn rvc_denoiser_process_device(d: *mut RvcDenoiser, d_in: *const c_void, d_out: *mut c_void, n: usize, in_stride: usize, out_stride: usize,
                                       sync: c_int) -> c_int;
    pub fn rvc_session_create(e: *mut RvcEngine, sample_rate: usize, sample_length: c_double, crossfade_length: c_double,
                              extra_inference_time: c_double, model_output_sample_rate: usize, pitch_shift: i32, rms_mix_rate: c_double,
                              skip_inference: c_int, out: *mut *mut RvcSession) -> c_int;
    pub fn rvc_session_destroy(s: *mut RvcSession);
    pub fn rvc_session_frame_size(s: *mut RvcSession) -> usize;
    pub fn rvc_session_set_params(s: *mut RvcSession, pitch_shift: i32, rms_mix_rate: c_double);
    pub fn rvc_session_set_params_stream(s: *mut RvcSession, stream: c_int, pitch_shift: i32, rms_mix_rate: f64) -> c_int;
    pub fn rvc_session_set_crossfade(s: *mut RvcSession, mode: c_int) -> c_int;
    pub fn rvc_session_set_crossfade_stream(s: *mut RvcSession, stream: c_int, mode: c_int) -> c_int;
    pub fn rvc_session_set_input_gate(s: *mut RvcSession, threshold_db: c_double) -> c_int;
    pub fn rvc_session_set_input_gate_stream(s: *mut RvcSession, stream: c_int, threshold_db: c_double) -> c_int;
    pub fn rvc_session_set_noise_reduction(s: *mut RvcSession, side: c_int, strength: c_double, threshold: c_double) -> c_int;
    pub fn rvc_session_set_noise_reduction_stream(s: *mut RvcSession, stream: c_int, side: c_int, strength: c_double, threshold: c_double) -> c_int;
    pub fn rvc_session_geometry(s: *mut RvcSession, out: *mut i32);
    pub fn rvc_session_process(s: *mut RvcSession, input_sample: *const c_float, n: usize, output: *mut c_float, cap: usize,
                               sola_offset: *mut usize) -> c_int;

    // ---- measurement / debugging
    pub fn rvc_last_gpu_ms(e: *mut RvcEngine) -> c_float;
    pub fn rvc_profile_last(e: *mut RvcEngine, launches: *mut c_int, kernel_ms: *mut c_double, flops: *mut c_double) -> c_int;
    pub fn rvc_profile_last_knn(e: *mut RvcEngine, launches: *mut c_int, kernel_ms: *mut c_double, bytes: *mut c_double) -> c_int;
    pub fn rvc_set_profile(e: *mut RvcEngine, on: c_int);
    pub fn rvc_enable_taps(e: *mut RvcEngine, on: c_int);
    pub fn rvc_get_tap(e: *mut RvcEngine, name: *const c_char, out: *mut c_float, cap: usize, n: *mut usize) -> c_int;
    pub fn rvc_get_pitch_cache(e: *mut RvcEngine, stream: c_int, out1024: *mut c_float);
    pub fn rvc_index_device_ptr(e: *mut RvcEngine, bytes: *mut usize) -> *mut c_void;
    pub fn rvc_device(e: *mut RvcEngine) -> c_int;
    pub fn rvc_version() -> *const c_char;
}
