//! `RvcInfer` of the reference (`rvc/src/rvc.rs:18-220`) over `librvc_mi355x.so`: same method names, argument meaning, return
//! shapes and error behaviour; the three ONNX Runtime sessions, the mel / STFT front end, the pitch cache and `get_f0_post` now
//! live on the GPU behind one opaque handle.  One handle = one stream = one thread at a time, as `&mut self` already demanded.
use std::ffi::{CStr, CString};
use std::path::PathBuf;

use ndarray::{Array1, Array3, ArrayView1};
use rvc_common::{
    enums::{PitchAlgorithm, RvcModelVersion},
    errors::{BackendError, RvcInferError},
};

use crate::ffi;

pub struct RvcInfer {
    handle: *mut ffi::RvcEngine,
}

// The reference's RvcInfer is Send (ort::Session is); the engine handle may move between threads but is not re-entrant.
unsafe impl Send for RvcInfer {}

fn c_path(p: &PathBuf) -> CString {
    CString::new(p.to_string_lossy().as_bytes()).expect("path contains a NUL byte")
}

impl RvcInfer {
    fn message(&self) -> String {
        unsafe {
            let m = ffi::rvc_last_error_message(self.handle);
            if m.is_null() { String::new() } else { CStr::from_ptr(m).to_string_lossy().into_owned() }
        }
    }

    /// rvc_status -> the reference's error type (`rvc-common/src/errors.rs:2-8`).  `RVC_PANIC` marks inputs on which the
    /// reference itself panics (`rmvpe.rs:124` out-of-range gather, `rvc.rs:155` slice out of range): panic here too.
    fn check(&self, rc: i32) -> Result<(), RvcInferError> {
        match rc {
            ffi::RVC_OK => Ok(()),
            ffi::RVC_MODEL_NOT_LOADED => Err(RvcInferError::ModelNotLoaded),
            ffi::RVC_CONTENTVEC_NOT_LOADED => Err(RvcInferError::ContentvecNotLoaded),
            ffi::RVC_F0_NOT_LOADED => Err(RvcInferError::F0NotLoaded),
            ffi::RVC_PANIC => panic!("rvc engine: {}", self.message()),
            code => Err(RvcInferError::Backend(BackendError { code, message: self.message() })),
        }
    }

    fn check_load(&self, rc: i32) -> Result<(), BackendError> {
        if rc == ffi::RVC_OK { Ok(()) } else { Err(BackendError { code: rc, message: self.message() }) }
    }

    /// `RvcInfer::new` (rvc.rs:30-44).  `data_path` holds `contentvec/`, `f0/` as before, with `.rvcw` blobs
    /// (`python -m obs_rvc_amd.importers` converts the `.onnx` / `.pth` files).  Panics without a usable MI355X: the reference has
    /// no fallible constructor either, and there is no CPU fallback.
    pub fn new(data_path: PathBuf) -> Self {
        let p = c_path(&data_path);
        let mut handle: *mut ffi::RvcEngine = std::ptr::null_mut();
        let rc = unsafe { ffi::rvc_create(p.as_ptr(), -1, &mut handle) };
        assert!(rc == ffi::RVC_OK && !handle.is_null(), "rvc_create failed (status {}): no HIP device?", rc);
        RvcInfer { handle }
    }

    /// rvc.rs:46-54: `<data>/contentvec/vec-{768-layer-12,256-layer-9}.rvcw` (models.rs:58-61)
    pub fn load_contentvec(&mut self, model_version: RvcModelVersion) -> Result<(), BackendError> {
        let v: i64 = model_version.into();
        self.check_load(unsafe { ffi::rvc_load_contentvec(self.handle, v as i32) })
    }

    /// rvc.rs:56-60: the user's synthesizer; a path ending in `.onnx` is mapped to its `.rvcw` sibling
    pub fn load_model(&mut self, model_path: PathBuf) -> Result<(), BackendError> {
        let p = c_path(&model_path);
        self.check_load(unsafe { ffi::rvc_load_model(self.handle, p.as_ptr()) })
    }

    /// rvc.rs:62-75: `<data>/f0/rmvpe.rvcw` (models.rs:72)
    pub fn load_f0(&mut self, pitch_algorithm: PitchAlgorithm) -> Result<(), BackendError> {
        let a: i64 = pitch_algorithm.into();
        self.check_load(unsafe { ffi::rvc_load_f0(self.handle, a as i32) })
    }

    /// Not in the reference: the engine's f0 method by `ffi::RVC_F0_RMVPE` (the same as `load_f0`), `ffi::RVC_F0_YIN`, the weight-free
    /// time-domain tracker (no `<data>/f0/rmvpe.rvcw` needed), or `ffi::RVC_F0_CREPE` / `ffi::RVC_F0_CREPE_TINY`
    /// (`<data>/f0/crepe-full.rvcw` / `crepe-tiny.rvcw`), or `ffi::RVC_F0_FCPE` (`<data>/f0/fcpe.rvcw`), or `ffi::RVC_F0_PM`, Praat's
    /// autocorrelation tracker with a Viterbi path over the window (upstream's `pm`; weight-free as YIN)
    pub fn load_f0_method(&mut self, method: i32) -> Result<(), BackendError> {
        self.check_load(unsafe { ffi::rvc_load_f0_method(self.handle, method) })
    }

    /// Not in the reference: CREPE's decoder, `ffi::RVC_CREPE_VITERBI` (the default) or `ffi::RVC_CREPE_ARGMAX`
    pub fn set_crepe_decoder(&mut self, decoder: i32) -> Result<(), BackendError> {
        self.check_load(unsafe { ffi::rvc_set_crepe_decoder(self.handle, decoder) })
    }

    /// Not in the reference: `Some(true)` = the loaded model was trained with pitch guidance, `Some(false)` = without (upstream's `_nono`
    /// synthesizers: `infer` needs no f0 method and ignores `pitch_shift`), `None` = no model loaded
    pub fn model_has_f0(&self) -> Option<bool> {
        match unsafe { ffi::rvc_model_has_f0(self.handle) } {
            v if v < 0 => None,
            v => Some(v != 0),
        }
    }

    /// Not in the reference: rows of the loaded model's speaker table (1 for a model without one, 0 with no model loaded)
    pub fn speakers(&self) -> usize {
        unsafe { ffi::rvc_model_speakers(self.handle) }.max(0) as usize
    }

    /// Not in the reference: the speaker of a multi-speaker model by id; engine-wide, may change between any two chunks
    pub fn set_speaker(&mut self, sid: i32) -> Result<(), BackendError> {
        self.check_load(unsafe { ffi::rvc_set_speaker(self.handle, sid) })
    }

    /// Not in the reference: a blend of 1 to 8 distinct speakers, `(id, weight)` with weights >= 0 that are normalised to sum 1
    pub fn set_speaker_mix(&mut self, mix: &[(i32, f64)]) -> Result<(), BackendError> {
        let ids: Vec<i32> = mix.iter().map(|m| m.0).collect();
        let ws: Vec<f64> = mix.iter().map(|m| m.1).collect();
        self.check_load(unsafe { ffi::rvc_set_speaker_mix(self.handle, ids.as_ptr(), ws.as_ptr(), mix.len()) })
    }

    /// Not in the reference: the mix in force, `(id, normalised weight)`; empty with no model loaded
    pub fn speaker_mix(&self) -> Vec<(i32, f64)> {
        let (mut ids, mut ws, mut n) = ([0i32; 8], [0f64; 8], 0usize);
        if unsafe { ffi::rvc_speaker_mix(self.handle, ids.as_mut_ptr(), ws.as_mut_ptr(), 8, &mut n) } != 0 {
            return Vec::new();
        }
        (0..n.min(8)).map(|i| (ids[i], ws[i])).collect()
    }

    /// Not in the reference: FCPE's voicing threshold in [0, 1) (default 0.006): f0 = 0 where a frame's largest posterior is at or below it
    pub fn set_fcpe_threshold(&mut self, threshold: f64) -> Result<(), BackendError> {
        self.check_load(unsafe { ffi::rvc_set_fcpe_threshold(self.handle, threshold) })
    }

    pub fn fcpe_threshold(&self) -> f64 {
        unsafe { ffi::rvc_fcpe_threshold(self.handle) }
    }

    /// Not in the reference: hybrid f0 -- 1 to 4 distinct members (`ffi::RVC_F0_RMVPE`, `_YIN`, `_CREPE`, `_CREPE_TINY`, `_FCPE`, `_PM`), the first the lead, run on
    /// the same audio and combined per frame under `ffi::RVC_HYBRID_VOTE` (majority voicing, median of the voiced values) or `ffi::RVC_HYBRID_MEDIAN`
    /// (the forks' plain median).  All or nothing: on an error the method in force stays.  (Written without a Rust toolchain at hand, like the rest of this shim.)
    pub fn load_f0_hybrid(&mut self, methods: &[i32], mode: i32) -> Result<(), BackendError> {
        self.check_load(unsafe { ffi::rvc_load_f0_hybrid(self.handle, methods.as_ptr(), methods.len() as i32, mode) })
    }

    /// Not in the reference: the members (the lead first) and the mode of the hybrid in force, `None` when the method is no hybrid
    pub fn f0_hybrid(&self) -> Option<(Vec<i32>, i32)> {
        let (mut m, mut mode) = ([0i32; 4], 0i32);
        let n = unsafe { ffi::rvc_f0_hybrid(self.handle, m.as_mut_ptr(), 4, &mut mode) };
        if n <= 0 {
            return None;
        }
        Some((m[..(n as usize).min(4)].to_vec(), mode))
    }

    /// rvc.rs:77-79
    pub fn unload_model(&mut self) {
        unsafe { ffi::rvc_unload_model(self.handle) }
    }

    /// rvc.rs:81-97: ContentVec features, shape (1, C, T)
    pub fn hubert(&self, input: ArrayView1<f32>) -> Result<Array3<f32>, RvcInferError> {
        let x = input.as_standard_layout();
        let cap = 1024 * (x.len() / 320 + 8);
        let mut out = vec![0f32; cap];
        let mut dims = [0usize; 3];
        self.check(unsafe { ffi::rvc_hubert(self.handle, x.as_ptr(), x.len(), out.as_mut_ptr(), cap, dims.as_mut_ptr()) })?;
        out.truncate(dims[0] * dims[1] * dims[2]);
        Ok(Array3::from_shape_vec((dims[0], dims[1], dims[2]), out)?)
    }

    /// rvc.rs:99-109: frames duplicated to 2T+1, shape (1, 2T+1, C)
    pub fn extract_feature(&self, input: ArrayView1<f32>) -> Result<Array3<f32>, RvcInferError> {
        let x = input.as_standard_layout();
        let cap = 1024 * (2 * (x.len() / 320) + 16);
        let mut out = vec![0f32; cap];
        let mut dims = [0usize; 3];
        self.check(unsafe { ffi::rvc_extract_feature(self.handle, x.as_ptr(), x.len(), out.as_mut_ptr(), cap, dims.as_mut_ptr()) })?;
        out.truncate(dims[0] * dims[1] * dims[2]);
        Ok(Array3::from_shape_vec((dims[0], dims[1], dims[2]), out)?)
    }

    /// rvc.rs:111-131: f0 in Hz, one value per RMVPE frame, already multiplied by 2^(pitch_shift / 12) (integer division, as there)
    pub fn pitch(&mut self, input: ArrayView1<f32>, pitch_shift: i32, sample_frame_16k_size: usize) -> Result<Array1<f32>, RvcInferError> {
        let x = input.as_standard_layout();
        let mut out = vec![0f32; 4096];
        let mut n = 0usize;
        self.check(unsafe {
            ffi::rvc_pitch(self.handle, x.as_ptr(), x.len(), pitch_shift, sample_frame_16k_size, out.as_mut_ptr(), out.len(), &mut n)
        })?;
        out.truncate(n);
        Ok(Array1::from_vec(out))
    }

    /// rvc.rs:133-220: one chunk through ContentVec -> (retrieval) -> RMVPE -> pitch cache -> synthesizer; float PCM at the model rate
    pub fn infer(
        &mut self,
        input: ArrayView1<f32>,
        sample_frame_16k_size: usize,
        pitch_shift: Option<i32>,
        skip_head: u32,
        return_length: u32,
    ) -> Result<Array1<f32>, RvcInferError> {
        let x = input.as_standard_layout();
        let mut out = vec![0f32; return_length as usize * 1024 + 16];
        let mut n = 0usize;
        self.check(unsafe {
            ffi::rvc_infer(self.handle, x.as_ptr(), x.len(), sample_frame_16k_size, pitch_shift.is_some() as i32, pitch_shift.unwrap_or(0),
                           skip_head, return_length, out.as_mut_ptr(), out.len(), &mut n)
        })?;
        out.truncate(n);
        Ok(Array1::from_vec(out))
    }

    // ---- what the reference plumbs through its settings but never implements (rvc.rs:159 `// TODO: index search`) ----

    /// flat-L2 retrieval index, row-major (n, dim) fp32; `set_index_rate(0.0)` switches retrieval off again
    pub fn load_index(&mut self, vectors: ndarray::ArrayView2<f32>) -> Result<(), RvcInferError> {
        let v = vectors.as_standard_layout();
        self.check(unsafe { ffi::rvc_load_index(self.handle, v.as_ptr(), v.nrows(), v.ncols()) })
    }

    /// Attach an IVF structure (coarse centroids and the list number of every row) to the loaded index.
    pub fn set_index_ivf(&mut self, centroids: ndarray::ArrayView2<f32>, assign: &[i32]) -> Result<(), RvcInferError> {
        let c = centroids.as_standard_layout();
        self.check(unsafe { ffi::rvc_set_index_ivf(self.handle, c.as_ptr(), c.nrows(), c.ncols(), assign.as_ptr(), assign.len()) })
    }

    /// Lists probed per query: 0 = flat search, 1..=64 = IVF search (clamped to the number of lists).
    pub fn set_index_nprobe(&mut self, nprobe: i32) -> Result<(), RvcInferError> {
        self.check(unsafe { ffi::rvc_set_index_nprobe(self.handle, nprobe) })
    }

    pub fn index_nprobe(&self) -> i32 {
        unsafe { ffi::rvc_index_nprobe(self.handle) }
    }

    /// Neighbours blended per query: 4 (the default) or 8 (what upstream's pipelines search with).  Kept across index loads.
    pub fn set_index_k(&mut self, k: i32) -> Result<(), RvcInferError> {
        self.check(unsafe { ffi::rvc_set_index_k(self.handle, k) })
    }

    pub fn index_k(&self) -> i32 {
        unsafe { ffi::rvc_index_k(self.handle) }
    }

    /// (lists, rows of the longest list, empty lists) of the attached IVF structure.
    pub fn index_ivf_info(&mut self) -> Result<(usize, usize, usize), RvcInferError> {
        let (mut nlist, mut longest, mut empty) = (0usize, 0usize, 0usize);
        self.check(unsafe { ffi::rvc_index_ivf_info(self.handle, &mut nlist, &mut longest, &mut empty) })?;
        Ok((nlist, longest, empty))
    }

    pub fn set_index_rate(&mut self, rate: f32) {
        unsafe { ffi::rvc_set_index_rate(self.handle, rate) }
    }

    /// rank 0 of a multi-GPU job: the 128-byte id to hand to the other ranks (pipe, file, TCP)
    pub fn rccl_unique_id() -> Result<[u8; ffi::RVC_RCCL_UNIQUE_ID_BYTES], BackendError> {
        let mut id = [0u8; ffi::RVC_RCCL_UNIQUE_ID_BYTES];
        let rc = unsafe { ffi::rvc_rccl_unique_id(id.as_mut_ptr() as *mut _) };
        if rc == ffi::RVC_OK { Ok(id) } else { Err(BackendError { code: rc, message: "librccl not available".into() }) }
    }

    /// every rank: ONE ncclBroadcast of the shared index from rank 0 into this GPU's HBM (RCCL over xGMI); `vectors` only on rank 0
    pub fn index_broadcast(&mut self, unique_id: &[u8; ffi::RVC_RCCL_UNIQUE_ID_BYTES], rank: i32, world: i32,
                           vectors: Option<ndarray::ArrayView2<f32>>) -> Result<(), RvcInferError> {
        let rc = match vectors {
            Some(v) => {
                let v = v.as_standard_layout();
                unsafe { ffi::rvc_index_broadcast(self.handle, unique_id.as_ptr() as *const _, rank, world, v.as_ptr(), v.nrows(), v.ncols()) }
            }
            None => unsafe { ffi::rvc_index_broadcast(self.handle, unique_id.as_ptr() as *const _, rank, world, std::ptr::null(), 0, 0) },
        };
        self.check(rc)
    }

    pub fn set_noise_seed(&mut self, seed: u32, stream_id: u32) {
        unsafe { ffi::rvc_set_noise_seed(self.handle, seed, stream_id) }
    }

    /// the plugin's resonance shift (obs-rvc/src/lib.rs:446-451: `state.resonance_shift`), semitones in [-5, 5], every stream
    pub fn set_formant_shift(&mut self, semitones: f64) -> Result<(), RvcInferError> {
        let rc = unsafe { ffi::rvc_set_formant_shift(self.handle, semitones) };
        self.check(rc)
    }

    /// transpose in semitones, [-24, 24], fractions allowed, every stream; the integer `pitch_shift` of `pitch` / `infer` keeps the
    /// reference's whole-octave meaning (rvc.rs:121)
    pub fn set_pitch_semitones(&mut self, semitones: f64) -> Result<(), RvcInferError> {
        let rc = unsafe { ffi::rvc_set_pitch_semitones(self.handle, semitones) };
        self.check(rc)
    }

    /// voiced range in Hz, every stream: a voiced f0 row outside [lo_hz, hi_hz] becomes unvoiced; (0, +inf) = off
    pub fn set_f0_range(&mut self, lo_hz: f64, hi_hz: f64) -> Result<(), RvcInferError> {
        let rc = unsafe { ffi::rvc_set_f0_range(self.handle, lo_hz, hi_hz) };
        self.check(rc)
    }

    /// median filter on the f0 curve (upstream's `filter_radius`), radius 0..7, every stream
    pub fn set_f0_median(&mut self, radius: i32) -> Result<(), RvcInferError> {
        let rc = unsafe { ffi::rvc_set_f0_median(self.handle, radius) };
        self.check(rc)
    }

    /// snap f0 to a scale, every stream: bit k of `pitch_class_mask` allows pitch class k (C = 0), `strength` in [0, 1]; mask 0 = off
    pub fn set_f0_snap(&mut self, pitch_class_mask: u32, strength: f64) -> Result<(), RvcInferError> {
        let rc = unsafe { ffi::rvc_set_f0_snap(self.handle, pitch_class_mask, strength) };
        self.check(rc)
    }

    /// consonant protection (upstream's `protect`), [0, 0.5], 0.5 = off, every stream: on calls that use the index, unvoiced rows become
    /// `protect * blended + (1 - protect) * raw` ContentVec features
    pub fn set_protect(&mut self, protect: f64) -> Result<(), RvcInferError> {
        let rc = unsafe { ffi::rvc_set_protect(self.handle, protect) };
        self.check(rc)
    }

    /// f0 from outside: `hz` rows for the END of the next f0 window of `stream` (NaN keeps the tracker's value, 0 = unvoiced, else up to 20000 Hz); an empty slice
    /// clears.  The rows are transposed like any f0; consumed by the stream's next infer call unless `set_f0_override_hold(true)`
    pub fn set_f0_override(&mut self, stream: i32, hz: &[f32]) -> Result<(), RvcInferError> {
        let rc = unsafe { ffi::rvc_set_f0_override_stream(self.handle, stream, hz.as_ptr(), hz.len()) };
        self.check(rc)
    }

    pub fn set_f0_override_hold(&mut self, hold: bool) -> Result<(), RvcInferError> {
        let rc = unsafe { ffi::rvc_set_f0_override_hold(self.handle, hold as i32) };
        self.check(rc)
    }

    /// the f0 curve of the recording the converter calls convert next: breakpoints `t_sec` (strictly increasing) and `hz` of one length; empty slices clear
    pub fn set_f0_curve(&mut self, t_sec: &[f64], hz: &[f32]) -> Result<(), RvcInferError> {
        let n = if t_sec.len() == hz.len() { hz.len() } else { return self.check(ffi::RVC_SHAPE) };
        let rc = unsafe { ffi::rvc_set_f0_curve(self.handle, t_sec.as_ptr(), hz.as_ptr(), n) };
        self.check(rc)
    }

    /// the first `n_frames` rows of the curve's 10 ms grid as the device builds it (NaN = keep the tracker's value)
    pub fn f0_curve_grid(&mut self, n_frames: usize) -> Result<Vec<f32>, RvcInferError> {
        let mut out = vec![0f32; n_frames];
        let rc = unsafe { ffi::rvc_f0_curve_grid(self.handle, n_frames, out.as_mut_ptr(), out.len()) };
        self.check(rc).map(|_| out)
    }

    /// the conditioned f0 of the last completed conversion, one value per 10 ms frame of the recording
    pub fn convert_f0(&mut self) -> Result<Vec<f32>, RvcInferError> {
        let mut n: usize = 0;
        unsafe { ffi::rvc_convert_f0(self.handle, std::ptr::null_mut(), 0, &mut n) };
        let mut out = vec![0f32; n.max(1)];
        let rc = unsafe { ffi::rvc_convert_f0(self.handle, out.as_mut_ptr(), out.len(), &mut n) };
        out.truncate(n);
        self.check(rc).map(|_| out)
    }
}

impl Drop for RvcInfer {
    fn drop(&mut self) {
        unsafe { ffi::rvc_destroy(self.handle) }
    }
}
