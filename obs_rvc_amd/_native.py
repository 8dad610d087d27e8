"""Loader for the in-tree C-ABI library (csrc/librvc_mi355x.so).  No fallback: if the HIP
extension is missing or no GPU is present the product path raises."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.path.join(CSRC, "librvc_mi355x.so")
RPC_PATH = os.path.join(CSRC, "rvc-rpc")
_LIB = None

# every symbol include/rvc_mi355x.h declares
SYMBOLS = [
    "rvc_create", "rvc_destroy", "rvc_load_contentvec", "rvc_load_model", "rvc_load_f0", "rvc_unload_model",
    "rvc_hubert", "rvc_extract_feature", "rvc_pitch", "rvc_infer", "rvc_last_error_message",
    "rvc_load_index", "rvc_load_index_device", "rvc_set_index_rate", "rvc_get_knn", "rvc_set_noise_seed", "rvc_reset_state",
    "rvc_set_streams", "rvc_infer_batch", "rvc_infer_device", "rvc_infer_batch_v", "rvc_infer_device_v", "rvc_infer_batch_g", "rvc_synchronize", "rvc_set_use_graph", "rvc_set_pipeline",
    "rvc_last_gpu_ms", "rvc_profile_last", "rvc_set_profile", "rvc_enable_taps", "rvc_get_tap", "rvc_get_pitch_cache",
    "rvc_index_device_ptr", "rvc_device", "rvc_version", "rvc_envelop_mixing", "rvc_sola_step", "rvc_profile_last_knn",
    "rvc_resampler_create", "rvc_resampler_destroy", "rvc_resampler_input_frames_next", "rvc_resampler_output_frames_max",
    "rvc_resampler_reset", "rvc_resampler_process", "rvc_resampler_process_device",
    "rvc_rccl_unique_id", "rvc_index_broadcast", "rvc_rccl_available", "rvc_index_broadcast_info",
    "rvc_set_plan_cache", "rvc_plan_cache_info", "rvc_set_plan_autotune", "rvc_plan_autotune_info", "rvc_retrieval_recoveries", "rvc_set_gemm_precision",
    "rvc_calibrate", "rvc_clock_monitor_start", "rvc_clock_monitor_stop",
    "rvc_session_create", "rvc_session_destroy", "rvc_session_process", "rvc_session_frame_size", "rvc_session_set_params", "rvc_session_set_params_stream", "rvc_session_geometry",
    "rvc_set_formant_shift", "rvc_set_formant_shift_stream", "rvc_formant_geometry",
    "rvc_load_f0_method", "rvc_f0_method", "rvc_set_crepe_decoder", "rvc_crepe_decoder", "rvc_model_has_f0", "rvc_set_fcpe_threshold", "rvc_fcpe_threshold",
    "rvc_load_f0_hybrid", "rvc_f0_hybrid",
    "rvc_set_pitch_semitones", "rvc_set_pitch_semitones_stream", "rvc_set_f0_range", "rvc_set_f0_range_stream",
    "rvc_set_f0_median", "rvc_set_f0_median_stream", "rvc_set_f0_snap", "rvc_set_f0_snap_stream",
    "rvc_set_protect", "rvc_set_protect_stream",
    "rvc_model_speakers", "rvc_set_speaker", "rvc_set_speaker_mix", "rvc_speaker_mix",
    "rvc_sola_step_x", "rvc_input_gate", "rvc_session_set_crossfade", "rvc_session_set_crossfade_stream", "rvc_session_set_input_gate", "rvc_session_set_input_gate_stream",
    "rvc_denoiser_create", "rvc_denoiser_destroy", "rvc_denoiser_reset", "rvc_denoiser_set", "rvc_denoiser_latency", "rvc_denoiser_process", "rvc_denoiser_process_device",
    "rvc_session_set_noise_reduction", "rvc_session_set_noise_reduction_stream",
    "rvc_set_index_ivf", "rvc_set_index_nprobe", "rvc_index_nprobe", "rvc_index_ivf_info",
    "rvc_train_index_ivf", "rvc_index_ivf_train_info", "rvc_get_index_ivf",
    "rvc_set_index_k", "rvc_index_k",
    "rvc_index_build_begin", "rvc_index_build_add", "rvc_index_build_add_device", "rvc_index_build_info", "rvc_index_build_finish", "rvc_index_build_abort",
    "rvc_convert_geometry", "rvc_convert", "rvc_convert_device", "rvc_convert_info", "rvc_sola_stitch", "rvc_highpass",
    "rvc_resample_geometry", "rvc_resample", "rvc_resample_device", "rvc_change_rms", "rvc_convert_file", "rvc_convert_file_device", "rvc_convert_file_info",
    "rvc_set_f0_override_stream", "rvc_set_f0_override_hold", "rvc_set_f0_curve", "rvc_f0_curve_grid", "rvc_convert_f0",
    "rvc_analyze_f0", "rvc_analyze_f0_device", "rvc_f0_stats", "rvc_f0_stats_stream", "rvc_set_auto_transpose", "rvc_auto_transpose", "rvc_auto_transpose_info",
    "rvc_convert_many_geometry", "rvc_convert_many", "rvc_convert_many_info", "rvc_sola_stitch_many",
    "rvc_set_convert_silence", "rvc_convert_silence", "rvc_convert_silence_info", "rvc_silence_map",
    "rvc_analyze_f0_many", "rvc_f0_stats_many", "rvc_set_convert_many_pitch", "rvc_set_convert_many_auto_transpose", "rvc_convert_many_auto_transpose",
    "rvc_convert_many_pitch_info",
]


def _include_closure(src):
    """every file `src` (relative to csrc) reaches through #include "..." lines, itself included, each resolved against the including file.  A plain scan:
    an include under a preprocessor conditional counts too (a superset is safe for a cache key).  -> sorted tuple of paths relative to csrc"""
    import re
    seen, todo = set(), [os.path.normpath(src)]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        with open(os.path.join(CSRC, f)) as fh:
            todo += [os.path.normpath(os.path.join(os.path.dirname(f), i)) for i in re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', fh.read(), re.M)]
    return tuple(sorted(seen))


# translation units of the library: (source, extra flags, files whose contents decide whether the object is stale = the source's include closure).  The
# implicit-GEMM template instantiations are the bulk of the compile time; as separate units they build in parallel (5 min -> about 1.5 min on 8 cores)
# and are not rebuilt when only the engine changes.
UNITS = [(src, flags, _include_closure(src)) for src, flags in
         [(u, []) for u in ("engine.hip", "debug.hip", "calib.hip", "plan.hip", "model_cv.hip", "model_rmvpe.hip", "model_yin.hip", "f0_pm.hip", "model_crepe.hip", "model_fcpe.hip", "model_synth.hip", "retrieval.hip")] +
         [("igemm2_inst.hip", ["-DRVC_IGEMM2_CFG=%d" % c]) for c in range(5)] +
         [("igemm_tiled_inst.hip", ["-DRVC_TILED_PART=%d" % c]) for c in range(4)] +
         [("igemm2w_inst.hip", ["-DRVC_G2W_PART=%d" % c]) for c in range(3)] +
         [("igemm_bf3_inst.hip", []), ("conv_tile_inst.hip", [])] +
         [("conv32s_inst.hip", ["-DRVC_C32S_PART=%d" % c]) for c in range(3)] +
         [("igemm32l_inst.hip", ["-DRVC_G32L_PART=%d" % c]) for c in range(2)]]
# what source_hash covers: every unit's closure inside csrc, and what is built or read besides the units
SOURCES = tuple(sorted({d for _, _, deps in UNITS for d in deps if not d.startswith("..")} | {"version.cpp", "exports.map", "rvc_rpc.cpp"}))
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
# Object cache: content-addressed (sources + flags).  It lives under the repository's build/ directory (git- and gpurun-ignored), is
# created 0700, and a directory that is not ours (other owner, or writable by group / others) is refused: objects are linked straight
# into the product library, so nobody else may be able to plant one.
OBJ_CACHE = os.environ.get("RVC_OBJ_CACHE", os.path.join(os.path.dirname(_HERE), "build", "obj_cache"))


def _private_cache_dir() -> str:
    os.makedirs(OBJ_CACHE, mode=0o700, exist_ok=True)
    st = os.stat(OBJ_CACHE)
    if st.st_uid != os.getuid() or (st.st_mode & 0o022):
        raise RuntimeError("object cache %s is not private to uid %d (owner %d, mode %o): refusing to link objects from it"
                           % (OBJ_CACHE, os.getuid(), st.st_uid, st.st_mode & 0o777))
    return OBJ_CACHE


def _tmp_name(path: str) -> str:
    """unique per builder (several ranks may call build() at once); published with os.replace, which is atomic"""
    import uuid
    return "%s.%d.%s.tmp.o" % (path, os.getpid(), uuid.uuid4().hex[:8])


def source_hash() -> str:
    """sha256 over the library's sources (+ the public header and the test hooks' header), first 16 hex digits.  It is compiled into the binary
    (`rvc_version()` ends in "src:<hash>"), so a tested .so can be tied to the sources it was built from."""
    import hashlib
    h = hashlib.sha256()
    for f in [os.path.join(CSRC, n) for n in SOURCES] + [os.path.join(os.path.dirname(_HERE), "include", h) for h in ("rvc_mi355x.h", "rvc_mi355x_debug.h")]:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def binary_hash(path: str = None) -> str:
    """The source hash embedded in a built library ("" if the file is missing or predates the scheme); read from the file's bytes,
    so no GPU and no dlopen is needed."""
    path = path or SO_PATH
    if not os.path.exists(path):
        return ""
    with open(path, "rb") as fh:
        blob = fh.read()
    i = blob.find(b"rvc-mi355x-src:")
    return blob[i + 15:i + 31].decode("ascii", "replace") if i >= 0 else ""


def _unit_key(src, flags, deps, extra_flags):
    import hashlib
    h = hashlib.sha256(" ".join(HIPCC_FLAGS + list(flags) + list(extra_flags)).encode())
    for n in deps:
        with open(os.path.join(CSRC, n), "rb") as fh:
            h.update(n.encode() + b"\0" + fh.read())
    return "%s-%s" % (os.path.splitext(src)[0], h.hexdigest()[:20])


def compile_units(extra_flags=(), verbose=False, extra_units=()):
    """Compile every translation unit whose object is not in the cache (content-addressed: sources + flags), in parallel.
    -> list of object paths"""
    from concurrent.futures import ThreadPoolExecutor
    _private_cache_dir()
    jobs, objs = [], []
    for src, flags, deps in list(UNITS) + list(extra_units):
        obj = os.path.join(OBJ_CACHE, _unit_key(src, flags, tuple(deps), extra_flags) + ".o")
        objs.append(obj)
        if not os.path.exists(obj):
            tmp = _tmp_name(obj)
            jobs.append((["hipcc"] + HIPCC_FLAGS + list(flags) + list(extra_flags) + ["-c", os.path.join(CSRC, src), "-o", tmp], obj, tmp))

    def run(job):
        cmd, obj, tmp = job
        if verbose:
            print(" ".join(cmd), flush=True)
        try:
            subprocess.check_call(cmd)
            os.replace(tmp, obj)
        finally:
            if os.path.exists(tmp):
                os.unlink(tmp)
    if jobs:
        with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), os.cpu_count() or 1))) as ex:
            list(ex.map(run, jobs))
    return objs


def link_library(objs, out, want_hash, verbose=False):
    ver = _tmp_name(os.path.join(_private_cache_dir(), "version-%s" % want_hash))
    tmp_out = "%s.%d.tmp" % (out, os.getpid())
    try:
        cmd = ["hipcc", "-O2", "-fPIC", "-c", '-DRVC_SRC_HASH="%s"' % want_hash, os.path.join(CSRC, "version.cpp"), "-o", ver]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        # exports.map: only the C ABI (rvc_*) is visible; the planner's C++ internals and the kernels' host stubs stay local
        cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + [ver, "-o", tmp_out, "-ldl", "-Wl,--version-script=" + os.path.join(CSRC, "exports.map")]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        os.replace(tmp_out, out)
    finally:
        for f in (ver, tmp_out):
            if os.path.exists(f):
                os.unlink(f)


def build(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950: the engine library (one object per translation unit, built in parallel, linked into
    csrc/librvc_mi355x.so) and the rvc-rpc protocol-compatible executable.  A library is reused only if the source hash compiled
    into it equals the hash of the sources on disk (never by modification time)."""
    want = source_hash()
    have = binary_hash()
    if force or have != want:
        if verbose:
            print("source hash %s, binary %s -> rebuilding" % (want, have or "(none)"))
        if force:
            import shutil
            shutil.rmtree(OBJ_CACHE, ignore_errors=True)
        link_library(compile_units(verbose=verbose), SO_PATH, want, verbose)
    elif verbose:
        print("librvc_mi355x.so carries source hash %s = sources on disk: up to date" % have)
    rpc_src = os.path.join(CSRC, "rvc_rpc.cpp")
    if force or have != want or not os.path.exists(RPC_PATH) or os.path.getmtime(RPC_PATH) < os.path.getmtime(rpc_src):
        cmd = ["hipcc", "-O2", "-std=c++17", rpc_src, "-o", RPC_PATH, "-L" + CSRC, "-lrvc_mi355x", "-Wl,-rpath,$ORIGIN"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return SO_PATH


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(SO_PATH):
        raise RuntimeError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % SO_PATH)
    # RVC_LIB_OVERRIDE (A/B timing of an older build) is honoured only together with RVC_TUNING=1: outside the tuning tools nothing but the
    # in-tree library is ever loaded
    override = os.environ.get("RVC_LIB_OVERRIDE") if os.environ.get("RVC_TUNING") == "1" else None
    L = C.CDLL(override or SO_PATH)
    vp, fp, sz, i32, u32 = C.c_void_p, C.POINTER(C.c_float), C.c_size_t, C.c_int32, C.c_uint32
    L.rvc_create.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.rvc_destroy.argtypes = [vp]
    L.rvc_destroy.restype = None
    L.rvc_load_contentvec.argtypes = [vp, C.c_int]
    L.rvc_load_model.argtypes = [vp, C.c_char_p]
    L.rvc_load_f0.argtypes = [vp, C.c_int]
    L.rvc_unload_model.argtypes = [vp]
    L.rvc_unload_model.restype = None
    L.rvc_hubert.argtypes = [vp, fp, sz, fp, sz, C.POINTER(sz)]
    L.rvc_extract_feature.argtypes = [vp, fp, sz, fp, sz, C.POINTER(sz)]
    L.rvc_pitch.argtypes = [vp, fp, sz, i32, sz, fp, sz, C.POINTER(sz)]
    L.rvc_infer.argtypes = [vp, fp, sz, sz, C.c_int, i32, u32, u32, fp, sz, C.POINTER(sz)]
    L.rvc_last_error_message.argtypes = [vp]
    L.rvc_last_error_message.restype = C.c_char_p
    L.rvc_load_index.argtypes = [vp, fp, sz, sz]
    L.rvc_load_index_device.argtypes = [vp, vp, sz, sz]
    L.rvc_set_index_rate.argtypes = [vp, C.c_float]
    L.rvc_set_index_rate.restype = None
    L.rvc_get_knn.argtypes = [vp, C.POINTER(i32), fp, sz, C.POINTER(sz)]
    if hasattr(L, "rvc_set_index_ivf") or not override:
        L.rvc_set_index_ivf.argtypes = [vp, fp, sz, sz, C.POINTER(i32), sz]
        L.rvc_set_index_nprobe.argtypes = [vp, C.c_int]
        L.rvc_index_nprobe.argtypes = [vp]
        L.rvc_index_ivf_info.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    if hasattr(L, "rvc_set_index_k") or not override:
        L.rvc_set_index_k.argtypes = [vp, C.c_int]
        L.rvc_index_k.argtypes = [vp]
    if hasattr(L, "rvc_train_index_ivf") or not override:
        L.rvc_train_index_ivf.argtypes = [vp, sz, C.c_int, C.POINTER(i32), u32]
        L.rvc_index_ivf_train_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(sz), C.POINTER(C.c_double), sz, C.POINTER(sz), C.POINTER(C.c_double)]
        L.rvc_get_index_ivf.argtypes = [vp, fp, sz, C.POINTER(i32), sz]
    if hasattr(L, "rvc_index_build_begin") or not override:
        L.rvc_index_build_begin.argtypes = [vp, sz, sz]
        L.rvc_index_build_add.argtypes = [vp, fp, sz, C.POINTER(sz)]
        L.rvc_index_build_add_device.argtypes = [vp, vp, sz, C.POINTER(sz)]
        L.rvc_index_build_info.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(C.c_double)]
        L.rvc_index_build_finish.argtypes = [vp, sz, sz, C.c_int, u32]
        L.rvc_index_build_abort.argtypes = [vp]
        L.rvc_index_build_abort.restype = None
    if hasattr(L, "rvc_convert") or not override:
        L.rvc_convert_geometry.argtypes = [sz, sz, sz, sz, sz, C.POINTER(sz)]
        L.rvc_convert.argtypes = [vp, fp, sz, sz, sz, sz, i32, C.c_int, fp, sz, C.POINTER(sz)]
        L.rvc_convert_device.argtypes = [vp, vp, sz, sz, sz, sz, i32, C.c_int, vp, sz, C.POINTER(sz)]
        L.rvc_convert_info.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(i32), sz, C.POINTER(C.c_double)]
        L.rvc_sola_stitch.argtypes = [vp, fp, sz, sz, sz, sz, sz, fp, C.POINTER(i32)]
        L.rvc_highpass.argtypes = [vp, fp, sz, fp]
    if hasattr(L, "rvc_convert_file") or not override:
        L.rvc_resample_geometry.argtypes = [sz, sz, sz, C.POINTER(sz)]
        L.rvc_resample.argtypes = [vp, fp, sz, sz, sz, fp, sz, C.POINTER(sz)]
        L.rvc_resample_device.argtypes = [vp, vp, sz, sz, sz, vp, sz, C.POINTER(sz)]
        L.rvc_change_rms.argtypes = [vp, fp, sz, sz, fp, sz, sz, C.c_double]
        L.rvc_convert_file.argtypes = [vp, fp, sz, sz, sz, sz, sz, i32, C.c_int, C.c_double, sz, fp, sz, C.POINTER(sz)]
        L.rvc_convert_file_device.argtypes = [vp, vp, sz, sz, sz, sz, sz, i32, C.c_int, C.c_double, sz, vp, sz, C.POINTER(sz)]
        L.rvc_convert_file_info.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(sz), fp]
    L.rvc_set_noise_seed.argtypes = [vp, u32, u32]
    L.rvc_set_noise_seed.restype = None
    L.rvc_reset_state.argtypes = [vp]
    L.rvc_reset_state.restype = None
    L.rvc_set_streams.argtypes = [vp, C.c_int]
    L.rvc_infer_batch.argtypes = [vp, fp, sz, sz, i32, u32, u32, fp, sz, C.POINTER(sz)]
    L.rvc_infer_device.argtypes = [vp, vp, sz, sz, i32, u32, u32, vp, sz, C.POINTER(sz), C.c_int]
    L.rvc_infer_batch_v.argtypes = [vp, fp, sz, sz, C.POINTER(i32), u32, u32, fp, sz, C.POINTER(sz)]
    L.rvc_infer_device_v.argtypes = [vp, vp, sz, sz, C.POINTER(i32), u32, u32, vp, sz, C.POINTER(sz), C.c_int]
    L.rvc_infer_batch_g.argtypes = [vp, C.POINTER(fp), C.POINTER(sz), C.POINTER(sz), C.POINTER(i32), C.POINTER(u32), C.POINTER(u32), C.POINTER(fp), C.POINTER(sz), C.POINTER(sz)]
    L.rvc_synchronize.argtypes = [vp]
    L.rvc_set_use_graph.argtypes = [vp, C.c_int]
    L.rvc_set_use_graph.restype = None
    if hasattr(L, "rvc_set_plan_cache") or not override:      # (an older build loaded for an A/B timing lacks the newer entry points)
        L.rvc_set_plan_cache.argtypes = [vp, C.c_int]
        L.rvc_plan_cache_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
        L.rvc_retrieval_recoveries.argtypes = [vp]
        L.rvc_retrieval_recoveries.restype = C.c_longlong
    if hasattr(L, "rvc_set_gemm_precision") or not override:
        L.rvc_set_gemm_precision.argtypes = [vp, C.c_int]
    if hasattr(L, "rvc_set_formant_shift") or not override:
        L.rvc_set_formant_shift.argtypes = [vp, C.c_double]
        L.rvc_set_formant_shift_stream.argtypes = [vp, C.c_int, C.c_double]
        L.rvc_formant_geometry.argtypes = [sz, sz, C.c_double, C.POINTER(sz)]
        L.rvc_debug_formant_table.argtypes = [sz, sz, fp, sz, C.POINTER(sz)]
        L.rvc_debug_formant_table.restype = C.c_int
    L.rvc_set_pipeline.argtypes = [vp, C.c_int]
    L.rvc_set_pipeline.restype = None
    L.rvc_last_gpu_ms.argtypes = [vp]
    L.rvc_last_gpu_ms.restype = C.c_float
    L.rvc_profile_last.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rvc_profile_last_knn.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rvc_set_profile.argtypes = [vp, C.c_int]
    L.rvc_set_profile.restype = None
    L.rvc_enable_taps.argtypes = [vp, C.c_int]
    L.rvc_enable_taps.restype = None
    L.rvc_get_tap.argtypes = [vp, C.c_char_p, fp, sz, C.POINTER(sz)]
    L.rvc_get_pitch_cache.argtypes = [vp, C.c_int, fp]
    L.rvc_get_pitch_cache.restype = None
    L.rvc_index_device_ptr.argtypes = [vp, C.POINTER(sz)]
    L.rvc_index_device_ptr.restype = vp
    L.rvc_device.argtypes = [vp]
    L.rvc_version.restype = C.c_char_p
    L.rvc_envelop_mixing.argtypes = [vp, fp, fp, sz, sz, C.c_double]
    L.rvc_sola_step.argtypes = [vp, fp, sz, fp, sz, sz, sz, fp, C.POINTER(sz)]
    L.rvc_resampler_create.argtypes = [vp, sz, sz, sz, C.POINTER(vp)]
    L.rvc_resampler_destroy.argtypes = [vp]
    L.rvc_resampler_destroy.restype = None
    L.rvc_resampler_input_frames_next.argtypes = [vp]
    L.rvc_resampler_input_frames_next.restype = sz
    L.rvc_resampler_output_frames_max.argtypes = [vp]
    L.rvc_resampler_output_frames_max.restype = sz
    L.rvc_resampler_reset.argtypes = [vp]
    L.rvc_resampler_reset.restype = None
    L.rvc_resampler_process.argtypes = [vp, fp, sz, fp, sz, C.POINTER(sz)]
    L.rvc_resampler_process_device.argtypes = [vp, vp, vp, C.c_int]
    if hasattr(L, "rvc_rccl_unique_id") or not override:
        L.rvc_rccl_unique_id.argtypes = [vp]
        L.rvc_index_broadcast.argtypes = [vp, vp, C.c_int, C.c_int, fp, sz, sz]
        L.rvc_index_broadcast_info.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.rvc_session_create.argtypes = [vp, sz, C.c_double, C.c_double, C.c_double, sz, i32, C.c_double, C.c_int, C.POINTER(vp)]
    L.rvc_session_destroy.argtypes = [vp]
    L.rvc_session_destroy.restype = None
    L.rvc_session_process.argtypes = [vp, fp, sz, fp, sz, C.POINTER(sz)]
    L.rvc_session_frame_size.argtypes = [vp]
    L.rvc_session_frame_size.restype = sz
    L.rvc_session_set_params.argtypes = [vp, i32, C.c_double]
    L.rvc_session_set_params.restype = None
    L.rvc_session_set_params_stream.argtypes = [vp, C.c_int, i32, C.c_double]
    L.rvc_session_geometry.argtypes = [vp, C.POINTER(i32)]
    L.rvc_session_geometry.restype = None
    if hasattr(L, "rvc_sola_step_x") or not override:
        L.rvc_sola_step_x.argtypes = [vp, fp, sz, fp, sz, sz, sz, fp, C.POINTER(sz), C.c_int]
        L.rvc_input_gate.argtypes = [vp, fp, fp, sz, sz, C.c_double, fp, fp]
        L.rvc_session_set_crossfade.argtypes = [vp, C.c_int]
        L.rvc_session_set_crossfade_stream.argtypes = [vp, C.c_int, C.c_int]
        L.rvc_session_set_input_gate.argtypes = [vp, C.c_double]
        L.rvc_session_set_input_gate_stream.argtypes = [vp, C.c_int, C.c_double]
        L.rvc_debug_session_sola_ms.argtypes = [vp, C.c_int]
        L.rvc_debug_session_sola_ms.restype = C.c_float
    if hasattr(L, "rvc_denoiser_create") or not override:
        L.rvc_denoiser_create.argtypes = [vp, sz, C.c_int, C.POINTER(vp)]
        L.rvc_denoiser_destroy.argtypes = [vp]
        L.rvc_denoiser_destroy.restype = None
        L.rvc_denoiser_reset.argtypes = [vp]
        L.rvc_denoiser_reset.restype = None
        L.rvc_denoiser_set.argtypes = [vp, C.c_int, C.c_double, C.c_double]
        L.rvc_denoiser_latency.argtypes = [vp]
        L.rvc_denoiser_latency.restype = sz
        L.rvc_denoiser_process.argtypes = [vp, fp, sz, fp]
        L.rvc_denoiser_process_device.argtypes = [vp, vp, vp, sz, sz, sz, C.c_int]
        L.rvc_session_set_noise_reduction.argtypes = [vp, C.c_int, C.c_double, C.c_double]
        L.rvc_session_set_noise_reduction_stream.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double]
        L.rvc_debug_session_denoise_ms.argtypes = [vp, C.c_int]
        L.rvc_debug_session_denoise_ms.restype = C.c_float
    if hasattr(L, "rvc_load_f0_method") or not override:
        L.rvc_load_f0_method.argtypes = [vp, C.c_int]
        L.rvc_f0_method.argtypes = [vp]
    if hasattr(L, "rvc_set_crepe_decoder") or not override:
        L.rvc_set_crepe_decoder.argtypes = [vp, C.c_int]
        L.rvc_crepe_decoder.argtypes = [vp]
        L.rvc_debug_crepe_decode.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, fp, vp, fp]
    if hasattr(L, "rvc_set_fcpe_threshold") or not override:
        L.rvc_set_fcpe_threshold.argtypes = [vp, C.c_double]
        L.rvc_fcpe_threshold.argtypes = [vp]
        L.rvc_fcpe_threshold.restype = C.c_double
        L.rvc_debug_fcpe_decode.argtypes = [vp, fp, C.c_int, C.c_int, fp, vp]
        L.rvc_debug_fcpe_dw.argtypes = [vp, fp, fp, fp, C.c_int, C.c_int, C.c_int, fp]
    if hasattr(L, "rvc_load_f0_hybrid") or not override:
        L.rvc_load_f0_hybrid.argtypes = [vp, C.POINTER(C.c_int), C.c_int, C.c_int]
        L.rvc_f0_hybrid.argtypes = [vp, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
        L.rvc_debug_f0_hybrid.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp, C.c_int, fp, fp, fp]
    if hasattr(L, "rvc_debug_pm") or not override:
        L.rvc_debug_pm.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, vp, fp, fp, fp, vp, fp]
    if hasattr(L, "rvc_set_f0_override_stream") or not override:
        L.rvc_set_f0_override_stream.argtypes = [vp, C.c_int, fp, sz]
        L.rvc_set_f0_override_hold.argtypes = [vp, C.c_int]
        L.rvc_set_f0_curve.argtypes = [vp, C.POINTER(C.c_double), fp, sz]
        L.rvc_f0_curve_grid.argtypes = [vp, sz, fp, sz]
        L.rvc_convert_f0.argtypes = [vp, fp, sz, C.POINTER(sz)]
        L.rvc_debug_f0_override.argtypes = [vp, C.c_int, fp, C.c_int, C.c_int, fp, C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.c_int, fp]
    if hasattr(L, "rvc_analyze_f0") or not override:
        dp = C.POINTER(C.c_double)
        L.rvc_analyze_f0.argtypes = [vp, fp, sz, sz, sz, sz, C.c_int, fp, sz, C.POINTER(sz)]
        L.rvc_analyze_f0_device.argtypes = [vp, vp, sz, sz, sz, sz, C.c_int, vp, sz, C.POINTER(sz)]
        L.rvc_f0_stats.argtypes = [vp, fp, sz, dp, sz, fp, C.POINTER(sz)]
        L.rvc_f0_stats_stream.argtypes = [vp, C.c_int, dp, sz, fp, C.POINTER(sz)]
        L.rvc_set_auto_transpose.argtypes = [vp, C.c_double, C.c_int, C.c_double]
        L.rvc_auto_transpose.argtypes = [vp, dp, C.POINTER(C.c_int), dp]
        L.rvc_auto_transpose_info.argtypes = [vp, fp, C.POINTER(sz), dp, dp]
    if hasattr(L, "rvc_convert_many") or not override:
        szp = C.POINTER(sz)
        L.rvc_convert_many_geometry.argtypes = [szp, sz, sz, sz, sz, sz, szp, szp, szp]
        L.rvc_convert_many.argtypes = [vp, C.POINTER(fp), szp, sz, sz, sz, sz, i32, C.c_int, C.POINTER(fp), szp, szp]
        L.rvc_convert_many_info.argtypes = [vp, szp, szp, C.POINTER(i32), sz, C.POINTER(C.c_double)]
        L.rvc_sola_stitch_many.argtypes = [vp, fp, szp, sz, sz, sz, sz, sz, fp, C.POINTER(i32)]
    if hasattr(L, "rvc_analyze_f0_many") or not override:
        szp, dp = C.POINTER(sz), C.POINTER(C.c_double)
        L.rvc_analyze_f0_many.argtypes = [vp, C.POINTER(fp), szp, sz, sz, sz, sz, C.c_int, C.POINTER(fp), szp, szp]
        L.rvc_f0_stats_many.argtypes = [vp, fp, szp, sz, dp, sz, fp, szp]
        L.rvc_set_convert_many_pitch.argtypes = [vp, dp, sz]
        L.rvc_set_convert_many_auto_transpose.argtypes = [vp, C.c_double, C.c_int, C.c_double]
        L.rvc_convert_many_auto_transpose.argtypes = [vp, dp, C.POINTER(C.c_int), dp]
        L.rvc_convert_many_pitch_info.argtypes = [vp, fp, szp, dp, dp, sz, dp]
    if hasattr(L, "rvc_set_convert_silence") or not override:
        szp, dp, u8p = C.POINTER(sz), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        L.rvc_set_convert_silence.argtypes = [vp, C.c_double, C.c_int]
        L.rvc_convert_silence.argtypes = [vp, dp, C.POINTER(C.c_int)]
        L.rvc_convert_silence_info.argtypes = [vp, szp, szp, szp, szp, dp]
        L.rvc_silence_map.argtypes = [vp, fp, sz, C.c_double, C.c_int, sz, sz, sz, sz, u8p, u8p, sz, u8p, C.POINTER(i32), sz]
    if hasattr(L, "rvc_model_has_f0") or not override:
        L.rvc_model_has_f0.argtypes = [vp]
    if hasattr(L, "rvc_model_speakers") or not override:
        L.rvc_model_speakers.argtypes = [vp]
        L.rvc_set_speaker.argtypes = [vp, C.c_int]
        L.rvc_set_speaker_mix.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_double), sz]
        L.rvc_speaker_mix.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_double), sz, C.POINTER(sz)]
        L.rvc_debug_speaker_biases.argtypes = [vp, C.c_int, fp, sz, C.POINTER(sz)]
        L.rvc_debug_speaker_fold_ms.argtypes = [vp]
        L.rvc_debug_speaker_fold_ms.restype = C.c_float
    if hasattr(L, "rvc_set_pitch_semitones") or not override:
        L.rvc_set_pitch_semitones.argtypes = [vp, C.c_double]
        L.rvc_set_pitch_semitones_stream.argtypes = [vp, C.c_int, C.c_double]
        L.rvc_set_f0_range.argtypes = [vp, C.c_double, C.c_double]
        L.rvc_set_f0_range_stream.argtypes = [vp, C.c_int, C.c_double, C.c_double]
        L.rvc_set_f0_median.argtypes = [vp, C.c_int]
        L.rvc_set_f0_median_stream.argtypes = [vp, C.c_int, C.c_int]
        L.rvc_set_f0_snap.argtypes = [vp, u32, C.c_double]
        L.rvc_set_f0_snap_stream.argtypes = [vp, C.c_int, u32, C.c_double]
    if hasattr(L, "rvc_set_protect") or not override:
        L.rvc_set_protect.argtypes = [vp, C.c_double]
        L.rvc_set_protect_stream.argtypes = [vp, C.c_int, C.c_double]
    if hasattr(L, "rvc_set_plan_autotune") or not override:
        L.rvc_set_plan_autotune.argtypes = [vp, C.c_int]
        L.rvc_plan_autotune_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(L, "rvc_calibrate") or not override:
        L.rvc_calibrate.argtypes = [C.c_int, C.POINTER(Calibration)]
        L.rvc_clock_monitor_start.argtypes = [C.c_int]
        L.rvc_clock_monitor_stop.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    _LIB = L
    return L


class Calibration(C.Structure):
    """rvc_calibration (include/rvc_mi355x.h)"""
    _fields_ = [("mfma_f32_tflops", C.c_double), ("mfma_sclk_mhz", C.c_double), ("mfma_ms", C.c_double),
                ("hbm_read_tbs", C.c_double), ("hbm_sclk_mhz", C.c_double), ("ms_total", C.c_double), ("compute_units", C.c_int)]


def calibrate(device: int = 0) -> dict:
    """rvc_calibrate: what this GPU sustains right now (bare fp32-MFMA stream, HBM read stream) -> dict"""
    c = Calibration()
    rc = lib().rvc_calibrate(device, C.byref(c))
    if rc != 0:
        raise RuntimeError("rvc_calibrate failed (%d)" % rc)
    return {k: getattr(c, k) for k, _ in Calibration._fields_}


def clock_monitor_start(device: int = 0) -> None:
    if lib().rvc_clock_monitor_start(device) != 0:
        raise RuntimeError("rvc_clock_monitor_start failed")


def clock_monitor_stop(device: int = 0) -> dict:
    mean, mn, secs = C.c_double(), C.c_double(), C.c_double()
    if lib().rvc_clock_monitor_stop(device, C.byref(mean), C.byref(mn), C.byref(secs)) != 0:
        raise RuntimeError("rvc_clock_monitor_stop failed")
    return {"sclk_mhz_mean": mean.value, "sclk_mhz_min": mn.value, "seconds": secs.value}
