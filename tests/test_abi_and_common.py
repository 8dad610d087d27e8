"""Host-side checks that need no GPU: the C-ABI library loads and exports every symbol the header declares;
rvc-common mirror; geometry formulas; blob round trip; stream sharding."""
import ctypes
import os
import re

import numpy as np
import pytest

from common import ROOT
from obs_rvc_amd import _native, dist, geometry, weights as W
from obs_rvc_amd.rvc_common import PitchAlgorithm, RvcInferError, RvcModelVersion


def _declared():
    hdr = open(os.path.join(ROOT, "include", "rvc_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(rvc_[a-z0-9_]+)\s*\(", hdr)))


def test_header_symbols_exported():
    names = _declared()
    assert "rvc_infer" in names and "rvc_create" in names and len(names) >= 30
    assert sorted(_native.SYMBOLS) == names
    if not os.path.exists(_native.SO_PATH):
        _native.build()
    lib = ctypes.CDLL(_native.SO_PATH)
    for n in names:
        assert hasattr(lib, n), n
    lib.rvc_version.restype = ctypes.c_char_p
    assert b"gfx950" in lib.rvc_version()


def test_library_carries_the_hash_of_its_sources():
    # build() never reuses a binary by modification time: the source hash compiled into rvc_version() must equal the sources on disk
    assert _native.binary_hash() == _native.source_hash()
    assert _native.lib().rvc_version().decode().endswith("rvc-mi355x-src:" + _native.source_hash())



# every environment variable the product library (and the rvc-rpc executable) may read: INTEGRATION.md lists the same names
PRODUCT_ENV = {"GPU_MAX_HW_QUEUES", "RVC_NO_RUNTIME_DEFAULTS", "LOCAL_RANK", "RVC_RCCL_LIB", "RVC_NOISE_SEED", "RVC_USE_GRAPH"}


def test_product_reads_only_the_documented_environment():
    # the library had become a laboratory of 64 RVC_* switches a host inherited from its environment.  Now: getenv() is
    # called with the documented names only, outside "#ifdef RVC_TUNING" blocks; tuning switches compile to nothing in the product
    # (tune_env is a constant nullptr) and test hooks are set by an explicit call (rvc_debug_option), never inherited.
    csrc = _native.CSRC
    seen = set()
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h", ".cpp")):
            continue
        text = open(os.path.join(csrc, f)).read()
        text = re.sub(r"#ifdef RVC_TUNING.*?#(?:else|endif)", "", text, flags=re.S)      # the tuning build's fall-back to the environment
        seen |= set(re.findall(r"\bgetenv\(\s*\"([^\"]+)\"", text))
        assert not re.findall(r"\bgetenv\(\s*[a-z_]", text), f      # no computed names
    assert seen <= PRODUCT_ENV, seen - PRODUCT_ENV
    assert len(seen) <= 10
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in seen:
        assert n in doc, n
    # the binary agrees with the text: no other RVC_* name sits next to a getenv call site (strings of the hooks exist, as table keys)
    lib = _native.lib()
    lib.rvc_debug_option.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    assert lib.rvc_debug_option(b"RVC_FORCE_CFG", b"0,4") == 0 and lib.rvc_debug_option(b"RVC_FORCE_CFG", None) == 0
    assert lib.rvc_debug_option(b"RVC_GEMM32", b"0") == -1          # a tuning switch: not settable in the product
    assert lib.rvc_debug_option(b"PATH", b"x") == -1

def test_library_exports_only_the_c_abi_and_no_result_changing_hook():
    # `nm -D` listed ~70 C++ internals of the planner and the kernels' host stubs; the link now takes an export list
    # (csrc/exports.map): the dynamic symbols are the C ABI of include/rvc_mi355x.h plus the rvc_debug_* test hooks of include/rvc_mi355x_debug.h,
    # nothing else.  And no hook of the PRODUCT build changes results: conv32s_kernel's ablation switches (RVC_C32S_DBG: they drop loads) exist
    # in the -DRVC_TUNING build only.
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _native.SO_PATH], capture_output=True, text=True, check=True).stdout
    syms = sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    assert syms and all(s.startswith("rvc_") for s in syms), [s for s in syms if not s.startswith("rvc_")][:5]
    dbg_hdr = open(os.path.join(ROOT, "include", "rvc_mi355x_debug.h")).read()
    dbg_hdr = re.sub(r"/\*.*?\*/", "", dbg_hdr, flags=re.S)
    dbg_declared = sorted(set(re.findall(r"\b(rvc_debug_[a-z0-9_]+)\s*\(", dbg_hdr)))
    assert sorted(s for s in syms if s.startswith("rvc_debug_")) == dbg_declared
    assert sorted(s for s in syms if not s.startswith("rvc_debug_")) == _declared()
    lib = _native.lib()
    lib.rvc_debug_option.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    assert lib.rvc_debug_option(b"RVC_C32S_DBG", b"7") == -1
    # every hook the product accepts is a planner CHOICE between kernels / tiles / plan structures (plan.hip kTestHooks); the names are listed in DESIGN.md
    plan = open(os.path.join(_native.CSRC, "plan.hip")).read()
    hooks = re.findall(r'"(RVC_[A-Z0-9_]+)"', plan[plan.index("kTestHooks[]"):plan.index("};", plan.index("kTestHooks[]"))])
    assert "RVC_C32S_DBG" not in hooks and len(hooks) >= 15
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for h in hooks:
        assert h in design, h


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from obs_rvc_amd.rvc import RvcInfer
    with pytest.raises(RvcInferError) as e:
        RvcInfer("/nonexistent")
    assert e.value.kind == "Backend"


def test_product_does_not_touch_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "obs_rvc_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f), errors="ignore").read()
                # no import / link / dlopen / include of anything under oracle/
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "librvc_oracle" not in src and not re.search(r"#include\s*[<\"].*oracle", src), f


def test_enums_mirror_rvc_common():
    assert RvcModelVersion.V1.text_encoder_in_channels() == 256 and RvcModelVersion.V1.output_layers() == 9
    assert RvcModelVersion.V2.text_encoder_in_channels() == 768 and RvcModelVersion.V2.output_layers() == 12
    assert RvcModelVersion.from_value("v1") is RvcModelVersion.V1 and RvcModelVersion.from_value("bogus") is RvcModelVersion.V2
    assert RvcModelVersion.from_value(1) is RvcModelVersion.V1 and RvcModelVersion.from_value(7) is RvcModelVersion.V2
    assert str(RvcModelVersion.V2) == "v2" and int(RvcModelVersion.V1) == 1
    assert RvcModelVersion.is_valid(2) and not RvcModelVersion.is_valid(3)
    assert PitchAlgorithm.from_value("anything") is PitchAlgorithm.Rmvpe and str(PitchAlgorithm.Rmvpe) == "rmvpe"
    assert PitchAlgorithm.is_valid(1) and not PitchAlgorithm.is_valid(2)
    assert RvcInferError(1).kind == "ModelNotLoaded" and RvcInferError(5).kind == "NdarrayShapeError"


def test_geometry_matches_plugin_formulas():
    g = geometry.BASELINE_160MS      # SURVEY.md section 8 header
    assert (g.sample_frame_16k, g.input_buffer_16k_size, g.skip_head, g.model_return_length, g.model_return_size) == (2560, 35840, 200, 21, 10080)
    d = geometry.derive()            # plugin defaults: 0.30 s, 40 k
    assert (d.sample_frame_16k, d.input_buffer_16k_size, d.model_return_length, d.model_return_size) == (4800, 38080, 35, 14000)
    assert d.sola_buffer_frame_size == 1920 and d.sola_search_frame_size == 480


def test_geometry_rounds_halves_away_from_zero():
    # lib.rs:202 uses f64::round(): 0.125 s at 48 kHz is 12.5 hops -> 13 (Python's round() would give 12); the native session
    # uses llround() (tests/test_postprocess.py compares the two on the GPU)
    g = geometry.derive(48000, 0.125, 0.065, 2.005, 48000)
    assert g.sample_frame_size == 13 * 480 and g.sample_frame_16k == 13 * 160
    assert g.crossfade_frame_size == 7 * 480 and g.extra_frame_size == 201 * 480
    assert geometry.derive(48000, 0.16, 0.07, 2.0, 48000) == geometry.BASELINE_160MS


def test_blob_roundtrip(tmp_path):
    t = {"a.w": np.arange(24, dtype=np.float32).reshape(2, 3, 4), "b": np.array([1.5], np.float32)}
    p = str(tmp_path / "x.rvcw")
    W.write_blob(p, {"k": 3, "f": 0.5}, t)
    cfg, tens = W.read_blob(p)
    assert cfg == {"k": 3.0, "f": 0.5}
    assert np.array_equal(tens["a.w"], t["a.w"]) and tens["a.w"].shape == (2, 3, 4) and tens["b"][0] == 1.5


def test_model_zoo_is_deterministic_and_sized():
    c1, t1 = W.make_synth("tiny", 48, seed=5)
    c2, t2 = W.make_synth("tiny", 48, seed=5)
    assert all(np.array_equal(t1[k], t2[k]) for k in t1)
    cfg, t = W.make_contentvec("full", 2)
    n = sum(v.size for v in t.values())
    assert 94e6 < n < 95e6                       # ContentVec-base ~94.4 M parameters
    cfg, t = W.make_rmvpe("full")
    assert 90e6 < sum(v.size for v in t.values()) < 91e6   # RMVPE 90.4 M (BN folded)


def test_shard_streams_round_robin():
    sh = dist.shard_streams(512, 8)
    assert [len(s) for s in sh] == [64] * 8 and sh[3][:3] == [3, 11, 19]
    assert sorted(sum(dist.shard_streams(13, 4), [])) == list(range(13))
    assert dist.local_streams(5, 1, 2) == [1, 3]


def test_header_is_plain_c(tmp_path):
    # the boundary is a C ABI: the header must compile as C99 (no C++-isms outside the extern "C" guards)
    import shutil, subprocess
    if not shutil.which("gcc"):
        pytest.skip("gcc not found")
    src = tmp_path / "abi_check.c"
    src.write_text('#include "rvc_mi355x.h"\nint main(void) { rvc_engine *e = 0; rvc_session *s = 0; rvc_resampler *r = 0; (void)e; (void)s; (void)r; return (int)RVC_OK; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


def test_debug_spec_mirrors_match_the_header(tmp_path):
    # tests/debug_abi.py restates the structs of include/rvc_mi355x_debug.h for ctypes: the size of each and the offset of every field, as the host C
    # compiler lays them out, against the mirrors (a field added to one side only would shift everything behind it without any GPU test saying why)
    import shutil, subprocess
    import debug_abi as D
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler found")
    mirrors = [("rvc_debug_layer_spec", D.LayerSpec), ("rvc_debug_op_spec", D.OpSpec), ("rvc_debug_front_spec", D.FrontSpec), ("rvc_debug_stream_state", D.StreamState),
               ("rvc_debug_rm_block_spec", D.RmBlockSpec), ("rvc_debug_retrieval_spec", D.RetrievalSpec),
               ("rvc_debug_post_spec", D.PostSpec)]
    c_name = {"cache": "cache_pitchf"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rvc_mi355x_debug.h"', 'int main(void) {']
    want = []
    for cname, mirror in mirrors:
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(ctypes.sizeof(mirror))
        for f, _ in mirror._fields_:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, c_name.get(f, f)))
            want.append(getattr(mirror, f).offset)
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0; }", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want, (got, want)


def _c_decls(text):
    """name -> parameter count of every function declared in the C header (comments stripped)."""
    import re
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(rvc_\w+)\s*\(([^;{]*?)\)\s*;", text):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_rust_ffi_matches_header():
    # bindings/rust/rvc/src/ffi.rs is hand-written (no Rust toolchain in the image): every extern "C" item must exist in
    # include/rvc_mi355x.h with the same number of parameters, and every header entry point must be declared there
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = _c_decls(open(os.path.join(root, "include", "rvc_mi355x.h")).read())
    ffi = open(os.path.join(root, "bindings", "rust", "rvc", "src", "ffi.rs")).read()
    rust = {}
    for m in re.finditer(r"pub fn (rvc_\w+)\s*\((.*?)\)\s*(?:->\s*[^;]+)?;", ffi, flags=re.S):
        args = m.group(2).strip()
        rust[m.group(1)] = 0 if not args else len([a for a in args.split(",") if a.strip()])
    assert set(hdr) == set(_native.SYMBOLS), set(hdr) ^ set(_native.SYMBOLS)
    assert set(rust) == set(hdr), set(rust) ^ set(hdr)
    for name, n in hdr.items():
        assert rust[name] == n, (name, rust[name], n)
    # the shim keeps the nine public methods of rvc/src/rvc.rs:30-220 with the reference's signatures
    shim = open(os.path.join(root, "bindings", "rust", "rvc", "src", "rvc.rs")).read()
    for sig in ("pub fn new(data_path: PathBuf) -> Self", "pub fn load_contentvec(&mut self, model_version: RvcModelVersion)",
                "pub fn load_model(&mut self, model_path: PathBuf)", "pub fn load_f0(&mut self, pitch_algorithm: PitchAlgorithm)",
                "pub fn unload_model(&mut self)", "pub fn hubert(&self, input: ArrayView1<f32>) -> Result<Array3<f32>, RvcInferError>",
                "pub fn extract_feature(&self, input: ArrayView1<f32>) -> Result<Array3<f32>, RvcInferError>",
                "pub fn pitch(&mut self, input: ArrayView1<f32>, pitch_shift: i32, sample_frame_16k_size: usize) -> Result<Array1<f32>, RvcInferError>",
                "pub fn infer("):
        assert sig in shim, sig


def _rust_pub_fns(text):
    """{name: (normalised argument list, normalised return type)} of the `pub fn`s of a Rust source"""
    import re
    out = {}
    for m in re.finditer(r"pub fn (\w+)\s*\((.*?)\)\s*(?:->\s*(.*?))?\s*\{", text, flags=re.S):
        norm = lambda t: re.sub(r"\s+", " ", (t or "").replace("ndarray::", "")).strip().rstrip(",").strip()
        args = [norm(a) for a in re.split(r",(?![^<>]*>)", m.group(2)) if norm(a)]
        out.setdefault(m.group(1), (args, norm(m.group(3))))
    return out


def test_rust_shim_signatures_match_the_reference():
    # bindings/rust/rvc/src/rvc.rs must keep the reference's public surface (rvc/src/rvc.rs:30-220): same method names, argument names
    # and types, return types -- modulo ort::Error -> BackendError (the one type of the API that named ONNX Runtime).  The reference
    # file is read where it lies (build container only); nothing of it is copied into the repo.
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ref_path = "/root/reference/rvc/src/rvc.rs"
    if not os.path.exists(ref_path):
        pytest.skip("reference sources not present on this machine")
    ref = _rust_pub_fns(open(ref_path).read())
    shim = _rust_pub_fns(open(os.path.join(root, "bindings", "rust", "rvc", "src", "rvc.rs")).read())
    nine = ["new", "load_contentvec", "load_model", "load_f0", "unload_model", "hubert", "extract_feature", "pitch", "infer"]
    assert [n for n in nine if n in ref] == nine, sorted(ref)
    for name in nine:
        assert name in shim, name
        rargs, rret = ref[name]
        sargs, sret = shim[name]
        assert sargs == rargs, (name, sargs, rargs)
        assert sret == rret.replace("ort::Error", "BackendError"), (name, sret, rret)


def test_rust_build_scripts_carry_the_library_path():
    # the library crate must not rely on rustc-link-arg (it does not reach dependent binaries) nor on a relative default path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    b = open(os.path.join(root, "bindings", "rust", "rvc", "build.rs")).read()
    code = "\n".join(ln for ln in b.splitlines() if not ln.lstrip().startswith("//"))
    assert "RVC_MI355X_LIB_DIR" in code and "cargo:libdir=" in code and "rustc-link-arg" not in code and "CARGO_MANIFEST_DIR" not in code
    assert 'links = "rvc_mi355x"' in open(os.path.join(root, "bindings", "rust", "rvc", "Cargo.toml")).read()
    r = open(os.path.join(root, "bindings", "rust", "rvc-rpc", "build.rs")).read()
    assert "DEP_RVC_MI355X_LIBDIR" in r and "cargo:rustc-link-arg-bins=-Wl,-rpath," in r
    assert '+build = "build.rs"' in open(os.path.join(root, "bindings", "rust", "rvc-rpc", "main.rs.patch")).read()
