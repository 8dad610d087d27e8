"""Models trained without pitch guidance on the GPU: seeded `tiny` / `tiny5` models written with make_synth(f0=False).

Stage by stage as tests/test_gpu_stream_taps.py does it, with that file's bounds: every stream of a batched plan has its own input and stream id, two
chunks are run, every tapped interval of the synthesizer is teacher-forced against its float64 value (tests/nof0_ref.py: synth_ref.py's stages, the embed
without the pitch term, the upsampling stage without the source) --

  * one launch (sy.emb, stats, prior, stretch, sy.pre, each sy.up{i}, post): e = max |gpu - ref64| / rms(ref64) <= TOL = 2e-5
  * multi-launch stages (encoder, encoder + stats, each flow, each ResBlock stage): e <= max(TOL, 4 delta32)
  * pure gathers (phone gather, the final flip): bitwise
  * the PCM against the whole float64 chain, which starts from the CPU oracle's ContentVec output of that stream's input and never sees the GPU: 1e-3
    absolute RMS; and cv.out against the same oracle output at that file's 1e-4 relative RMS

-- then an f0 twin with a zero pitch embedding and zero noise convolutions as an independent cross-check, the settings a no-f0 model ignores (bit for
bit, no plan built, pitch cache untouched), the plan's shape, and the public surface.  None of this loads on the parent commit: its ModelSY reads
sy.enc.pitch_emb unconditionally."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import debug_abi as D
import nof0_ref as NR
import synth_ref as SR
import test_gpu_stream_taps as T
from common import BASELINE_160MS as g, rel_rms, rms, voice_signal, zoo
from obs_rvc_amd import _native
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc_common import RvcInferError
from test_formant import back_to_model_rate, geometry

pytestmark = pytest.mark.gpu
TOL, PCM_TOL, SEED, ID0, SHIFTS = T.TOL, T.PCM_TOL, T.SEED, T.ID0, T.SHIFTS
_FP = C.POINTER(C.c_float)


@functools.lru_cache(maxsize=None)
def _model(preset, f0=False):
    """(zoo, path of the seeded model beside the zoo's own, cfg, tensors): the no-f0 kind, or (f0=True) its f0 twin"""
    z = zoo("tiny", 2, "tiny5") if preset == "tiny5" else zoo(preset)
    if f0:
        return (z, z["model"]) + W.read_blob(z["model"])
    path = os.path.join(os.path.dirname(z["model"]), "model-%s-nof0-v2.rvcw" % preset)
    cfg, tens = W.make_synth(preset, 48 if preset != "full" else 768, f0=False)
    if not os.path.exists(path):
        W.write_blob(path, cfg, tens)
    return z, path, cfg, tens


@functools.lru_cache(maxsize=None)
def _reference(preset, s, R, phi=0.0):
    """stream s of T._inputs, second chunk: (the oracle's ContentVec output [C][T], the float64 chain on it).  No GPU anywhere in it."""
    from oracle import oracle as O
    z, _, cfg, tens = _model(preset)
    x = voice_signal(g.input_buffer_16k_size, seed=1 + s + 20)             # T._inputs(S)[1][s]
    o = O.OracleRvcInfer(z["data"]); o.load_contentvec(2)
    cv = np.asarray(o.hubert(x), np.float32)
    o.close()
    cv = cv.reshape(cv.shape[-2], cv.shape[-1])
    I = int(cfg["inter"])
    eps = O.philox_normal(SEED, ID0 + s, 1, 0, I * R).reshape(I, R)
    R2 = geometry(R, int(cfg["sr"]), phi)[0] if phi else None
    st = NR.synth(cfg, tens, SR.phone_gather(cv, g.skip_head, R), eps, R2)
    if phi:
        upp = int(cfg["sr"]) // 100
        st["pcm"] = back_to_model_rate(st["pcm"], R, upp, geometry(R, int(cfg["sr"]), phi)[1])
    return cv, st


def _engine(preset, S=1, level=0, f0_method=None, formant=None, model=None):
    from obs_rvc_amd.rvc import RvcInfer
    z, path, _, _ = _model(preset)
    eng = RvcInfer(z["data"]); eng.load_contentvec(2)
    if f0_method:
        eng.load_f0_method(f0_method)
    eng.load_model(model or path)
    if S > 1:
        eng.set_streams(S)
    eng.set_noise_seed(SEED, ID0)
    for s, phi in (formant or {}).items():
        eng.set_formant_shift(phi, stream=s)
    if level:
        eng.enable_taps(level)
    return eng


def _run(eng, S, R, shifts=None):
    xs = T._inputs(S)
    for c in range(2):
        y = eng.infer_batch(xs[c], g.sample_frame_16k, np.array(SHIFTS[:S], np.int32) if shifts is None else shifts, g.skip_head, R)
    return y


def _stages(rep, cfg, tens, eng, p, gs, R, pcm):
    """T._synth_stages for a plan without a pitch: no pitchf, no source"""
    from oracle import oracle as O
    Cd, H, I, fn, n_ups = (int(cfg[k]) for k in ("phone_dim", "hidden", "inter", "flow_n", "n_ups"))

    def tap(name, rows):
        return eng.tap(name, p).reshape(rows, -1)

    def single(stage, got, fnc, *args):
        rep.add(gs, stage, SR.max_over_rms(got, fnc(*args)), TOL)

    def multi(stage, got, fnc, *args):
        ref, d32 = SR.stage_delta32(fnc, *args)
        rep.add(gs, stage, SR.max_over_rms(got, ref), max(TOL, 4 * d32), d32)

    phone = tap("phone_ct", Cd)
    assert phone.shape == (Cd, R)
    rep.bits(gs, "gather", phone, SR.phone_gather(tap("cv.out", Cd), g.skip_head, R))
    emb = tap("sy.emb", H)
    single("embed", emb, NR.embed, cfg, tens, phone)
    stats = tap("sy.stats", 2 * I)
    if T._has(eng, "sy.enc", p):
        enc = tap("sy.enc", H)
        multi("encoder", enc, SR.encoder, cfg, tens, emb)
        single("stats", stats, SR.stats, cfg, tens, enc)
    else:
        assert T._has(eng, "sy.enc.raw", p)
        multi("enc+stats", stats, SR.encoder_stats, cfg, tens, emb)
    zp = tap("sy.zp", I)
    single("prior", zp, SR.prior, cfg, stats, O.philox_normal(SEED, ID0 + gs, 1, 0, I * R).reshape(I, R))
    zin = zp
    for fi in reversed(range(fn)):
        zf = tap("sy.flow%d" % fi, I)
        multi("flow%d" % fi, zf, SR.flow, cfg, tens, fi, zin)
        zin = zf
    z = tap("sy.z", I)
    rep.bits(gs, "flip", z, SR.final_flip(cfg, zin))
    if T._has(eng, "sy.zi", p):
        zi = tap("sy.zi", I)
        single("stretch", zi, SR.latent_stretch, z, zi.shape[1])
        z = zi
    x = tap("sy.pre", int(cfg["up_init"]))
    single("pre", x, SR.dec_pre, cfg, tens, z)
    for i in range(n_ups):
        u = tap("sy.up%d" % i, int(cfg["up_init"]) >> (i + 1))
        single("up%d" % i, u, NR.dec_up, cfg, tens, i, x)
        x = tap("sy.rb%d" % i, int(cfg["up_init"]) >> (i + 1))
        multi("rb%d" % i, x, SR.dec_rb, cfg, tens, i, u)
    out = tap("sy.dec", 1) if T._has(eng, "sy.dec", p) else np.asarray(pcm).reshape(1, -1)
    single("post", out, SR.dec_post, cfg, tens, x)


def _no_pitch_taps(eng, p=0):
    for name in ("sy.src", "sy.srci", "pitchf", "f0", "no.such.tap"):
        with pytest.raises(RvcInferError) as a:
            eng.tap(name, p)
        with pytest.raises(RvcInferError) as b:
            eng.tap("no.such.tap", p)
        assert a.value.code == b.value.code, name             # what an unknown tap name gives


def _case(preset, S, level, R=g.model_return_length, formant=None, plan_streams=None):
    z, path, cfg, tens = _model(preset)
    eng = _engine(preset, S, level, formant=formant)           # (no f0 method loaded)
    assert eng.model_has_f0() is False and eng.f0_method == 0
    y = _run(eng, S, R)
    plan_streams = list(range(S)) if plan_streams is None else plan_streams
    rep = T.Report("nof0 %s S=%d R=%d taps=%d%s" % (preset, S, R, level, " formant" if formant else ""))
    for gs in plan_streams:
        p = plan_streams.index(gs)
        cv, st = _reference(preset, gs, R, (formant or {}).get(gs, 0.0))
        rep.add(gs, "cv.out", rel_rms(eng.tap("cv.out", p).reshape(cv.shape), cv), 1e-4)
        _stages(rep, cfg, tens, eng, p, gs, R, y[gs])
        e_pcm = rms(y[gs] - st["pcm"])
        print("nof0 %s S=%d stream %d PCM abs rms %.2e (bound %.0e)" % (preset, S, gs, e_pcm, PCM_TOL))
        assert y[gs].shape == st["pcm"].shape and e_pcm < PCM_TOL, (gs, e_pcm)
        _no_pitch_taps(eng, p)
    for s in range(S):
        assert not np.any(eng.pitch_cache(s)), s                # never written
    for name in ("cv.out", "phone_ct", "sy.emb", "sy.stats", "sy.flow0", "sy.z", "sy.up0", "sy.rb0"):
        rc, a = D.debug_tap(eng, name, 0)
        assert rc == 0 and D.same_bits(a, eng.tap(name)), name
    ops = eng.plan_ops()
    eng.close()
    rep.done()
    return ops, rep


# ---- stage by stage, every stream, both plan levels.  tiny: 1 | 2 one chain at one and at several streams, 5 past what would be the CU partition, 9 past
# ---- the composed WaveNets, 17 past the 16-stream LayerNorm / LDS-GEMM / fused-ResBlock rules
@pytest.mark.parametrize("S", [1, 2, 5, 9, 17])
def test_tiny_every_stream_both_plans(S):
    ops1, _ = _case("tiny", S, 1)
    ops2, _ = _case("tiny", S, 2)
    T._composed_or_not(_model("tiny")[2], S, ops1, ops2)


@pytest.mark.parametrize("S", [1, 3])          # tiny5: odd flow count, five upsampling stages, three ResBlock kernels
def test_tiny5_every_stream_both_plans(S):
    ops1, _ = _case("tiny5", S, 1)
    ops2, _ = _case("tiny5", S, 2)
    T._composed_or_not(_model("tiny5")[2], S, ops1, ops2)


@pytest.mark.parametrize("R", [1, 3])          # the shortest windows, shorter than the WaveNet's 5 taps
def test_tiny_shortest_windows(R):
    for level in (1, 2):
        _case("tiny", 2, level, R=R)


def test_tiny5_formant_shift_on_one_stream_of_three():
    # streams with different decoder lengths run one plan per length (infer_r2_buckets): the last plan is stream 1's alone, its latent stretched to R2,
    # its decoder on R2 frames, its output resampled back; there is no source to stretch
    for level in (1, 2):
        _, rep = _case("tiny5", 3, level, formant={1: 3.0}, plan_streams=[1])
        assert "stretch" in rep.worst


# ---- independent cross-check: an f0 model whose pitch embedding and noise convolutions are zero computes what its no-f0 twin computes
@pytest.mark.parametrize("S", [1, 5])
def test_f0_twin_with_zero_pitch_terms(S, tmp_path):
    z, path, cfg, tens = _model("tiny")
    cfg1, t1 = W.make_synth("tiny", 48)
    t1 = dict(t1)
    for k in t1:
        if k == "sy.enc.pitch_emb" or k.startswith("sy.dec.nc"):
            t1[k] = np.zeros_like(t1[k])
    assert all(t1[k].tobytes() == tens[k].tobytes() for k in tens)
    twin_path = str(tmp_path / "twin.rvcw")
    W.write_blob(twin_path, cfg1, t1)
    ea, eb = _engine("tiny", S), _engine("tiny", S, f0_method="yin", model=twin_path)
    assert ea.model_has_f0() is False and eb.model_has_f0() is True
    ya, yb = _run(ea, S, g.model_return_length), _run(eb, S, g.model_return_length)
    assert eb.plan_ops() > ea.plan_ops()
    ea.close(); eb.close()
    for s in range(S):
        e = SR.max_over_rms(yb[s], ya[s])
        print("twin S=%d stream %d: max |f0 twin - nof0| / rms %.2e (bound %.0e)" % (S, s, e, TOL))
        assert ya[s].shape == yb[s].shape and e <= TOL, (s, e)


# ---- what a no-f0 model ignores: bit for bit, no plan built, pitch cache untouched
def test_ignored_settings_change_no_bit_and_build_no_plan():
    eng = _engine("tiny")
    x = T._inputs(1)[0][0]
    R = g.model_return_length

    def run(shift=0):
        eng.reset_state()
        y = eng.infer(x, g.sample_frame_16k, shift, g.skip_head, R)
        assert not np.any(eng.pitch_cache(0))
        return y
    base = run()
    builds = eng.plan_cache_info()["builds"]

    def same(what, y):
        assert D.same_bits(y, base), what
        assert eng.plan_cache_info()["builds"] == builds, what
    same("again", run())
    eng.load_f0_method("yin")
    same("YIN loaded", run())
    same("pitch_shift 12", run(12))
    same("pitch_shift None", run(None))
    same("infer_batch, pitch_shift None", (eng.reset_state(), eng.infer_batch(x[None], g.sample_frame_16k, None, g.skip_head, R)[0])[1])
    eng.set_pitch_semitones(5.0); same("semitones 5", run()); eng.set_pitch_semitones(0.0)
    eng.set_f0_median(3); same("median 3", run()); eng.set_f0_median(0)
    eng.set_f0_snap("C major", 1.0); same("snap on", run()); eng.set_f0_snap(0, 0.0)
    same("snap off", run())
    eng.set_crepe_decoder("argmax"); same("crepe decoder", run())
    # with an index: protect 0.2 against 0.5 (off)
    eng.load_index(np.random.default_rng(5).standard_normal((64, 48)).astype(np.float32))
    eng.set_index_rate(0.5)
    base = run()
    assert not D.same_bits(base, eng.infer(x, g.sample_frame_16k, 0, g.skip_head, R))      # (the chunk counter has advanced: another prior sample)
    builds = eng.plan_cache_info()["builds"]
    eng.set_protect(0.2); same("protect 0.2", run())
    eng.set_protect(0.5); same("protect 0.5", run())
    eng.close()


# ---- plan shape
def test_plan_is_a_single_chain_and_smaller():
    R = g.model_return_length
    x = T._inputs(1)[0]
    ea = _engine("tiny")
    ea.infer_batch(x, g.sample_frame_16k, 0, g.skip_head, R)
    ops0 = ea.plan_ops()
    with pytest.raises(RvcInferError):
        ea.tap("sy.z")                                           # no taps on this plan
    ea.close()
    eb = _engine("tiny", f0_method="yin", model=_model("tiny", True)[1])
    eb.infer_batch(x, g.sample_frame_16k, 0, g.skip_head, R)
    ops1 = eb.plan_ops()
    eb.close()
    n_ups = int(_model("tiny")[2]["n_ups"])
    print("plan_ops: no-f0 %d, f0 with YIN %d" % (ops0, ops1))
    assert ops0 <= ops1 - (n_ups + 2), (ops0, ops1)              # the source, n_ups noise convolutions, at least one tracker launch
    et = _engine("tiny", 1, 2)
    et.infer_batch(x, g.sample_frame_16k, 0, g.skip_head, R)
    _no_pitch_taps(et)
    et.close()


def test_graph_replay_gives_the_eager_bits():
    R = g.model_return_length
    xs = [voice_signal(g.input_buffer_16k_size, seed=60 + c) for c in range(3)]
    ea, eb = _engine("tiny"), _engine("tiny")
    eb.set_use_graph(True)
    for c in range(3):
        ya = ea.infer(xs[c], g.sample_frame_16k, None, g.skip_head, R)
        yb = eb.infer(xs[c], g.sample_frame_16k, None, g.skip_head, R)
        assert D.same_bits(ya, yb), c
    assert ea.plan_cache_info()["builds"] == eb.plan_cache_info()["builds"] == 1
    ea.close(); eb.close()


# ---- public surface
def test_model_has_f0_and_statuses():
    from obs_rvc_amd.rvc import RvcInfer
    L = _native.lib()
    z, path, _, _ = _model("tiny")
    x = T._inputs(1)[0][0]
    R = g.model_return_length
    out, n = np.empty(R * 1024 + 16, np.float32), C.c_size_t()

    def infer(e):
        return L.rvc_infer(e._h, x.ctypes.data_as(_FP), len(x), g.sample_frame_16k, 0, 0, g.skip_head, R, out.ctypes.data_as(_FP), len(out), C.byref(n))
    e = RvcInfer(z["data"]); e.load_contentvec(2)
    assert L.rvc_model_has_f0(e._h) == -1 and e.model_has_f0() is None and L.rvc_model_has_f0(None) == -1
    e.load_model(z["model"])
    assert L.rvc_model_has_f0(e._h) == 1 and e.model_has_f0() is True
    assert infer(e) == 3                                         # RVC_F0_NOT_LOADED: an f0 model still needs its method
    e.load_model(path)
    assert L.rvc_model_has_f0(e._h) == 0 and e.model_has_f0() is False
    assert infer(e) == 0 and n.value == R * 48
    # rvc_pitch is the tracker's: unchanged
    f0 = np.empty(4096, np.float32)
    assert L.rvc_pitch(e._h, x.ctypes.data_as(_FP), len(x), 0, g.sample_frame_16k, f0.ctypes.data_as(_FP), 4096, C.byref(n)) == 3
    e.unload_model()
    assert L.rvc_model_has_f0(e._h) == -1
    e.load_model(path)
    # chunk pipelining has no front pair to overlap here
    e.set_pipeline(True)
    assert infer(e) == 5 and len(L.rvc_last_error_message(e._h)) > 0 and b"pipelin" in L.rvc_last_error_message(e._h)
    e.set_pipeline(False)
    assert infer(e) == 0
    e.close()


def test_session_convert_and_knn_with_an_index():
    from obs_rvc_amd.streaming import NativeStreamingSession
    R = g.model_return_length
    index = np.random.default_rng(5).standard_normal((64, 48)).astype(np.float32)
    x = T._inputs(1)[0][0]
    hits = []
    for f0_method, model in ((None, None), ("yin", _model("tiny", True)[1])):
        e = _engine("tiny", f0_method=f0_method, model=model)
        e.load_index(index); e.set_index_rate(0.5)
        e.infer(x, g.sample_frame_16k, 0, g.skip_head, R)
        hits.append(e.knn())
        e.close()
    (ia, da), (ib, db) = hits
    assert ia.shape == ib.shape and ia.shape[0] == R and np.array_equal(ia, ib) and np.allclose(da, db, rtol=1e-5, atol=0)      # the retrieval sees ContentVec alone
    # the native session, three chunks
    e = _engine("tiny")
    e.load_index(index); e.set_index_rate(0.5)
    nat = NativeStreamingSession(e, 48000, 0.16, 0.07, 2.0, 4800, 12, 0.6)
    F = nat.sample_frame_size
    a = np.interp(np.arange(F * 3) / 48000.0, np.arange(F) / 16000.0, voice_signal(F, seed=10)).astype(np.float32)
    frames = [nat.process_one_frame(a[c * F:(c + 1) * F]) for c in range(3)]
    assert all(f.shape == (F,) and np.all(np.isfinite(f)) for f in frames) and rms(frames[-1]) > 0
    assert not np.any(e.pitch_cache(0))
    e.close()
    # the file converter: a 1 s signal at 2 streams
    e = _engine("tiny", 2)
    e.load_index(index); e.set_index_rate(0.5)
    sig = voice_signal(16000, seed=4)
    y, rate = e.convert(sig, k=2, context=3, crossfade=2, pitch_shift=None)
    assert rate == 4800 and y.shape == (4800,) and np.all(np.isfinite(y)) and rms(y) > 0
    y2, _ = e.convert(sig, k=2, context=3, crossfade=2, pitch_shift=12)
    assert D.same_bits(y, y2)
    assert e.convert_info()["windows"] >= 1
    e.close()
