"""The FCPE f0 method (rvc_load_f0_method(RVC_F0_FCPE), fcpe.hip.h + RMVPE's mel kernel + the implicit-GEMM planner + the pitch tail)
against the float64 restatement of tests/fcpe_ref.py: every stage by its tap, the depthwise kernel and the decoder alone through their debug entries, and the
public calls.  Micro sizes (H 64, I 128, 2 layers) at 32 frames unless a test names another.

Bounds are not invented here.  A stage's bound is 8 x the largest deviation of the same definition run in float32 numpy from float64 on the same input --
what single precision costs -- with a floor of 1e-6 x the tap's rms; every case prints base, bound and the device's error before it asserts.  fc.f0 is
judged against the float64 decoder applied to the device's own fc.prob: the decisions are then made on identical floats, so bins and voicing agree on every
frame and f0 within 1e-6 relative."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fcpe_ref as R
import yin_ref as Y
from common import BASELINE_160MS as g, voice_signal, zoo
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc_common import F0_FCPE, F0_RMVPE, RvcInferError

pytestmark = pytest.mark.gpu

FRAME16K = g.sample_frame_16k          # 2560
RL = g.model_return_length
SHIFT, CACHE_START = FRAME16K // 160, 1024 + 4 - 32          # rvc.rs:168,172 at 32 frames
_FP = C.POINTER(C.c_float)
assert FRAME16K == 2560 and Y.f0_frame(FRAME16K) == 4960


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """the tiny zoo with the micro FCPE next to rmvpe, a directory that holds the full-size FCPE alone, and the presets' tensors"""
    z = zoo("tiny")
    W.write_fcpe(z["data"], "micro")
    full = str(tmp_path_factory.mktemp("fcpe_full"))
    W.write_fcpe(full, "full")
    return {"zoo": z, "full": full, "micro_t": W.make_fcpe("micro")[1], "full_t": W.make_fcpe("full")[1]}


def _engine(data_dir, method="fcpe", streams=1, model=None):
    from obs_rvc_amd.rvc import RvcInfer
    e = RvcInfer(data_dir)
    if model:
        e.load_contentvec(2); e.load_model(model)
    e.load_f0_method(method)
    if streams > 1:
        e.set_streams(streams)
    e.set_noise_seed(1234, 0)
    return e


def _judge(what, got, ref, f32):
    ref, f32, got = np.asarray(ref, np.float64), np.asarray(f32, np.float64), np.asarray(got, np.float64).reshape(np.shape(ref))
    rms, base = float(np.sqrt(np.mean(ref ** 2))), float(np.max(np.abs(f32 - ref)))
    bound, err = max(8.0 * base, 1e-6 * rms), float(np.max(np.abs(got - ref)))
    print("%s: rms %.3e  float32 base %.3e  bound %.3e  device error %.3e  device range %.4g .. %.4g" % (what, rms, base, bound, err, got.min(), got.max()))
    assert np.all(np.isfinite(got)) and err <= bound, (what, err, bound)


def _check_f0_on_own_prob(e, stream, thr=R.THRESHOLD, what=""):
    """fc.f0 against the float64 decoder on the device's fc.prob: every bin and voicing decision, f0 within 1e-6 relative, no frame left out"""
    prob = e.tap("fc.prob", stream).reshape(-1, 360)
    f0 = e.tap("fc.f0", stream).reshape(-1).astype(np.float64)
    ref = R.decode(prob, thr)
    assert np.array_equal(f0 > 0, ref["f0"] > 0), np.where((f0 > 0) != (ref["f0"] > 0))
    v = ref["f0"] > 0
    err = float(np.max(np.abs(f0[v] - ref["f0"][v]) / ref["f0"][v])) if v.any() else 0.0
    print("%s fc.f0 on the device's fc.prob: voiced %d of %d, largest relative error %.3e (bound 1e-6)" % (what, v.sum(), len(v), err))
    assert err <= 1e-6
    return int(v.sum())


def _check_stages(e, t, x, frame16k=FRAME16K, stream=0, what=""):
    r64, r32 = R.fcpe(t, x, frame16k), R.fcpe(t, x, frame16k, dtype=np.float32)
    for name in R.stage_names(t):
        if name == "f0":
            continue
        _judge("%s fc.%s" % (what, name), e.tap("fc." + name, stream), r64[name], r32[name])
    return _check_f0_on_own_prob(e, stream, what=what)


# ------------------------------------------------------------------------------------------------ every tap
def test_stages_against_float64(data):
    x = Y.composite_signal()
    e = _engine(data["zoo"]["data"])
    assert e.f0_method == F0_FCPE and e.fcpe_threshold == 0.006
    e.enable_taps(True)
    f0 = e.pitch(x, 0, FRAME16K)
    assert f0.shape == (32,) and np.all(np.isfinite(f0))
    assert _check_stages(e, data["micro_t"], x, what="micro") >= 8
    assert np.array_equal(f0, e.tap("fc.f0").reshape(-1))          # no pitch shift, no controls: the tail passes the raw f0 on
    e.close()


def test_stages_at_64_frames(data):
    """n == frame, a window of the file converter (k = 2, tests/long_shapes.py's smallest geometry): the f0 window starts at sample 0 of the buffer"""
    x = Y.whole_window_signal(5120)
    assert len(x) == Y.f0_frame(5120)
    e = _engine(data["zoo"]["data"])
    e.enable_taps(True)
    assert e.pitch(x, 0, 5120).shape == (64,)
    _check_stages(e, data["micro_t"], x, frame16k=5120, what="64 frames")
    e.close()


def test_stages_three_streams(data):
    z = data["zoo"]
    xs = np.stack([voice_signal(g.input_buffer_16k_size, seed=s + 1) for s in range(3)])
    xs[2, -4960:] = Y.composite_signal()[-4960:]
    e = _engine(z["data"], streams=3, model=z["model"])
    e.enable_taps(True)
    y = e.infer_batch(xs, FRAME16K, (0, 0, 0), g.skip_head, RL)
    assert np.all(np.isfinite(y))
    for s in (0, 2):
        _check_stages(e, data["micro_t"], xs[s], stream=s, what="stream %d" % s)
    e.close()


def test_full_size_posteriors(data):
    """upstream's sizes (H 512, I 1024, 6 layers), one stream, 32 frames: fc.prob and fc.f0"""
    x = Y.composite_signal()
    t = data["full_t"]
    r64, r32 = R.fcpe(t, x, FRAME16K), R.fcpe(t, x, FRAME16K, dtype=np.float32)
    e = _engine(data["full"])
    e.enable_taps(True)
    e.pitch(x, 0, FRAME16K)
    _judge("full fc.prob", e.tap("fc.prob"), r64["prob"], r32["prob"])
    _check_f0_on_own_prob(e, 0, what="full")
    e.close()


# ------------------------------------------------------------------------------------------------ the depthwise kernel alone
@pytest.fixture(scope="module")
def bare_engine(data):
    e = _engine(data["zoo"]["data"], "yin")          # the debug entries need an engine, no weights
    yield e
    e.close()


def _dw(e, z, w, b):
    z, w, b = (np.ascontiguousarray(a, np.float32) for a in (z, w, b))
    B, I2, T = z.shape
    y = np.empty((B, I2 // 2, T), np.float32)
    rc = e._L.rvc_debug_fcpe_dw(e._h, z.ctypes.data_as(_FP), w.ctypes.data_as(_FP), b.ctypes.data_as(_FP), B, I2 // 2, T, y.ctypes.data_as(_FP))
    assert rc == 0, rc
    return y


def _dw_ref(z, w, b, dtype):
    return np.stack([R.glu_dw_silu(zz.astype(dtype), w.astype(dtype), b.astype(dtype)) for zz in z])


@pytest.mark.parametrize("T", [16, 32, 65, 101])
@pytest.mark.parametrize("kind", ["tap0", "tap30", "per_channel"])
def test_depthwise_adversarial(bare_engine, T, kind):
    """three streams of different signals, 40 channels (two full channel blocks and half of a third); T = 16 is shorter than the filter, 65 one past the time
    tile, 101 odd.  A filter that is 1 at tap 0 only reads frame t - 15, at tap 30 only frame t + 15: direction and zero padding; a different filter per
    channel: no channel takes another's.  A stream's edges see zeros, never a neighbour"""
    rng = np.random.default_rng(1000 + T)
    B, I = 3, 40
    z = rng.standard_normal((B, 2 * I, T)).astype(np.float32) * np.array([1.0, 3.0, 0.3], np.float32)[:, None, None]
    b = (0.1 * rng.standard_normal(I)).astype(np.float32)
    w = np.zeros((I, 31), np.float32)
    if kind == "tap0":
        w[:, 0] = 1.0
    elif kind == "tap30":
        w[:, 30] = 1.0
    else:
        w = rng.standard_normal((I, 31)).astype(np.float32) * (1.0 + np.arange(I, dtype=np.float32)[:, None] / I)
    got = _dw(bare_engine, z, w, b)
    _judge("dw %s T %d" % (kind, T), got, _dw_ref(z, w, b, np.float64), _dw_ref(z, w, b, np.float32))
    if kind != "per_channel":          # what the one-tap filters are for, stated directly: a shift by 15 frames with zeros coming in
        u = (z[:, :I] * (1.0 / (1.0 + np.exp(-z[:, I:].astype(np.float64))))).astype(np.float64)
        sh = np.zeros_like(u)
        if kind == "tap0":
            sh[:, :, 15:] = u[:, :, :max(T - 15, 0)]
        else:
            sh[:, :, :max(T - 15, 0)] = u[:, :, 15:]
        pre = sh + b[None, :, None]
        assert np.max(np.abs(got - pre / (1.0 + np.exp(-pre)))) < 1e-5 * max(1.0, np.abs(pre).max())


# ------------------------------------------------------------------------------------------------ the decoder alone
def _decode(e, prob):
    prob = np.ascontiguousarray(prob, np.float32)
    B, Tm, _ = prob.shape
    f0, bins = np.empty((B, Tm), np.float32), np.empty((B, Tm), np.int32)
    rc = e._L.rvc_debug_fcpe_decode(e._h, prob.ctypes.data_as(_FP), B, Tm, f0.ctypes.data_as(_FP), bins.ctypes.data)
    assert rc == 0, rc
    return f0, bins


def _check_decode(f0, bins, prob, thr):
    for b in range(len(prob)):
        ref = R.decode(prob[b], thr)
        assert np.array_equal(bins[b], ref["bins"]), np.where(bins[b] != ref["bins"])
        assert np.array_equal(f0[b] > 0, ref["f0"] > 0), np.where((f0[b] > 0) != (ref["f0"] > 0))
        v = ref["f0"] > 0
        if v.any():
            assert np.max(np.abs(f0[b][v] - ref["f0"][v]) / ref["f0"][v]) <= 1e-6


@pytest.mark.parametrize("B", [1, 3])
def test_decoder_alone(bare_engine, B):
    e = bare_engine
    e.set_fcpe_threshold(0.006)
    # ridges with decoys: the decoder follows the decoy, frame by frame
    cases = [R.ridge_case(32, 320 + b) for b in range(B)]
    prob = np.stack([c[0] for c in cases])
    f0, bins = _decode(e, prob)
    _check_decode(f0, bins, prob, 0.006)
    assert all(bins[b, t] == k for b, c in enumerate(cases) for t, k in c[2].items()) and np.all(f0 > 0)
    # exact ties (the lower bin), peaks at both edges with their clamped windows, all below the threshold, a peak under 50 Hz
    p = np.full((B, 8, 360), 0.01, np.float32)
    p[:, 0, [100, 200]] = 0.9
    p[:, 1, :] = 0.5
    for r, k in ((2, 0), (3, 3), (4, 356), (5, 359)):
        p[:, r, k] = 0.9; p[:, r, max(k - 1, 0)] = max(0.2, p[0, r, max(k - 1, 0)]); p[:, r, min(k + 1, 359)] = max(0.4, p[0, r, min(k + 1, 359)])
    p[:, 6, :] = 0.005; p[:, 6, 150] = 0.0059
    p[:, 7, 10] = 0.9
    f0, bins = _decode(e, p)
    _check_decode(f0, bins, p, 0.006)
    assert bins[0].tolist() == [100, 0, 0, 3, 356, 359, 150, 10]
    assert f0[0, 0] > 0 and f0[0, 4] > 1900 and f0[0, 5] > f0[0, 4] and np.all(f0[:, [1, 2, 3, 6, 7]] == 0)
    # a value exactly at the threshold is unvoiced, the next float above it voiced; the setter takes effect with nothing reloaded
    q = np.full((B, 3, 360), 0.001, np.float32)
    q[:, 0, 180] = 0.25; q[:, 1, 180] = np.nextafter(np.float32(0.25), np.float32(1)); q[:, 2, 180] = 0.2
    f0, _ = _decode(e, q)
    assert np.all(f0 > 0)
    e.set_fcpe_threshold(0.25)
    assert e.fcpe_threshold == 0.25
    f0, bins = _decode(e, q)
    _check_decode(f0, bins, q, 0.25)
    assert np.all(f0[:, 0] == 0) and np.all(f0[:, 1] > 0) and np.all(f0[:, 2] == 0)
    e.set_fcpe_threshold(0.006)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(RvcInferError) as ei:
            e.set_fcpe_threshold(bad)
        assert ei.value.kind == "NdarrayShapeError" and e.fcpe_threshold == 0.006


# ------------------------------------------------------------------------------------------------ the public calls
def _f0_bound(t, x):
    r64, r32 = R.fcpe(t, x, FRAME16K), R.fcpe(t, x, FRAME16K, dtype=np.float32)
    v = (r64["f0"] > 0) & (r32["f0"] > 0)
    base = float(np.max(np.abs(r32["f0"][v].astype(np.float64) - r64["f0"][v]) / r64["f0"][v])) if v.any() else 0.0
    return r64, r32, max(8.0 * base, 1e-6)


def _check_f0(got, r64, r32, bound):
    """against the float64 chain: frames on which the float32 and the float64 reference agree about bin and voicing (the others sit on a decision's edge)"""
    got = np.asarray(got, np.float64)
    sure = (r64["bins"] == r32["bins"]) & ((r64["f0"] > 0) == (r32["f0"] > 0))
    assert np.sum(~sure) <= 0.10 * len(got)
    assert np.array_equal(got[sure] > 0, r64["f0"][sure] > 0)
    v = sure & (r64["f0"] > 0)
    err = float(np.max(np.abs(got[v] - r64["f0"][v]) / r64["f0"][v])) if v.any() else 0.0
    print("voiced %d of %d, unsure %d, largest relative error %.3e (bound %.3e)" % (v.sum(), len(got), np.sum(~sure), err, bound))
    assert err <= bound


def test_pitch_against_the_reference(data):
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    x[-4960:] = Y.composite_signal()[-4960:]
    r64, r32, bound = _f0_bound(data["micro_t"], x)
    e = _engine(data["zoo"]["data"])
    got = e.pitch(x, 0, FRAME16K)
    assert got.shape == (32,)
    _check_f0(got, r64, r32, bound)
    for shift in (12, -7, -12):          # the pitch shift of rvc.rs:121 on top: a power of two, exact
        assert np.array_equal(e.pitch(x, shift, FRAME16K), got * np.float32(Y.uppower(shift)))
    e.close()


def test_streams_two_chunks(data):
    z = data["zoo"]
    sr = int(W.read_blob(z["model"])[0]["sr"])
    shifts = (12, 0, -7)
    xs = [np.stack([voice_signal(g.input_buffer_16k_size, seed=10 * k + s + 1) for s in range(3)]) for k in range(2)]
    xs[1][1, -4960:] = Y.composite_signal()[-4960:]
    e = _engine(z["data"], streams=3, model=z["model"])
    for k in range(2):
        y = e.infer_batch(xs[k], FRAME16K, shifts, g.skip_head, RL)
        assert y.shape == (3, RL * sr // 100) and np.all(np.isfinite(y))
    for s in range(3):
        c64, c32, bins64, bins32, bound = np.zeros(1024), np.zeros(1024), np.zeros(1024), np.zeros(1024), 1e-6
        for k in range(2):
            r64, r32, b = _f0_bound(data["micro_t"], xs[k][s])
            bound = max(bound, b)
            c64, _ = Y.update_cache(c64, r64["f0"] * Y.uppower(shifts[s]), SHIFT, CACHE_START, 0, 0)
            c32, _ = Y.update_cache(c32, r32["f0"].astype(np.float64) * Y.uppower(shifts[s]), SHIFT, CACHE_START, 0, 0)
            bins64, _ = Y.update_cache(bins64, r64["bins"].astype(np.float64), SHIFT, CACHE_START, 0, 0)
            bins32, _ = Y.update_cache(bins32, r32["bins"].astype(np.float64), SHIFT, CACHE_START, 0, 0)
        got = e.pitch_cache(s)
        lo = CACHE_START - SHIFT
        assert np.all(got[:lo] == 0.0)
        _check_f0(got[lo:], dict(f0=c64[lo:], bins=bins64[lo:]), dict(f0=c32[lo:], bins=bins32[lo:]), bound)
    e.close()


def test_plan_identity_threshold_and_graph_replay(data):
    z = data["zoo"]
    x = Y.composite_signal()
    e = _engine(z["data"], "rmvpe", model=z["model"])
    builds = lambda: e.plan_cache_info()["builds"]
    n = builds()
    rm = e.pitch(x, 0, FRAME16K); assert builds() == n + 1
    e.load_f0_method("fcpe")
    fc = e.pitch(x, 0, FRAME16K); assert builds() == n + 2 and e.f0_method == F0_FCPE
    # rmvpe -> fcpe -> rmvpe: each method's plan serves only that method.  Loading RMVPE is rvc_load_f0, which reads its file again and drops every plan (as it
    # did before FCPE existed), so that step builds; FCPE's weights stay loaded across it
    e.load_f0_method("rmvpe")
    assert np.array_equal(e.pitch(x, 0, FRAME16K), rm) and e.f0_method == F0_RMVPE and not np.array_equal(fc, rm)
    e.load_f0_method("fcpe")
    n = builds()
    assert np.array_equal(e.pitch(x, 0, FRAME16K), fc) and builds() == n + 1
    # fcpe -> yin -> fcpe: going back hits the cache
    e.load_f0_method("yin")
    yin = e.pitch(x, 0, FRAME16K); assert builds() == n + 2 and not np.array_equal(yin, fc)
    e.load_f0_method("fcpe")
    assert np.array_equal(e.pitch(x, 0, FRAME16K), fc) and builds() == n + 2
    e.load_f0_method("yin")
    assert np.array_equal(e.pitch(x, 0, FRAME16K), yin) and builds() == n + 2
    e.load_f0_method("fcpe")
    # the threshold holds from the next call on, with nothing reloaded: a plan of its own, and the old value finds its plan again
    e.enable_taps(True)
    e.pitch(x, 0, FRAME16K)
    peak = e.tap("fc.prob").reshape(32, 360).max(axis=1)
    e.enable_taps(False)
    thr = float(np.sort(peak)[16])          # half of the frames have their peak at or below it
    e.set_fcpe_threshold(thr)
    n = builds()
    hi = e.pitch(x, 0, FRAME16K)
    assert builds() == n + 1 and np.all(hi[peak <= thr] == 0) and np.array_equal(hi[peak > thr], fc[peak > thr])
    e.set_fcpe_threshold(0.006)
    assert np.array_equal(e.pitch(x, 0, FRAME16K), fc) and builds() == n + 1
    # graph replay: the same pitch cache, bit for bit
    xv = voice_signal(g.input_buffer_16k_size, seed=3)
    xv[-4960:] = x[-4960:]
    e.infer(xv, FRAME16K, 12, g.skip_head, RL)
    eager = e.pitch_cache()
    e.reset_state()
    e.set_use_graph(True)
    e.infer(xv, FRAME16K, 12, g.skip_head, RL)
    assert np.array_equal(e.pitch_cache(), eager) and np.any(eager > 0)
    e.close()


def test_missing_file_and_unknown_method(tmp_path):
    from obs_rvc_amd.rvc import RvcInfer
    e = RvcInfer(str(tmp_path))                      # a data directory without f0/
    statuses = {}
    for name, call in (("rmvpe", e.load_f0), ("fcpe", lambda: e.load_f0_method("fcpe")), ("fcpe7", lambda: e.load_f0_method(7))):
        with pytest.raises(RvcInferError) as ei:
            call()
        statuses[name] = ei.value.kind
        assert e.f0_method == 0
    assert statuses["fcpe"] == statuses["fcpe7"] == statuses["rmvpe"] == "Backend"
    for bad in (3, 6, 8, -1):
        with pytest.raises(RvcInferError) as ei:
            e.load_f0_method(bad)
        assert ei.value.kind == "NdarrayShapeError" and all(w in str(ei.value) for w in ("RMVPE", "YIN", "CREPE", "CREPE_TINY", "FCPE"))
    with pytest.raises(ValueError):
        e.load_f0_method("harvest")
    W.write_fcpe(str(tmp_path), "micro")
    e.load_f0_method("fcpe")
    f0 = e.pitch(Y.composite_signal(), 0, FRAME16K)
    assert e.f0_method == F0_FCPE and f0.shape == (32,) and np.all(np.isfinite(f0))
    e.close()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_session_chunk_is_the_composition(data):
    """one chunk through the native session against the same chunk through StreamingSession, which is the composition of public calls (the converters,
    rvc_infer, envelope mixing, rvc_sola_step) on a second engine: the posteriors, FCPE's raw f0, the tail's f0, the pitch cache, the ContentVec output,
    the SOLA offset and the frame itself, bit for bit"""
    from obs_rvc_amd.geometry import derive
    from obs_rvc_amd.resample import FftFixedInOut
    from obs_rvc_amd.streaming import NativeStreamingSession, StreamingSession
    z = data["zoo"]
    sr = int(W.read_blob(z["model"])[0]["sr"])
    e1, e2 = _engine(z["data"], model=z["model"]), _engine(z["data"], model=z["model"])
    for e in (e1, e2):
        e.enable_taps(2)
    gg = derive(48000, 0.16, 0.07, 2.0, sr)
    nat = NativeStreamingSession(e1, 48000, 0.16, 0.07, 2.0, sr, 12, 0.6)
    pys = StreamingSession(e2, gg, 12, 0.6, sr, lambda ri, ro, n: FftFixedInOut(e2, ri, ro, n))
    assert nat.sample_frame_16k == FRAME16K
    F = nat.sample_frame_size
    rng = np.random.default_rng(5)
    t = np.arange(F) / 48000.0
    audio = (0.2 * sum(np.sin(2 * np.pi * 150.0 * k * t) / k for k in range(1, 5)) + 1e-3 * rng.standard_normal(F)).astype(np.float32)
    fn, fp = nat.process_one_frame(audio), pys.process_one_frame(audio)
    assert fn.shape == (F,) and np.all(np.isfinite(fn))
    for name in ("fc.prob", "fc.f0", "f0", "cv.out"):
        assert _same_bits(e1.tap(name), e2.tap(name)), name
    assert _same_bits(e1.pitch_cache(), e2.pitch_cache())
    assert nat.last_sola_offset == pys.last_sola_offset and _same_bits(fn, fp)
    del nat
    e1.close(); e2.close()


def test_convert_of_three_windows_is_the_composition(data):
    """rvc_convert with FCPE against tests/test_gpu_convert.py's composition of public calls (numpy window gather, reset_state, infer_batch per batch,
    sola_stitch): audio and offsets bit for bit"""
    import test_gpu_convert as TC
    x = voice_signal(160 * 150, seed=11)
    assert TC.RvcInfer.convert_geometry(len(x), 100 * TC.ZC, TC.K, TC.CTX, TC.XF)["windows"] == 3
    e = TC.engine(3, "fcpe")
    ref, ref_off = TC.composition(e, x)
    got, rate = TC.guard(e.convert, x, k=TC.K, context=TC.CTX, crossfade=TC.XF, pitch_shift=TC.SHIFT, highpass=False)
    info = e.convert_info()
    assert rate == 100 * TC.ZC and info["windows"] == 3 and info["batches"] == 1
    assert info["offsets"].tolist() == ref_off.tolist() and TC.same_bits(got, ref) and np.all(np.isfinite(got))
    assert e.f0_method == F0_FCPE
    e.close()
