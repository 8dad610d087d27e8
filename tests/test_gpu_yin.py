"""The YIN f0 method (rvc_load_f0_method, yin_f0_kernel + the pitch tail) against the float64 restatement of tests/yin_ref.py:
method loading, rvc_pitch, several streams through two chunks, plan identity between the methods, graph replay, formant shift, the native session.
The smallest geometry: sample_frame_16k_size = 2560, an f0 window of 4960 samples, 32 frames.

The bound on a voiced frame's f0 is not invented here: the same recipe in float32 numpy deviates from float64 by at most 4.9e-8 (relative) on the
composite input -- what single precision costs -- and the kernel, whose summation order and division rounding are not numpy's, is allowed 8 times
the measured value with a floor of 1e-6: BOUND = max(8 x 4.9e-8, 1e-6) = 1e-6.  The `yin_case` fixture measures the base value again on every run.
Voicing (zero against non-zero) must agree on EVERY frame whose float64 decision margin min |d' - 0.15| is at least 1e-4; frames under it are
left out of the voicing check only, and at most 10 % of the frames may be (tests/test_yin_ref.py shows the input itself has none).
The kernel's own error has not been observed on a device yet; every case prints it before it asserts."""
from __future__ import annotations

import numpy as np
import pytest

import yin_ref as Y
from common import BASELINE_160MS as g, voice_signal, zoo
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc_common import F0_RMVPE, F0_YIN, RvcInferError

pytestmark = pytest.mark.gpu

FRAME16K = g.sample_frame_16k          # 2560
R = g.model_return_length
MARGIN = 1e-4
SHIFT, CACHE_START = FRAME16K // 160, 1024 + 4 - 32          # rvc.rs:168,172 at 32 frames
assert FRAME16K == 2560 and Y.f0_frame(FRAME16K) == 4960


def _engine(z, method="yin", streams=1, full=True):
    from obs_rvc_amd.rvc import RvcInfer
    e = RvcInfer(z["data"])
    if full:
        e.load_contentvec(2); e.load_model(z["model"])
    if method == "load_f0":
        e.load_f0()
    else:
        e.load_f0_method(method)
    if streams > 1:
        e.set_streams(streams)
    e.set_noise_seed(1234, 0)
    return e


def _check(got, ref, margin, bound):
    """got (float32, device) against ref (float64) entry by entry: voicing wherever the margin allows, the relative error wherever both are voiced"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    sure = margin >= MARGIN
    assert np.sum(~sure) <= 0.10 * len(ref), "more than 10 %% of the frames within %g of the threshold: %d" % (MARGIN, np.sum(~sure))
    assert np.array_equal(got[sure] > 0, ref[sure] > 0), np.where((got > 0) != (ref > 0))
    v = (got > 0) & (ref > 0)
    err = float(np.max(np.abs(got[v] - ref[v]) / ref[v])) if v.any() else 0.0
    print("voiced %d of %d, under the margin %d, largest relative error %.3e (bound %.3e)" % (v.sum(), len(ref), np.sum(~sure), err, bound))
    assert err <= bound, err


@pytest.fixture(scope="module")
def yin_case():
    """the composite input, its float64 reference, the bound derived from the float32 run, and the device's rvc_pitch result on a fresh engine"""
    x = Y.composite_signal()
    ref, margin = Y.yin(x, FRAME16K)
    f32, _ = Y.yin(x, FRAME16K, np.float32)
    v = (ref > 0) & (f32 > 0) & (margin >= MARGIN)
    base = float(np.max(np.abs(f32[v].astype(np.float64) - ref[v]) / ref[v]))
    bound = max(8.0 * base, 1e-6)
    print("float32 numpy against float64: %.3e -> bound %.3e" % (base, bound))
    e = _engine(zoo("tiny"), full=False)
    got = e.pitch(x, 0, FRAME16K)
    e.close()
    return {"x": x, "ref": ref, "margin": margin, "bound": bound, "got": got}


def test_method_loading(tmp_path):
    from obs_rvc_amd.rvc import RvcInfer
    x = Y.composite_signal()
    e = RvcInfer(str(tmp_path))                      # a data directory without f0/rmvpe.rvcw
    assert e.f0_method == 0
    with pytest.raises(RvcInferError) as ei:
        e.pitch(x, 0, FRAME16K)
    assert ei.value.kind == "F0NotLoaded"
    with pytest.raises(RvcInferError):
        e.load_f0()
    assert e.f0_method == 0
    e.load_f0_method(F0_YIN)
    assert e.f0_method == 2
    with pytest.raises(RvcInferError) as ei:
        e.load_f0_method(3)
    assert ei.value.kind == "NdarrayShapeError" and e.f0_method == 2
    f0 = e.pitch(x, 0, FRAME16K)
    assert f0.shape == (32,) and np.all(np.isfinite(f0)) and np.any(f0 > 0) and f0[0] == 0.0
    e.close()
    z = zoo("tiny")
    a, b = _engine(z, "load_f0", full=False), _engine(z, "rmvpe", full=False)
    assert a.f0_method == b.f0_method == F0_RMVPE
    pa, pb = a.pitch(x, 12, FRAME16K), b.pitch(x, 12, FRAME16K)
    assert pa.shape == (32,) and np.array_equal(pa, pb)
    b.load_f0_method("yin")
    assert b.f0_method == F0_YIN
    with pytest.raises(ValueError):
        b.load_f0_method("harvest")
    a.close(); b.close()


def test_pitch_against_the_reference(yin_case):
    c = yin_case
    assert c["got"].shape == (32,)
    _check(c["got"], c["ref"], c["margin"], c["bound"])
    assert np.sum(c["ref"] > 0) >= 12 and c["ref"][0] == 0.0 and c["got"][0] == 0.0
    # the pitch shift of rvc.rs:121 on top: a power of two, exact
    e = _engine(zoo("tiny"), full=False)
    for shift in (12, -7, -12):
        assert np.array_equal(e.pitch(c["x"], shift, FRAME16K), c["got"] * np.float32(Y.uppower(shift)))
    e.close()


def _cache_ref(chunks, up, scale=1.0):
    """reference pitch cache of one stream after the chunks, and the decision margin of the frame each entry came from (1 where nothing was written)"""
    cache, marg = np.zeros(1024), np.ones(1024)
    for x in chunks:
        f0, m = Y.yin(x, FRAME16K)
        cache, _ = Y.update_cache(cache, f0 * up * scale, SHIFT, CACHE_START, 0, 0)
        marg, _ = Y.update_cache(marg, m, SHIFT, CACHE_START, 0, 0)
    return cache, marg


def test_streams_two_chunks(yin_case):
    z = zoo("tiny")
    sr = int(W.read_blob(z["model"])[0]["sr"])
    shifts = (12, 0, -7)
    xs = [np.stack([voice_signal(g.input_buffer_16k_size, seed=10 * k + s + 1) for s in range(3)]) for k in range(2)]
    xs[1][1, -4960:] = Y.composite_signal()[-4960:]          # the interior stream's second chunk has unvoiced frames too
    e = _engine(z, streams=3)
    for k in range(2):
        y = e.infer_batch(xs[k], FRAME16K, shifts, g.skip_head, R)
        assert y.shape == (3, R * sr // 100) and np.all(np.isfinite(y))
    for s in range(3):
        ref, marg = _cache_ref([xs[0][s], xs[1][s]], Y.uppower(shifts[s]))
        got = e.pitch_cache(s)
        assert np.all(got[:CACHE_START - SHIFT] == 0.0)
        lo = CACHE_START - SHIFT
        _check(got[lo:], ref[lo:], marg[lo:], yin_case["bound"])
    e.close()


def test_plan_identity_between_the_methods(yin_case):
    c = yin_case
    z = zoo("tiny")
    e = _engine(z, "load_f0")
    p1 = e.pitch(c["x"], 0, FRAME16K)
    e.load_f0_method("yin")
    y1 = e.pitch(c["x"], 0, FRAME16K)
    e.enable_taps(True)
    y_tap_run = e.pitch(c["x"], 0, FRAME16K)
    tap = e.tap("f0")
    e.enable_taps(False)
    e.load_f0_method("rmvpe")
    p3 = e.pitch(c["x"], 0, FRAME16K)
    e.load_f0_method("yin")
    y2 = e.pitch(c["x"], 0, FRAME16K)
    assert np.array_equal(p1, p3) and not np.array_equal(p1, y1)
    assert np.array_equal(y1, c["got"]) and np.array_equal(y2, c["got"])
    assert np.array_equal(tap, y_tap_run) and np.array_equal(tap, c["got"])
    # graph replay: the same pitch cache, bit for bit
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    e.infer(x, FRAME16K, 12, g.skip_head, R)
    eager = e.pitch_cache()
    e.reset_state()
    e.set_use_graph(True)
    e.infer(x, FRAME16K, 12, g.skip_head, R)
    assert np.array_equal(e.pitch_cache(), eager) and np.any(eager > 0)
    e.close()


def test_formant_shift_and_native_session(yin_case):
    from obs_rvc_amd.streaming import NativeStreamingSession
    z = zoo("tiny")
    sr = int(W.read_blob(z["model"])[0]["sr"])
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    x[-4960:] = Y.composite_signal()[-4960:]
    e = _engine(z)
    e.set_formant_shift(3.0)
    y = e.infer(x, FRAME16K, 12, g.skip_head, R)
    assert y.shape == (R * sr // 100,) and np.all(np.isfinite(y))
    # the cached f0 is the reference times uppower (exact) times (float)2^(-3/12): one more rounding of the product, 2^-24 relative
    ref, marg = _cache_ref([x], Y.uppower(12), float(np.float32(2.0 ** (-3.0 / 12.0))))
    lo = CACHE_START
    _check(e.pitch_cache()[lo:], ref[lo:], marg[lo:], yin_case["bound"] + 2.0 ** -24)
    e.close()
    e = _engine(z)
    s = NativeStreamingSession(e, 48000, 0.16, 0.07, 2.0, sr, 12, 0.6)
    assert s.sample_frame_16k == FRAME16K
    rng = np.random.default_rng(5)
    t = np.arange(2 * s.sample_frame_size) / 48000.0
    audio = (0.2 * sum(np.sin(2 * np.pi * 150.0 * k * t) / k for k in range(1, 5)) + 1e-3 * rng.standard_normal(len(t))).astype(np.float32)
    for k in range(2):
        out = s.process_one_frame(audio[k * s.sample_frame_size:(k + 1) * s.sample_frame_size])          # (raises unless RVC_OK)
        assert out.shape == (s.sample_frame_size,) and np.all(np.isfinite(out))
    assert np.any(e.pitch_cache() > 0)
    del s
    e.close()


@pytest.mark.parametrize("frame16k", [5120, 5120 * 13], ids=["Tm64", "Tm448"])
def test_pitch_over_a_whole_converter_window(frame16k):
    """n == frame, as every window of the file converter: the f0 window starts at sample 0 of the buffer, so the first and last frames reflect about
    the buffer's own first and last samples (a DC step sits on each).  Tm = 64 (k = 2) and the default window's Tm = 448, one workgroup per frame.
    The bound is this input's own: 8 x the float32-numpy deviation, floor 1e-6 (tests/test_yin_ref.py shows the reference side)"""
    x = Y.whole_window_signal(frame16k)
    Tm = frame16k // 160 + 32
    assert len(x) == Y.f0_frame(frame16k) == 160 * (Tm - 1)
    ref, margin = Y.yin(x, frame16k)
    f32, _ = Y.yin(x, frame16k, np.float32)
    v = (ref > 0) & (f32 > 0) & (margin >= MARGIN)
    base = float(np.max(np.abs(f32[v].astype(np.float64) - ref[v]) / ref[v]))
    bound = max(8.0 * base, 1e-6)
    print("Tm %d: float32 numpy against float64 %.3e -> bound %.3e" % (Tm, base, bound))
    e = _engine(zoo("tiny"), full=False)
    got = e.pitch(x, 0, frame16k)
    e.close()
    assert got.shape == (Tm,) and np.any(ref[-4:] > 0)
    _check(got, ref, margin, bound)
    for t in (0, 1, 2, 3, Tm - 4, Tm - 3, Tm - 2, Tm - 1):
        print("  frame %3d: gpu %.6f, float64 %.6f, margin %.2e" % (t, got[t], ref[t], margin[t]))
