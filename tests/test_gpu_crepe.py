"""The CREPE f0 method (rvc_load_f0_method, crepe.hip.h + the implicit-GEMM planner + the pitch tail) against the float64 restatement
of tests/crepe_ref.py: every stage by its tap, the decoder alone through rvc_debug_crepe_decode, and the public calls.  The smallest geometry:
sample_frame_16k_size = 2560, an f0 window of 4960 samples, 32 frames.

Bounds are not invented here.  A stage's bound is 8 x the largest deviation of the same definition run in float32 numpy from float64 on the same input --
what single precision costs -- with a floor of 1e-6 x the tap's rms; every case prints base, bound and the device's error before it asserts.  A decoded
path is judged by its float64 score against the optimum's, allowed 8 x the shortfall of the float32 reference path with a floor of 1e-6 (relative): at a
near-tie two paths may differ and both be right.  Voicing must agree on every frame whose float64 margin |pd - 0.1| is at least 1e-4.

The seeded weights (weights.make_crepe) are scaled so that posteriors are not saturated: on the composite input the float64 reference's cr.prob spans
0.0015 .. 0.948 (tiny) and 0.0006 .. 0.645 (micro); the stage test prints the device's range."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import crepe_ref as R
import yin_ref as Y
from common import BASELINE_160MS as g, voice_signal, zoo
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc_common import F0_CREPE, F0_CREPE_TINY, RvcInferError

pytestmark = pytest.mark.gpu

FRAME16K = g.sample_frame_16k          # 2560
RL = g.model_return_length
MARGIN = 1e-4
SHIFT, CACHE_START = FRAME16K // 160, 1024 + 4 - 32          # rvc.rs:168,172 at 32 frames
STAGES = ("frames", "p1", "p2", "p3", "p4", "p5", "p6", "prob", "f0")
assert FRAME16K == 2560 and Y.f0_frame(FRAME16K) == 4960


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """the tiny zoo with crepe-tiny / crepe-full next to rmvpe, a directory whose crepe-tiny is the micro preset, and the presets' tensors"""
    z = zoo("tiny")
    W.write_crepe(z["data"], "tiny"); W.write_crepe(z["data"], "full")
    micro = str(tmp_path_factory.mktemp("crepe_micro"))
    W.write_crepe(micro, "micro", as_preset="tiny")
    return {"zoo": z, "micro": micro, "tiny_t": W.make_crepe("tiny")[1], "micro_t": W.make_crepe("micro")[1]}


def _engine(data_dir, method="crepe-tiny", streams=1, model=None):
    from obs_rvc_amd.rvc import RvcInfer
    e = RvcInfer(data_dir)
    if model:
        e.load_contentvec(2); e.load_model(model)
    e.load_f0_method(method)
    if streams > 1:
        e.set_streams(streams)
    e.set_noise_seed(1234, 0)
    return e


def _ref_pair(t, x, decoder="viterbi"):
    return R.crepe(t, x, FRAME16K, decoder), R.crepe(t, x, FRAME16K, decoder, np.float32)


def _shape_tap(name, a, ref):
    """a tap as the reference shapes the stage: p6 comes in the classifier's layout [time * channels + channel][frame]"""
    if name == "p6":
        n, c, l = ref.shape
        return a.reshape(l, c, n).transpose(2, 1, 0)
    return a.reshape(ref.shape)


def _check_stages(e, r64, r32, stream=0, what=""):
    for name in STAGES:
        ref, f32 = np.asarray(r64[name], np.float64), np.asarray(r32[name], np.float64)
        got = _shape_tap(name, e.tap("cr." + name, stream).astype(np.float64), ref)
        rms = float(np.sqrt(np.mean(ref ** 2)))
        base = float(np.max(np.abs(f32 - ref)))
        bound = max(8.0 * base, 1e-6 * rms)
        err = float(np.max(np.abs(got - ref)))
        extra = "  device range %.4g .. %.4g" % (got.min(), got.max()) if name == "prob" else ""
        print("%s cr.%s: rms %.3e  float32 base %.3e  bound %.3e  device error %.3e%s" % (what, name, rms, base, bound, err, extra))
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("preset", ["tiny", "micro"])
def test_stages_against_float64(data, preset):
    x = Y.composite_signal()
    e = _engine(data["zoo"]["data"] if preset == "tiny" else data["micro"])
    e.enable_taps(True)
    f0 = e.pitch(x, 0, FRAME16K)
    assert f0.shape == (32,) and np.all(np.isfinite(f0))
    r64, r32 = _ref_pair(data[preset + "_t"], x)
    assert np.array_equal(r64["bins"], r32["bins"])
    _check_stages(e, r64, r32, what=preset)
    e.close()


@pytest.mark.parametrize("preset", ["tiny", "micro"])
def test_stages_over_a_whole_converter_window(data, preset):
    """n == frame, as every window of the file converter: the f0 window starts at sample 0 of the buffer, so frames 0..3 and 60..63 are zero-extended
    past the buffer's own ends (a DC step sits on each).  64 frames (k = 2); the bounds are _check_stages' own, from this input's float32 run"""
    frame16k = 5120
    x = Y.whole_window_signal(frame16k)
    assert len(x) == Y.f0_frame(frame16k)
    e = _engine(data["zoo"]["data"] if preset == "tiny" else data["micro"])
    e.enable_taps(True)
    f0 = e.pitch(x, 0, frame16k)
    assert f0.shape == (64,) and np.all(np.isfinite(f0))
    t = data[preset + "_t"]
    r64, r32 = R.crepe(t, x, frame16k, "viterbi"), R.crepe(t, x, frame16k, "viterbi", np.float32)
    assert np.array_equal(r64["bins"], r32["bins"])
    _check_stages(e, r64, r32, what="whole window, " + preset)
    v = (r64["f0"] > 0) & (r32["f0"] > 0)
    base = float(np.max(np.abs(r32["f0"][v].astype(np.float64) - r64["f0"][v]) / r64["f0"][v])) if v.any() else 0.0
    _check_f0(f0, r64["f0"], r64["margin"], max(8.0 * base, 1e-6))
    assert np.any(r64["f0"][:4] > 0) or np.any(r64["f0"][-4:] > 0)
    e.close()


def test_stages_three_streams(data):
    z = data["zoo"]
    xs = np.stack([voice_signal(g.input_buffer_16k_size, seed=s + 1) for s in range(3)])
    xs[1, -4960:] = Y.composite_signal()[-4960:]
    e = _engine(z["data"], streams=3, model=z["model"])
    e.enable_taps(True)
    y = e.infer_batch(xs, FRAME16K, (0, 0, 0), g.skip_head, RL)
    assert np.all(np.isfinite(y))
    for s in (0, 1):
        r64, r32 = _ref_pair(data["tiny_t"], xs[s])
        _check_stages(e, r64, r32, stream=s, what="stream %d" % s)
    e.close()


def _torch_prob(t, F):
    """the network in torch float64 (F.conv1d / batch_norm / max_pool1d), as tests/test_crepe_ref.py states it"""
    from test_crepe_ref import torch_network
    return torch_network(t, F)["prob"]


def test_full_preset_posteriors(data):
    """full capacity, 1 stream, 32 frames: cr.prob against the float64 torch restatement (under a second for all 32 frames on 16 CPU threads, so nothing is cut);
    the reference's posteriors span 0.0002 .. 0.397 here"""
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    x = Y.composite_signal()
    t = W.make_crepe("full")[1]
    F = R.frames(x, FRAME16K)
    ref = _torch_prob(t, F)
    f32 = R.network(t, F, np.float32)["prob"].astype(np.float64)
    e = _engine(data["zoo"]["data"], "crepe")
    assert e.f0_method == F0_CREPE
    e.enable_taps(True)
    e.pitch(x, 0, FRAME16K)
    got = e.tap("cr.prob").astype(np.float64).reshape(32, 360)
    e.close()
    rms, base = float(np.sqrt(np.mean(ref ** 2))), float(np.max(np.abs(f32 - ref)))
    bound, err = max(8.0 * base, 1e-6 * rms), float(np.max(np.abs(got - ref)))
    print("full cr.prob: rms %.3e  float32 base %.3e  bound %.3e  device error %.3e  device range %.4g .. %.4g" % (rms, base, bound, err, got.min(), got.max()))
    assert err <= bound


# ------------------------------------------------------------------------------------------------ the decoder alone
def _decode(e, prob, decoder):
    prob = np.ascontiguousarray(prob, np.float32)
    B, Tm, _ = prob.shape
    f0, pd, bins = np.empty((B, Tm), np.float32), np.empty((B, Tm), np.float32), np.empty((B, Tm), np.int32)
    fp = C.POINTER(C.c_float)
    rc = e._L.rvc_debug_crepe_decode(e._h, prob.ctypes.data_as(fp), B, Tm, int(decoder), f0.ctypes.data_as(fp), bins.ctypes.data, pd.ctypes.data_as(fp))
    assert rc == 0, rc
    return f0, bins, pd


_ridge, _smooth = R.ridge_case, R.smooth_case


@pytest.fixture(scope="module")
def dec_engine(data):
    e = _engine(data["zoo"]["data"], "yin")          # the hook needs an engine, no weights
    yield e
    e.close()


@pytest.mark.parametrize("B,Tm", [(1, 32), (3, 32), (1, 1024), (3, 1024)])
def test_decoder_ridge_and_decoys(dec_engine, B, Tm):
    cases = [_ridge(Tm, 10 * Tm + b) for b in range(B)]
    prob = np.stack([c[0] for c in cases])
    _, vb, _ = _decode(dec_engine, prob, 0)
    _, ab, _ = _decode(dec_engine, prob, 1)
    for b, (p, centre, decoy) in enumerate(cases):
        r64, r32 = R.decode(p, "viterbi"), R.decode(p, "viterbi", np.float32)
        assert np.array_equal(r64["bins"], r32["bins"])          # the margins of the construction: float32 and float64 agree bin for bin
        assert np.max(np.abs(r64["bins"] - centre)) <= 2 and np.max(np.abs(np.diff(r64["bins"]))) <= 11
        assert np.array_equal(vb[b], r64["bins"]), np.where(vb[b] != r64["bins"])
        assert all(ab[b, t] == d for t, d in decoy.items()) and all(abs(int(vb[b, t]) - d) > 40 for t, d in decoy.items())
        assert np.array_equal(ab[b], R.decode(p, "argmax")["bins"])


@pytest.mark.parametrize("B,Tm", [(1, 32), (3, 32), (1, 1024), (3, 1024)])
def test_decoder_random_smooth_posteriors(dec_engine, B, Tm):
    prob = np.stack([_smooth(Tm, 7 * Tm + b) for b in range(B)])
    _, vb, _ = _decode(dec_engine, prob, 0)
    lt = R.log_transition()
    for b in range(B):
        lo = R.log_observation(prob[b])
        opt = R.path_score(lo, lt, R.decode(prob[b], "viterbi")["bins"])
        base = (opt - R.path_score(lo, lt, R.decode(prob[b], "viterbi", np.float32)["bins"])) / abs(opt)
        short = (opt - R.path_score(lo, lt, vb[b])) / abs(opt)
        bound = max(8.0 * base, 1e-6)
        print("B %d Tm %d stream %d: optimum %.6f  float32 shortfall %.3e  bound %.3e  device shortfall %.3e" % (B, Tm, b, opt, base, bound, short))
        assert np.isfinite(short) and -1e-12 <= short <= bound


@pytest.mark.parametrize("Tm", [32, 1024])
def test_decoder_ties_silence_and_out_of_range(dec_engine, Tm):
    flat = np.full((Tm, 360), 0.5, np.float32)                                   # every column equal: the lowest decoded bin
    two = np.full((Tm, 360), 0.1, np.float32); two[:, [100, 200]] = 0.9          # two equal columns: the lower one
    edge = np.zeros((Tm, 360), np.float32); edge[:, :R.LO] = 0.9; edge[:, R.HI:] = 0.9          # all the mass outside the decoded range
    silent = np.zeros((Tm, 360), np.float32)
    prob = np.stack([flat, two, edge, silent])
    for dec in (0, 1):
        f0, bins, pd = _decode(dec_engine, prob, dec)
        assert np.all(np.isfinite(f0)) and np.all(np.isfinite(pd))
        assert np.all(bins[0] == R.LO) and np.all(bins[1] == 100)
        assert np.all((bins >= R.LO) & (bins < R.HI))
        assert np.all(f0[2] == 0.0) and np.all(f0[3] == 0.0) and np.all(pd[2] == 0.0)
        assert np.all(f0[1] == np.float32(R.F0_OF_BIN[100])) and np.all(f0[0] == np.float32(R.F0_OF_BIN[R.LO]))


@pytest.mark.parametrize("Tm", [32, 1024])
def test_decoder_filters_and_threshold(dec_engine, Tm):
    # a ridge whose height crosses the threshold in single frames, pairs and at both ends: the median of three removes the single ones, the ends see two entries
    p, centre, _ = _ridge(Tm, 99)
    p = np.minimum(p, 0.8)                                                       # no decoys here
    h = np.full(Tm, 0.8); h[[0, 5, 9, 10, 15, 16, 17, Tm - 1]] = 0.04; h[[20, 22]] = 0.0796; h[21] = 0.6          # (the floor of 0.02 comes on top: just under 0.1)
    p = (0.02 + (p - 0.02) * (h[:, None] / 0.78)).astype(np.float32)
    f0, bins, pd = _decode(dec_engine, p[None], 0)
    r64, r32 = R.decode(p, "viterbi"), R.decode(p, "viterbi", np.float32)
    assert np.array_equal(bins[0], r64["bins"]) and np.array_equal(pd[0], p[np.arange(Tm), bins[0]])
    sure = r64["margin"] >= MARGIN
    assert np.sum(~sure) <= 0.10 * Tm
    assert np.array_equal(f0[0][sure] > 0, r64["f0"][sure] > 0)
    assert r64["f0"][5] > 0 and r64["f0"][9] == 0 and r64["f0"][16] == 0 and r64["f0"][21] == 0 and r64["f0"][1] > 0 and r64["f0"][Tm - 2] > 0          # what the filters are for
    v = (f0[0] > 0) & (r64["f0"] > 0)
    base = float(np.max(np.abs(r32["f0"][v].astype(np.float64) - r64["f0"][v]) / r64["f0"][v]))
    err = float(np.max(np.abs(f0[0][v].astype(np.float64) - r64["f0"][v]) / r64["f0"][v]))
    print("Tm %d: voiced %d, float32 base %.3e, device error %.3e" % (Tm, v.sum(), base, err))
    assert err <= max(8.0 * base, 1e-6)
    # the first and the last frame: the mean of the two entries that exist
    F = R.F0_OF_BIN
    if f0[0][Tm - 1] > 0:
        assert abs(f0[0][Tm - 1] - 0.5 * (F[bins[0][Tm - 1]] + F[bins[0][Tm - 2]])) <= 1e-6 * f0[0][Tm - 1]
    assert (f0[0][0] > 0) == (0.5 * (float(pd[0][0]) + float(pd[0][1])) >= 0.1)


# ------------------------------------------------------------------------------------------------ the public calls
def _check_f0(got, ref, margin, bound):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    sure = margin >= MARGIN
    assert np.sum(~sure) <= 0.10 * len(ref), "more than 10 %% of the frames within %g of the threshold: %d" % (MARGIN, np.sum(~sure))
    assert np.array_equal(got[sure] > 0, ref[sure] > 0), np.where((got > 0) != (ref > 0))
    v = (got > 0) & (ref > 0)
    err = float(np.max(np.abs(got[v] - ref[v]) / ref[v])) if v.any() else 0.0
    print("voiced %d of %d, under the margin %d, largest relative error %.3e (bound %.3e)" % (v.sum(), len(ref), np.sum(~sure), err, bound))
    assert err <= bound, err


def _f0_bound(t, x):
    r64, r32 = _ref_pair(t, x)
    v = (r64["f0"] > 0) & (r32["f0"] > 0)
    base = float(np.max(np.abs(r32["f0"][v].astype(np.float64) - r64["f0"][v]) / r64["f0"][v])) if v.any() else 0.0
    return r64, max(8.0 * base, 1e-6)


def test_pitch_against_the_reference(data):
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    x[-4960:] = Y.composite_signal()[-4960:]
    r64, bound = _f0_bound(data["tiny_t"], x)
    e = _engine(data["zoo"]["data"])
    assert e.f0_method == F0_CREPE_TINY and e.crepe_decoder == 0
    got = e.pitch(x, 0, FRAME16K)
    assert got.shape == (32,)
    _check_f0(got, r64["f0"], r64["margin"], bound)
    for shift in (12, -7, -12):          # the pitch shift of rvc.rs:121 on top: a power of two, exact
        assert np.array_equal(e.pitch(x, shift, FRAME16K), got * np.float32(Y.uppower(shift)))
    e.set_crepe_decoder("argmax")
    a = e.pitch(x, 0, FRAME16K)
    ra = R.crepe(data["tiny_t"], x, FRAME16K, "argmax")
    _check_f0(a, ra["f0"], ra["margin"], bound)
    assert not np.array_equal(a, got)
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
        cache, marg, bound = np.zeros(1024), np.ones(1024), 1e-6
        for k in range(2):
            r64, b = _f0_bound(data["tiny_t"], xs[k][s])
            bound = max(bound, b)
            cache, _ = Y.update_cache(cache, r64["f0"] * Y.uppower(shifts[s]), SHIFT, CACHE_START, 0, 0)
            marg, _ = Y.update_cache(marg, r64["margin"], SHIFT, CACHE_START, 0, 0)
        got = e.pitch_cache(s)
        lo = CACHE_START - SHIFT
        assert np.all(got[:lo] == 0.0)
        _check_f0(got[lo:], cache[lo:], marg[lo:], bound)
    e.close()


def test_plan_identity_and_graph_replay(data):
    z = data["zoo"]
    x = Y.composite_signal()
    e = _engine(z["data"], "rmvpe", model=z["model"])
    builds = lambda: e.plan_cache_info()["builds"]
    out, n = {}, builds()
    for step, (method, dec) in enumerate([("rmvpe", None), ("crepe", "viterbi"), ("crepe-tiny", "viterbi"), ("crepe-tiny", "argmax")]):
        if step:
            e.load_f0_method(method); e.set_crepe_decoder(dec)
        out[(method, dec)] = e.pitch(x, 0, FRAME16K)
        assert builds() == n + 1, (method, dec)          # each its own plan
        n = builds()
    vals = list(out.values())
    assert all(not np.array_equal(vals[i], vals[j]) for i in range(4) for j in range(i))
    for method, dec in [("crepe-tiny", "viterbi"), ("crepe", "viterbi"), ("crepe-tiny", "argmax"), ("crepe", "argmax")]:
        e.load_f0_method(method); e.set_crepe_decoder(dec)
        got = e.pitch(x, 0, FRAME16K)
        if (method, dec) in out:
            assert builds() == n and np.array_equal(got, out[(method, dec)])          # going back hits the cache
        else:
            assert builds() == n + 1
            n = builds()
    with pytest.raises(ValueError):
        e.set_crepe_decoder("beam")
    with pytest.raises(RvcInferError) as ei:
        e.set_crepe_decoder(2)
    assert ei.value.kind == "NdarrayShapeError" and e.crepe_decoder == 1
    # graph replay: the same pitch cache, bit for bit
    e.load_f0_method("crepe-tiny"); e.set_crepe_decoder("viterbi")
    xv = voice_signal(g.input_buffer_16k_size, seed=3)
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
    for name, call in (("rmvpe", e.load_f0), ("crepe", lambda: e.load_f0_method("crepe")), ("crepe-tiny", lambda: e.load_f0_method(F0_CREPE_TINY))):
        with pytest.raises(RvcInferError) as ei:
            call()
        statuses[name] = ei.value.kind
        assert e.f0_method == 0
    assert statuses["crepe"] == statuses["crepe-tiny"] == statuses["rmvpe"] == "Backend"
    for bad in (3, 6, -1):
        with pytest.raises(RvcInferError) as ei:
            e.load_f0_method(bad)
        assert ei.value.kind == "NdarrayShapeError" and all(w in str(ei.value) for w in ("RMVPE", "YIN", "CREPE", "CREPE_TINY"))
    with pytest.raises(ValueError):
        e.load_f0_method("harvest")
    W.write_crepe(str(tmp_path), "micro", as_preset="tiny")
    e.load_f0_method("crepe-tiny")
    f0 = e.pitch(Y.composite_signal(), 0, FRAME16K)
    assert e.f0_method == F0_CREPE_TINY and f0.shape == (32,) and np.all(np.isfinite(f0))
    e.close()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_session_chunk_is_the_composition(data):
    """one chunk through the native session against the same chunk through StreamingSession, which is the composition of public calls (the converters,
    rvc_infer, envelope mixing, rvc_sola_step) on a second engine: the posteriors, CREPE's raw f0, the tail's f0, the pitch cache, the ContentVec output,
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
    for name in ("cr.prob", "cr.f0", "f0", "cv.out"):
        assert _same_bits(e1.tap(name), e2.tap(name)), name
    assert _same_bits(e1.pitch_cache(), e2.pitch_cache()) and np.any(e1.pitch_cache() > 0)
    print("session chunk: frames differ by %.3e" % float(np.abs(fn - fp).max()))
    assert nat.last_sola_offset == pys.last_sola_offset and _same_bits(fn, fp)
    del nat
    e1.close(); e2.close()


@pytest.mark.parametrize("decoder", ["viterbi", "argmax"])
def test_convert_of_three_windows_is_the_composition(data, decoder):
    """rvc_convert with CREPE against tests/test_gpu_convert.py's composition of public calls (numpy window gather, reset_state, infer_batch per batch,
    sola_stitch): audio and offsets bit for bit"""
    import test_gpu_convert as TC
    x = voice_signal(160 * 150, seed=11)
    assert TC.RvcInfer.convert_geometry(len(x), 100 * TC.ZC, TC.K, TC.CTX, TC.XF)["windows"] == 3
    e = TC.engine(3, "crepe-tiny")
    e.set_crepe_decoder(decoder)
    ref, ref_off = TC.composition(e, x)
    got, rate = TC.guard(e.convert, x, k=TC.K, context=TC.CTX, crossfade=TC.XF, pitch_shift=TC.SHIFT, highpass=False)
    info = e.convert_info()
    assert rate == 100 * TC.ZC and info["windows"] == 3 and info["batches"] == 1
    assert info["offsets"].tolist() == ref_off.tolist() and TC.same_bits(got, ref) and np.all(np.isfinite(got))
    assert e.f0_method == F0_CREPE_TINY and e.crepe_decoder == (0 if decoder == "viterbi" else 1) and np.any(e.pitch_cache(1) > 0)
    e.close()
