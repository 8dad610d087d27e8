"""rvc_analyze_f0 (obs_rvc_amd/csrc/f0_analyze.hip.h) on the tiny zoo: the f0 of the composition tests' file (37 370 samples at 16 kHz,
Nf = 234) with k = 2, C = 3, X = 2 (W = 5 windows of Tm = 64 rows, hop 54) against the composition of public calls -- numpy gather, rvc_pitch per window with
pitch_shift 0, the hop export --, one stream against three, under non-neutral pitch controls, against the f0 a conversion reports, a hybrid, the statuses.

Bounds.  YIN runs one kernel at every stream count: one stream against the composition and three streams against one are held bit for bit.  RMVPE's analysis
against rvc_convert_f0 of a plain conversion with neutral controls: at three streams the pitch-only plan and the infer plan queue the same f0 launches (the
planner's rules alone decide below five streams, and RMVPE's launch list depends on the engine's partition and the stream count, not on the plan's mode), so
this too is held bit for bit; the relative RMS is printed beside it (DESIGN.md section 28 records both cases)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import convert_ref as R
import f0_override_ref as O
from common import voice_signal, zoo
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError
from test_gpu_convert import CTX, K, XF, ZC, engine, guard
from test_gpu_convert_file import N_IN, RATE_IN

pytestmark = pytest.mark.gpu

_FP = C.POINTER(C.c_float)
NF = 234


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def bare(method="yin", streams=1):
    e = RvcInfer(zoo("tiny")["data"])
    if method:
        e.load_f0_method(method)
    if streams > 1:
        e.set_streams(streams)
    return e


@pytest.fixture(scope="module")
def x16():
    e = bare(None)
    x = guard(e.resample, voice_signal(N_IN, seed=11, sr=RATE_IN), RATE_IN, 16000)
    e.close()
    assert len(x) == 37370
    return x


@pytest.fixture(scope="module")
def yin_one(x16):
    """the analysis at one stream, shared by the tests that compare against it"""
    e = bare("yin")
    f0 = guard(e.analyze_f0, x16, K, CTX, XF, highpass=False)
    e.close()
    assert f0.shape == (NF,) and f0.dtype == np.float32
    return f0


def analyze(e, x, **kw):
    return guard(e.analyze_f0, x, K, CTX, XF, **kw)


def test_one_stream_is_the_composition(x16, yin_one):
    geo, og = RvcInfer.convert_geometry(len(x16), 100 * ZC, K, CTX, XF), O.geometry(K, CTX, XF, NF)
    assert geo["windows"] == og["W"] == 5 and geo["hop"] == og["H"] == 54 and geo["n"] == 160 * og["F"]
    e = bare("yin")
    win = R.gather_windows(np.asarray(x16, np.float32), geo)
    rows = np.stack([guard(e.pitch, w, 0, geo["sample_frame_16k_size"]) for w in win])
    assert rows.shape == (5, og["Tm"])
    want, hits = O.export(rows, og)
    assert np.all(hits == 1)
    assert same_bits(yin_one, want) and np.count_nonzero(yin_one > 0) > 20
    # the high-pass in front is rvc_highpass
    hp = analyze(e, x16, highpass=True)
    assert same_bits(hp, analyze(e, guard(e.highpass, x16), highpass=False)) and not same_bits(hp, yin_one)
    # ... and the geometry's defaults are the converter's (k = 14, C = 48, X = 5: one window here)
    d = guard(e.analyze_f0, x16, highpass=False)
    assert d.shape == (NF,) and same_bits(d, guard(e.analyze_f0, x16, 14, 48, 5, highpass=False))
    e.close()


def test_three_streams_are_one_stream(x16, yin_one):
    e = bare("yin", 3)          # two batches, the second with one zero-padded stream
    b0 = e.plan_cache_info()["builds"]
    got = analyze(e, x16, highpass=False)
    assert e.plan_cache_info()["builds"] == b0 + 1          # one pitch-only plan of three streams, through the plan cache
    voiced_same = np.array_equal(got > 0, yin_one > 0)
    v = (got > 0) & (yin_one > 0)
    rel = float(np.max(np.abs(got[v].astype(np.float64) - yin_one[v]) / yin_one[v])) if v.any() else 0.0
    print("YIN analysis, 3 streams against 1: identical voicing %s, largest relative difference %.3e, equal bits %s" % (voiced_same, rel, same_bits(got, yin_one)))
    assert same_bits(got, yin_one)
    assert same_bits(analyze(e, x16, highpass=False), got) and e.plan_cache_info()["builds"] == b0 + 1
    e.close()


def test_the_streams_settings_do_not_apply_and_stay(x16, yin_one):
    e = bare("yin")
    geo = RvcInfer.convert_geometry(len(x16), 100 * ZC, K, CTX, XF)
    w1 = R.gather_windows(np.asarray(x16, np.float32), geo)[1]
    neutral = guard(e.pitch, w1, 0, geo["sample_frame_16k_size"])
    e.set_pitch_semitones(3.0); e.set_f0_median(2); e.set_f0_snap("C major", 1.0); e.set_f0_range(70.0, 600.0)
    cond = guard(e.pitch, w1, 0, geo["sample_frame_16k_size"])
    assert not same_bits(cond, neutral)
    assert same_bits(analyze(e, x16, highpass=False), yin_one)                   # the tracker's own rows
    assert same_bits(guard(e.pitch, w1, 0, geo["sample_frame_16k_size"]), cond)    # ... and the settings are what they were
    e.close()
    e = bare("yin", 3)
    e.set_pitch_semitones(3.0); e.set_f0_median(2, stream=1); e.set_f0_snap("C major", 1.0, stream=2)
    assert same_bits(analyze(e, x16, highpass=False), yin_one)
    e.close()


def test_rmvpe_against_the_f0_of_a_conversion(x16):
    e = engine(3, "rmvpe")
    guard(e.convert, x16, k=K, context=CTX, crossfade=XF, pitch_shift=0, highpass=False)
    conv = e.convert_f0()
    got = analyze(e, x16, highpass=False)
    assert got.shape == conv.shape == (NF,)
    num, den = float(np.sqrt(np.mean((got.astype(np.float64) - conv) ** 2))), float(np.sqrt(np.mean(conv.astype(np.float64) ** 2)))
    print("RMVPE analysis against rvc_convert_f0: relative RMS %.3e, equal bits %s, voiced %d / %d" % (num / den, same_bits(got, conv), (got > 0).sum(), (conv > 0).sum()))
    assert den > 0 and num / den <= 1e-4 and same_bits(got, conv)
    # a conversion behind the analysis is the conversion in front of it: the analysis leaves the reset state
    y0, _ = guard(e.convert, x16, k=K, context=CTX, crossfade=XF, pitch_shift=0, highpass=False)
    analyze(e, x16, highpass=False)
    y1, _ = guard(e.convert, x16, k=K, context=CTX, crossfade=XF, pitch_shift=0, highpass=False)
    assert same_bits(y0, y1) and same_bits(e.convert_f0(), conv)
    e.close()


def test_a_hybrid_runs(x16, yin_one):
    e = bare("hybrid[yin+pm]", 2)
    got = analyze(e, x16, highpass=False)
    assert got.shape == (NF,) and np.all(np.isfinite(got)) and np.all(got >= 0) and np.count_nonzero(got) > 20
    e.close()


def test_statuses(x16):
    e = bare(None)
    out, n = np.zeros(NF, np.float32), C.c_size_t(77)
    call = lambda e, x, k, c, xf, cap: e._L.rvc_analyze_f0(e._h, x.ctypes.data_as(_FP), len(x), k, c, xf, 0, out.ctypes.data_as(_FP), cap, C.byref(n))
    assert call(e, x16, K, CTX, XF, NF) == 3                           # RVC_F0_NOT_LOADED, before any argument is looked at
    with pytest.raises(RvcInferError) as ei:
        e.analyze_f0(x16)
    assert ei.value.kind == "F0NotLoaded"
    e.load_f0_method("yin")                                            # no voice model, no ContentVec: not needed
    assert call(e, x16[:0], K, CTX, XF, NF) == 5 and b"empty" in e._L.rvc_last_error_message(e._h)
    for k, c, xf in ((1, CTX, XF), (33, CTX, XF), (K, 2, XF), (K, 30, XF)):
        assert call(e, x16, k, c, xf, NF) == 5, (k, c, xf)
    n.value = 77
    assert call(e, x16, K, CTX, XF, NF - 1) == 5 and n.value == NF     # cap short: the size is still written
    assert call(e, x16, K, CTX, XF, NF) == 0 and n.value == NF and np.count_nonzero(out) > 20
    e.close()
