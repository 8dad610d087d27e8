"""The file converter (obs_rvc_amd/csrc/convert.hip.h, stitch.hip.h, highpass.hip.h) on the tiny zoo (sr = 4800, zc = 48): the high-pass
against fp64, the stitch against the chained public rvc_sola_step bit for bit and against fp64, rvc_convert against the composition of public calls bit
for bit (numpy window gather, reset_state, infer_batch per batch, sola_stitch), its independence of what the engine ran before, one stream, the statuses.
A HIP error ends the session: nothing more is started on the device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import convert_ref as R
from common import BASELINE_160MS as g160, voice_signal, zoo
from obs_rvc_amd import _native
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError

pytestmark = pytest.mark.gpu

ZC = 48
K, CTX, XF = 2, 3, 2                       # F = 63, n = 10 080, H = 54, return_length = 57
N = 160 * 233 + 77                         # Nf = 234, W = 5
SHIFT = 12                                 # the integer pitch_shift: one octave
_FP = C.POINTER(C.c_float)


def guard(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except RvcInferError as x:
        if "hip" in str(x).lower():
            pytest.exit("a HIP call failed (%s): nothing more is started on this device" % x, returncode=3)
        raise


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def engine(streams=3, f0="rmvpe"):
    z = zoo("tiny", 2)
    e = RvcInfer(z["data"])
    e.load_contentvec(2); e.load_model(z["model"]); e.load_f0_method(f0)
    e.set_streams(streams); e.set_noise_seed(1234, 0)
    return e


def recording():
    return voice_signal(N, seed=11)


def composition(e, x):
    """what rvc_convert computes, from public calls: numpy gather of the windows, reset_state, infer_batch per batch (a short last batch padded with all-zero
    windows whose outputs are dropped), sola_stitch, cut to Nf zc samples -> (audio, offsets)"""
    geo = RvcInfer.convert_geometry(len(x), 100 * ZC, K, CTX, XF)
    win = R.gather_windows(np.asarray(x, np.float32), geo)
    W, S = geo["windows"], e.n_streams
    pad = np.concatenate([win, np.zeros(((-W) % S, geo["n"]), np.float32)])
    e.reset_state()
    ys = [guard(e.infer_batch, pad[i: i + S], geo["sample_frame_16k_size"], SHIFT, geo["skip_head"], geo["return_length"]) for i in range(0, len(pad), S)]
    y = np.concatenate(ys)[:W]
    assert y.shape == (W, geo["return_length"] * ZC)
    audio, off = guard(e.sola_stitch, y, XF * ZC, ZC, geo["hop"] * ZC)
    return audio[: geo["output_samples"]], off


# ---------------------------------------------------------------- 1. high-pass against fp64
def hp_signal(n):
    t = np.arange(n) / 16000.0
    x = 0.3 + 0.2 * np.sin(2 * np.pi * 30.0 * t) + 0.2 * np.sin(2 * np.pi * 200.0 * t)
    if n > 7:
        x[7] += 1.0
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def plain_engine():
    e = RvcInfer(zoo("tiny", 2)["data"])
    yield e
    e.close()


@pytest.mark.parametrize("n", [5000, 1, 100])
def test_highpass_against_fp64(plain_engine, n):
    x = hp_signal(n)
    ref = R.highpass(x)
    # the bound: 8 x the largest error of the same recipe evaluated in float32 numpy, floor 1e-6 absolute
    err32 = float(np.max(np.abs(R.highpass_f32(x).astype(np.float64) - ref)))
    got = guard(plain_engine.highpass, x)
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print("highpass n = %d: kernel error %.3e, float32 numpy error %.3e" % (n, err, err32))
    assert got.shape == (n,) and got.dtype == np.float32
    assert err <= max(8.0 * err32, 1e-6), (err, err32)
    if n == 5000:      # DC and 30 Hz are gone in the middle, 200 Hz is not
        assert abs(float(np.mean(got[1500:3500]))) < 0.02 and float(np.std(got[1500:3500])) > 0.1


# ---------------------------------------------------------------- 2. stitch against the public step and against fp64
def stitch_windows(sola_len, search, frame, shift):
    """4 windows: random; a window that repeats its predecessor's tail at lag `shift`; all zeros (every lag ties); random"""
    r = np.random.default_rng(2024)
    wl = search + frame + sola_len
    w = r.uniform(-0.5, 0.5, (4, wl)).astype(np.float32)
    # window 0 meets the zero tail: offset = search, tail = its samples [search + frame, + sola_len)
    w[1, shift: shift + sola_len] = w[0, search + frame: search + frame + sola_len]
    w[2] = 0.0
    return w


@pytest.mark.parametrize("sola_len,search,frame", [(96, 48, 240), (48, 48, 48)])
def test_stitch_is_the_chained_step(plain_engine, sola_len, search, frame):
    e, shift = plain_engine, 17
    w = stitch_windows(sola_len, search, frame, shift)
    assert w.shape[1] == (384 if frame == 240 else 144)
    audio, off = guard(e.sola_stitch, w, sola_len, search, frame)
    tail = np.zeros(sola_len, np.float32)
    frames, offs = [], []
    for i in range(len(w)):
        o, fr, tail = guard(e.sola_step, w[i], tail, search, frame)
        frames.append(fr); offs.append(o)
    assert off.tolist() == offs == [search, shift, search, search]
    assert same_bits(audio, np.concatenate(frames))
    ref, ref_off = R.stitch(w, sola_len, search, frame, offsets=off)
    err = float(np.max(np.abs(audio.astype(np.float64) - ref)))
    print("stitch (%d, %d, %d): error against fp64 %.3e" % (sola_len, search, frame, err))
    assert err <= 2e-6
    assert R.stitch(w, sola_len, search, frame)[1].tolist() == off.tolist()      # the fp64 search agrees on these windows


def test_stitch_refusals(plain_engine):
    w = np.zeros((2, 384), np.float32)
    for a in ((96, 48, 241), (96, 1024, 240), (97, 48, 96), (0, 48, 240)):      # window too short; search > 1023; frame < sola_len; no crossfade
        with pytest.raises(RvcInferError) as x:
            plain_engine.sola_stitch(w if a[1] < 1024 else np.zeros((1, 2000), np.float32), *a)
        assert x.value.code == 5


# ---------------------------------------------------------------- 3. convert = the composition of public calls
def configure(e, case):
    if case == "index":
        e.load_index(np.random.default_rng(5).standard_normal((64, 48)).astype(np.float32))
        e.set_index_rate(0.5); e.set_protect(0.33)
    elif case == "formant":
        e.set_formant_shift(2.0)


@pytest.mark.parametrize("case", ["plain", "index", "yin", "formant"])
def test_convert_is_the_composition(case):
    e = engine(3, "yin" if case == "yin" else "rmvpe")
    configure(e, case)
    x = recording()
    ref, ref_off = composition(e, x)
    got, rate = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    info = e.convert_info()
    assert rate == 100 * ZC and got.shape == (234 * ZC,) and info["windows"] == 5 and info["batches"] == 2
    assert info["offsets"].tolist() == ref_off.tolist()
    assert same_bits(got, ref)
    assert np.all(np.isfinite(got))
    assert info["ms_highpass"] == 0.0 and info["ms_model"] > 0 and info["ms_stitch"] > 0 and info["ms_total"] >= info["ms_model"]
    # high-pass on: the same composition fed rvc_highpass(x)
    xh = guard(e.highpass, x)
    ref_h, off_h = composition(e, xh)
    got_h, _ = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=True)
    assert same_bits(got_h, ref_h) and e.convert_info()["offsets"].tolist() == off_h.tolist() and e.convert_info()["ms_highpass"] > 0
    assert not same_bits(got_h, got)
    e.close()


# ---------------------------------------------------------------- 4. no dependence on history
def test_convert_does_not_depend_on_history():
    x = recording()
    fresh = engine(3)
    want, _ = guard(fresh.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    want_off = fresh.convert_info()["offsets"].tolist()
    fresh.close()
    e = engine(3)
    junk = np.stack([voice_signal(g160.input_buffer_16k_size, seed=s) for s in (1, 2, 3)])
    for _ in range(3):      # another geometry: pitch caches and chunk counters are left dirty
        guard(e.infer_batch, junk, g160.sample_frame_16k, 0, g160.skip_head, g160.model_return_length)
    got, _ = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    assert same_bits(got, want) and e.convert_info()["offsets"].tolist() == want_off
    e.close()


# ---------------------------------------------------------------- 5. one stream
def test_convert_one_stream():
    e = engine(1)
    x = recording()
    ref, ref_off = composition(e, x)
    got, _ = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    info = e.convert_info()
    assert info["windows"] == 5 and info["batches"] == 5
    assert same_bits(got, ref) and info["offsets"].tolist() == ref_off.tolist()
    e.close()


# ---------------------------------------------------------------- 6. statuses
def test_convert_statuses():
    L, z = _native.lib(), zoo("tiny", 2)
    x = recording()
    out = np.empty(234 * ZC, np.float32)
    n = C.c_size_t(0)

    def call(e, n_in=len(x), cap=len(out)):
        n.value = 0
        return L.rvc_convert(e._h, x.ctypes.data_as(_FP), n_in, K, CTX, XF, SHIFT, 0, out.ctypes.data_as(_FP), cap, C.byref(n))
    e = RvcInfer(z["data"])
    with pytest.raises(RvcInferError):
        e.convert_info()                                    # before a convert has completed
    assert call(e) == 1                                     # RVC_MODEL_NOT_LOADED, and before the arguments are looked at:
    assert call(e, n_in=0) == 1
    e.load_model(z["model"])
    assert call(e) == 2                                     # RVC_CONTENTVEC_NOT_LOADED
    e.load_contentvec(2)
    assert call(e) == 3                                     # RVC_F0_NOT_LOADED
    e.load_f0_method("yin")
    assert call(e, cap=len(out) - 1) == 5 and n.value == len(out)      # cap one short: RVC_SHAPE, *out_len written
    assert call(e, n_in=0) == 5                             # n = 0
    assert L.rvc_convert(e._h, x.ctypes.data_as(_FP), len(x), 1, CTX, XF, 0, 0, out.ctypes.data_as(_FP), len(out), C.byref(n)) == 5      # k = 1
    assert b"k" in L.rvc_last_error_message(e._h)
    with pytest.raises(RvcInferError):
        e.convert_info()                                    # still none
    assert guard(call, e) == 0 and n.value == len(out)
    assert e.convert_info()["windows"] == 5 and e.convert_info()["batches"] == 5
    with pytest.raises(RvcInferError) as err:
        e.highpass(np.zeros(0, np.float32))
    assert err.value.code == 5
    e.close()
