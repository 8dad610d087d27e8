"""A file at any rate, with the volume envelope (obs_rvc_amd/csrc/resample_whole.hip.h, change_rms.hip.h, convert.hip.h) on the tiny zoo
(sr = 4800, zc = 48): the whole-signal converter and the envelope against the fp64 definitions of tests/resample_whole_ref.py, rvc_convert_file against the
composition of the public calls bit for bit, the statuses.  A HIP error ends the session: nothing more is started on the device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import resample_whole_ref as R
from common import synth_zoo, voice_signal, zoo
from obs_rvc_amd import _native
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError
from test_gpu_convert import CTX, K, SHIFT, XF, ZC, engine, guard, same_bits

pytestmark = pytest.mark.gpu

_FP = C.POINTER(C.c_float)
RATE_IN, N_IN, RMS_MIX, RATE_OUT = 22050, 51500, 0.25, 4410      # the file of the composition tests: 37 370 samples at 16 kHz, Nf = 234, W = 5


@pytest.fixture(scope="module")
def plain_engine():
    e = RvcInfer(zoo("tiny", 2)["data"])
    yield e
    e.close()


def engine_taps(o, n):
    """the engine's own filter table [n][K] (rvc_debug_formant_table): the definition's taps, bit for bit"""
    L = _native.lib()
    width = C.c_size_t()
    assert L.rvc_debug_formant_table(o, n, None, 0, C.byref(width)) == 1
    out = np.zeros(n * width.value, np.float32)
    assert L.rvc_debug_formant_table(o, n, out.ctypes.data_as(_FP), out.size, C.byref(width)) == 0
    return out.reshape(n, width.value)


# ---------------------------------------------------------------- 1. the converter against fp64
# the issue's cases, then the launch shapes they do not reach: two outputs per thread (12 -> 1), one (40 -> 1), a tile shorter than the phase cycle (1 -> 2048),
# and a filter too long for the LDS (2048 -> 1: the kernel that reads global memory)
RESAMPLE_CASES = [(22050, 16000, 5003), (44100, 16000, 4410), (48000, 16000, 1000), (16000, 48000, 333), (4800, 4410, 700), (3, 2, 1), (3, 2, 7), (441, 160, 440),
                  (192000, 16000, 9000), (40, 1, 20000), (1, 2048, 3), (2048, 1, 600000)]


@pytest.mark.parametrize("ri,ro,n_in", RESAMPLE_CASES)
def test_resampler_against_fp64(plain_engine, ri, ro, n_in):
    geo = R.geometry(ri, ro, n_in)
    assert RvcInfer.resample_geometry(ri, ro, n_in) == geo
    x = R.resample_signal(n_in, 20.0 * max(1, -(-geo["o"] // geo["n"])))      # (the sine stays inside the output's band)
    taps = engine_taps(geo["o"], geo["n"])
    assert np.abs(taps - R.table(geo["o"], geo["n"])).max() <= 1e-7
    ref = R.resample(x, ri, ro, np.float64, taps)
    # the bound: 8 x the largest error of the same recipe evaluated in float32 numpy, floor 1e-6 absolute (the rule of test_highpass_against_fp64).  The
    # recipe's sums are numpy's matrix product, which adds in blocks; the one row of 24 826 taps of 2048 -> 1 is defined as ONE chain, whose float32 error
    # grows with the square root of its length (about sqrt(24 826) 2^-24 |sum| = 5e-6 here): its yardstick adds sequentially too
    err32 = float(np.max(np.abs(R.resample(x, ri, ro, np.float32, taps, sequential=geo["o"] == 2048).astype(np.float64) - ref)))
    got = guard(plain_engine.resample, x, ri, ro)
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print("resample %d -> %d, n = %d: kernel error %.3e, float32 numpy error %.3e" % (ri, ro, n_in, err, err32))
    assert got.shape == (geo["n_out"],) and got.dtype == np.float32 and np.all(np.isfinite(got))
    assert err <= max(8.0 * err32, 1e-6), (err, err32)
    assert float(np.max(np.abs(got))) > 0.1


def test_resampler_identity_is_a_copy(plain_engine):
    x = R.resample_signal(100)
    assert same_bits(guard(plain_engine.resample, x, 16000, 16000), x)
    assert same_bits(guard(plain_engine.resample, x, 300, 300), x)


@pytest.mark.parametrize("ri,ro,n_in", [(44100, 16000, 4410), (16000, 48000, 333), (2048, 1, 600000), (16000, 16000, 100)])
def test_resample_device_is_resample(plain_engine, ri, ro, n_in):
    import torch
    x = R.resample_signal(n_in)
    want = guard(plain_engine.resample, x, ri, ro)
    d_x = torch.from_numpy(x).cuda()
    d_y = torch.full((len(want) + 3,), -7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    n = C.c_size_t()
    rc = _native.lib().rvc_resample_device(plain_engine._h, C.c_void_p(d_x.data_ptr()), n_in, ri, ro, C.c_void_p(d_y.data_ptr()), len(want), C.byref(n))
    if rc != 0:
        guard(plain_engine._chk, rc)
    got = d_y.cpu().numpy()
    assert n.value == len(want) and same_bits(got[:len(want)], want) and (got[len(want):] == -7.5).all()
    assert same_bits(d_x.cpu().numpy(), x)


# ---------------------------------------------------------------- 2. the envelope against fp64
def env_lengths(rate_src, rate_y):
    """(n_src, n_y): F_1 = F_2 = 1 (signals shorter than a hop; none at a hop of one sample), F_1 = 5 with F_2 = 3, exact multiples of the hop"""
    h1, h2 = rate_src // 2, rate_y // 2
    short = [(h1 - 1, h2 - 1)] if h1 > 1 and h2 > 1 else []
    return short + [(4 * h1 + h1 // 3, 2 * h2 + h2 // 2), (3 * h1, 4 * h2)]


ENV_CASES = [(rs, ry, n1, n2) for rs, ry in ((16000, 4800), (201, 99), (2, 2)) for n1, n2 in env_lengths(rs, ry)]


@pytest.mark.parametrize("rate_src,rate_y,n_src,n_y", ENV_CASES)
def test_envelope_against_fp64(plain_engine, rate_src, rate_y, n_src, n_y):
    F1, F2 = R.rms_frames(n_src, rate_src)[2], R.rms_frames(n_y, rate_y)[2]
    assert (F1, F2) in ((1, 1), (5, 3), (4, 5))
    for kind in R.ENV_KINDS:
        src, y = R.env_case(n_src, n_y, kind)
        for rate in (0.0, 0.25, 1.0):
            m64 = R.change_rms(src, rate_src, y, rate_y, rate)
            d32 = float(np.abs(R.change_rms(src, rate_src, y, rate_y, rate, np.float32).astype(np.float64) - m64).max())
            peak = float(np.abs(m64).max())
            got = guard(plain_engine.change_rms, src, rate_src, y, rate_y, rate)
            err = float(np.abs(got.astype(np.float64) - m64).max())
            print("change_rms %d/%d n = %d/%d %s rate = %.2f: delta32 = %.3e kernel = %.3e peak = %.3e" % (rate_src, rate_y, n_src, n_y, kind, rate, d32, err, peak))
            # the rule of tests/test_gpu_post.py: the kernel gets 2 x delta32, and an ill-conditioned input must not widen its own tolerance
            assert d32 <= 1e-4 * peak or peak == 0, (kind, rate, d32, peak)
            assert got.dtype == np.float32 and np.isfinite(got).all() and err <= 2.0 * d32, (kind, rate, err, d32)
            if rate == 1.0:
                assert same_bits(got, y)
            elif kind in ("silent_out", "silent_src"):
                assert not np.any(got)
            else:
                assert not same_bits(got, y)


# ---------------------------------------------------------------- 3. convert_file = the composition of public calls
def file_recording():
    return voice_signal(N_IN, seed=11, sr=RATE_IN)


def file_composition(e, x, highpass):
    """what rvc_convert_file computes, from public calls -> (audio, offsets)"""
    x16 = guard(e.resample, x, RATE_IN, 16000)
    y, sr = guard(e.convert, x16, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=highpass)
    off = e.convert_info()["offsets"].tolist()
    assert sr == 100 * ZC and len(x16) == 37370 and len(y) == 234 * ZC
    src = guard(e.highpass, x16) if highpass else x16
    y2 = guard(e.change_rms, src, 16000, y, sr, RMS_MIX)
    assert not same_bits(y2, y)
    return guard(e.resample, y2, sr, RATE_OUT), off


@pytest.mark.parametrize("highpass", [True, False])
def test_convert_file_is_the_composition(highpass):
    e = engine(3)
    x = file_recording()
    ref, ref_off = file_composition(e, x, highpass)
    got, rate = guard(e.convert_file, x, RATE_IN, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=highpass, rms_mix_rate=RMS_MIX, out_rate=RATE_OUT)
    info, f = e.convert_info(), e.convert_file_info()
    assert rate == RATE_OUT == f["rate"] and got.shape == (234 * ZC * 147 // 160 + 1,) and info["windows"] == 5 and info["batches"] == 2
    assert info["offsets"].tolist() == ref_off
    assert same_bits(got, ref) and np.all(np.isfinite(got))
    assert f["peak"] == np.max(np.abs(got)) and f["peak"] > 0
    assert f["ms_resample_in"] > 0 and f["ms_envelope"] > 0 and f["ms_resample_out"] > 0 and (f["ms_highpass"] > 0) == highpass
    assert f["ms_model"] == info["ms_model"] and f["ms_stitch"] == info["ms_stitch"] and f["ms_total"] >= f["ms_model"]
    # a junk call of another geometry, rate and setting in between: the result is unchanged
    junk, jr = guard(e.convert_file, voice_signal(30000, seed=3, sr=48000), 48000, k=3, context=4, crossfade=1, pitch_shift=0, highpass=not highpass, rms_mix_rate=0.0)
    assert jr == 100 * ZC and e.convert_file_info()["ms_resample_out"] == 0.0
    again, _ = guard(e.convert_file, x, RATE_IN, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=highpass, rms_mix_rate=RMS_MIX, out_rate=RATE_OUT)
    assert same_bits(again, got) and e.convert_info()["offsets"].tolist() == ref_off and e.convert_file_info()["peak"] == f["peak"]
    e.close()


def test_convert_file_at_32k_five_stages_is_the_composition():
    # the rate plumbing at a model rate of 32000 (zc = 320) behind a five-stage decoder: upstream's v1 32k layout at toy width (10 * 4 * 2 * 2 * 2, ContentVec v1),
    # a 44.1 kHz file of the same 37 370 samples at 16 kHz, out at 22.05 kHz.  Not new numerics: bit for bit the composition of the public calls
    rate_in, rate_out, zc = 44100, 22050, 320
    z, version = synth_zoo("tiny_v1_32k")
    e = RvcInfer(z["data"])
    e.load_contentvec(version); e.load_model(z["model"]); e.load_f0_method("rmvpe")
    e.set_streams(3); e.set_noise_seed(1234, 0)
    x = voice_signal(2 * N_IN, seed=11, sr=rate_in)
    x16 = guard(e.resample, x, rate_in, 16000)
    y, sr = guard(e.convert, x16, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=True)
    off = e.convert_info()["offsets"].tolist()
    assert sr == 100 * zc == 32000 and len(x16) == 37370 and y.shape == (234 * zc,)
    y2 = guard(e.change_rms, guard(e.highpass, x16), 16000, y, sr, RMS_MIX)
    ref = guard(e.resample, y2, sr, rate_out)
    got, rate = guard(e.convert_file, x, rate_in, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=True, rms_mix_rate=RMS_MIX, out_rate=rate_out)
    info, f = e.convert_info(), e.convert_file_info()
    assert rate == rate_out == f["rate"] and got.shape == (RvcInfer.resample_geometry(sr, rate_out, 234 * zc)["n_out"],) and info["windows"] == 5 and info["batches"] == 2
    assert info["offsets"].tolist() == off
    assert same_bits(got, ref) and np.all(np.isfinite(got)) and f["peak"] == np.max(np.abs(got)) and f["peak"] > 0
    # ... and at the model's own rate: no output converter, 234 x 320 samples
    own, rate = guard(e.convert_file, x, rate_in, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=True, rms_mix_rate=RMS_MIX, out_rate=0)
    assert rate == 32000 and same_bits(own, y2) and e.convert_file_info()["ms_resample_out"] == 0.0
    e.close()


def test_convert_file_without_its_stages_is_convert():
    e = engine(3)
    x16 = voice_signal(160 * 233 + 77, seed=11)
    want, sr = guard(e.convert, x16, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=True)
    want_off = e.convert_info()["offsets"].tolist()
    got, rate = guard(e.convert_file, x16, 16000, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=True, rms_mix_rate=1.0, out_rate=0)
    f = e.convert_file_info()
    assert rate == sr and same_bits(got, want) and e.convert_info()["offsets"].tolist() == want_off
    assert f["ms_resample_in"] == 0.0 and f["ms_envelope"] == 0.0 and f["ms_resample_out"] == 0.0 and f["peak"] == np.max(np.abs(got))
    got2, rate2 = guard(e.convert_file, x16, 16000, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=True, rms_mix_rate=1.0, out_rate=sr)      # the model's rate by name
    assert rate2 == sr and same_bits(got2, want)
    e.close()


def test_convert_file_device_is_convert_file():
    import torch
    e = engine(3)
    x = file_recording()
    want, _ = guard(e.convert_file, x, RATE_IN, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=True, rms_mix_rate=RMS_MIX, out_rate=RATE_OUT)
    peak = e.convert_file_info()["peak"]
    d_x = torch.from_numpy(x).cuda()
    d_y = torch.full((len(want) + 3,), -7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    n = C.c_size_t()
    rc = _native.lib().rvc_convert_file_device(e._h, C.c_void_p(d_x.data_ptr()), len(x), RATE_IN, K, CTX, XF, SHIFT, 1, RMS_MIX, RATE_OUT, C.c_void_p(d_y.data_ptr()), len(want),
                                               C.byref(n))
    if rc != 0:
        guard(e._chk, rc)
    got = d_y.cpu().numpy()
    assert n.value == len(want) and same_bits(got[:len(want)], want) and (got[len(want):] == -7.5).all() and e.convert_file_info()["peak"] == peak
    e.close()


# ---------------------------------------------------------------- 4. statuses
def test_resample_and_change_rms_statuses(plain_engine):
    L, e = _native.lib(), plain_engine
    x = R.resample_signal(441)
    out = np.full(161, -7.5, np.float32)
    n = C.c_size_t(0)

    def call(n_in=441, ri=44100, ro=16000, cap=160):
        n.value = 0
        return L.rvc_resample(e._h, x.ctypes.data_as(_FP), n_in, ri, ro, out.ctypes.data_as(_FP), cap, C.byref(n))
    assert call(ri=0) == 5 and call(ro=0) == 5 and b"rate" in L.rvc_last_error_message(e._h)
    assert call(ri=16001) == 5 and call(ri=1, ro=2049) == 5 and b"2048" in L.rvc_last_error_message(e._h)
    assert call(n_in=0) == 5 and n.value == 0
    assert call(cap=159) == 5 and n.value == 160 and out[0] == -7.5      # cap one short: *n_out written, nothing else
    assert guard(call) == 0 and n.value == 160 and out[160] == -7.5 and same_bits(out[:160], e.resample(x, 44100, 16000))
    g = (C.c_size_t * 4)()
    assert L.rvc_resample_geometry(44100, 16000, 441, g) == 0 and list(g) == [441, 160, 17, 160]
    src, y = R.env_case(300, 200, "plain")
    for bad in (dict(rate=-0.01), dict(rate=1.01), dict(rate=float("nan")), dict(rate_src=1), dict(rate_y=1), dict(rate_y=0), dict(src=src[:0]), dict(y=y[:0])):
        a = {**dict(src=src, rate_src=201, y=y, rate_y=99, rate=0.25), **bad}
        with pytest.raises(RvcInferError) as err:
            e.change_rms(**a)
        assert err.value.code == 5, bad
    assert not same_bits(guard(e.change_rms, src, 201, y, 99, 0.25), y)


def test_convert_file_statuses():
    L, z = _native.lib(), zoo("tiny", 2)
    x = file_recording()
    n_out = 234 * ZC * 147 // 160 + 1
    out = np.full(n_out, -7.5, np.float32)
    n = C.c_size_t(0)

    def call(e, n_in=len(x), ri=RATE_IN, k=K, mix=RMS_MIX, ro=RATE_OUT, cap=n_out):
        n.value = 0
        return L.rvc_convert_file(e._h, x.ctypes.data_as(_FP), n_in, ri, k, CTX, XF, SHIFT, 1, mix, ro, out.ctypes.data_as(_FP), cap, C.byref(n))
    e = RvcInfer(z["data"])
    with pytest.raises(RvcInferError):
        e.convert_file_info()                               # before one has completed
    assert call(e) == 1 and call(e, n_in=0) == 1 and call(e, ri=0) == 1      # RVC_MODEL_NOT_LOADED, and before the arguments are looked at
    e.load_model(z["model"])
    assert call(e) == 2                                     # RVC_CONTENTVEC_NOT_LOADED
    e.load_contentvec(2)
    assert call(e) == 3                                     # RVC_F0_NOT_LOADED
    e.load_f0_method("yin")
    for bad in (dict(ri=0), dict(ri=16001), dict(n_in=0), dict(k=1), dict(mix=-0.5), dict(mix=1.5), dict(mix=float("nan")), dict(ro=4801)):
        assert call(e, **bad) == 5 and n.value == 0, bad
        assert L.rvc_last_error_message(e._h)
    assert call(e, cap=n_out - 1) == 5 and n.value == n_out and out[0] == -7.5      # cap one short: RVC_SHAPE, *out_len written
    with pytest.raises(RvcInferError):
        e.convert_file_info()                               # still none
    assert guard(call, e) == 0 and n.value == n_out
    f = e.convert_file_info()
    assert f["rate"] == RATE_OUT and f["peak"] == np.max(np.abs(out)) and e.convert_info()["windows"] == 5 and e.convert_info()["batches"] == 5
    e.close()
