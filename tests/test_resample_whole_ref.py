"""The definitions of tests/resample_whole_ref.py checked by what they must do, and the host-only entry points against them:
rvc_resample_geometry, the command-line tools' new options.  No GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import resample_whole_ref as R
from obs_rvc_amd import _native
from obs_rvc_amd.build_index import parse_args as index_args
from obs_rvc_amd.convert import normalise_peak, parse_args
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError


def test_reference_self_checks():
    R.self_check()


@pytest.mark.parametrize("ri,ro", [(22050, 16000), (44100, 16000), (48000, 16000), (16000, 48000), (4800, 4410), (3, 2), (441, 160), (16000, 16000)])
@pytest.mark.parametrize("n_in", [1, 7, 440, 5003])
def test_length_rule_and_the_c_geometry(ri, ro, n_in):
    geo = R.geometry(ri, ro, n_in)
    o, n = geo["o"], geo["n"]
    assert o * ro == n * ri and np.gcd(o, n) == 1
    assert geo["n_out"] == -(-n_in * n // o) and (geo["n_out"] - 1) * o < n_in * n <= geo["n_out"] * o
    x = np.random.default_rng(n_in).standard_normal(n_in).astype(np.float32)
    assert len(R.resample(x, ri, ro)) == geo["n_out"]
    out = (C.c_size_t * 4)()
    assert _native.lib().rvc_resample_geometry(ri, ro, n_in, out) == 0
    assert dict(zip(("o", "n", "w", "n_out"), (int(v) for v in out))) == geo == RvcInfer.resample_geometry(ri, ro, n_in)


@pytest.mark.parametrize("ri,ro,n_in", [(0, 16000, 5), (16000, 0, 5), (16000, 16000, 0), (4099, 2, 5), (2, 2049, 5), (1 << 20, (1 << 20) - 1, 5)])
def test_geometry_refusals(ri, ro, n_in):
    assert R.geometry(ri, ro, n_in) is None
    out = (C.c_size_t * 4)()
    assert _native.lib().rvc_resample_geometry(ri, ro, n_in, out) == 5
    with pytest.raises(RvcInferError):
        RvcInfer.resample_geometry(ri, ro, n_in)
    assert _native.lib().rvc_resample_geometry(3, 2, 5, None) == 5
    assert R.geometry(2048 * 7, 2047 * 7, 5) is not None and _native.lib().rvc_resample_geometry(2048 * 7, 2047 * 7, 5, out) == 0      # the largest terms accepted


def test_identity_ratio_is_a_copy():
    x = R.resample_signal(100)
    for dtype in (np.float64, np.float32):
        y = R.resample(x, 16000, 16000, dtype)
        assert y.dtype == dtype and np.array_equal(y, x.astype(dtype))
    assert np.array_equal(R.resample(x, 300, 300), R.resample(x, 1, 1))


def test_sine_through_441_to_160():
    # 440 Hz at 44.1 kHz -> 16 kHz: far inside the pass band, so the samples are the sine's at the new rate, away from the ends
    n = 8820
    x = np.sin(2 * np.pi * 440.0 * np.arange(n) / 44100.0)
    y = R.resample(x, 44100, 16000)
    ref = np.sin(2 * np.pi * 440.0 * np.arange(len(y)) / 16000.0)
    mid = slice(200, len(y) - 200)
    assert len(y) == 3200 and np.abs(y[mid] - ref[mid]).max() < 1e-3
    assert abs(np.abs(y[mid]).max() - 1.0) < 1e-3
    assert np.abs(R.resample(x, 44100, 16000, np.float32).astype(np.float64) - y).max() < 1e-5


def test_half_pixel_interpolation_by_hand():
    # F = 1: a constant
    assert np.array_equal(R.lerp_half_pixel([0.25], 5), np.full(5, 0.25))
    # F = 3 to 6 points: u = 0, 0.25, 0.75, 1.25, 1.75, 2.25 (the first clamped at 0 from -0.25), the last with i1 clamped at 2
    u, i0, i1 = R.half_pixel_positions(3, 6)
    assert np.allclose(u, [0, 0.25, 0.75, 1.25, 1.75, 2.25], rtol=0, atol=1e-15)
    assert i0.tolist() == [0, 0, 0, 1, 1, 2] and i1.tolist() == [1, 1, 1, 2, 2, 2]
    r = np.array([1.0, 3.0, 11.0])
    assert np.allclose(R.lerp_half_pixel(r, 6), [1.0, 1.5, 2.5, 5.0, 9.0, 11.0], rtol=0, atol=1e-14)
    torch = pytest.importorskip("torch")
    for F, size in ((3, 6), (5, 7200), (1, 9), (7, 4)):
        v = np.random.default_rng(F + size).standard_normal(F)
        want = torch.nn.functional.interpolate(torch.from_numpy(v)[None, None], size=size, mode="linear", align_corners=False)[0, 0].numpy()
        assert np.abs(R.lerp_half_pixel(v, size) - want).max() <= 1e-12


@pytest.mark.parametrize("rate_src,rate_y,n_src,n_y", [(16000, 4800, 80000, 24000), (201, 99, 2010, 990), (2, 2, 40, 40)])
def test_change_rms_at_rate_0_takes_on_the_source_envelope(rate_src, rate_y, n_src, n_y):
    src, y = R.env_case(n_src, n_y, "plain")
    out = R.change_rms(src, rate_src, y, rate_y, 0.0)
    # out = y R_1 / R_2 sample by sample, so where both interpolated tracks are flat the framed RMS of the output is the source's.  Made flat here: signals of
    # constant magnitude, whose tracks are flat wherever no frame that a sample interpolates between reaches into the zero padding
    src_c, y_c = np.sign(src) * np.float32(0.3), np.sign(y) * np.float32(0.05)
    out_c = R.change_rms(src_c, rate_src, y_c, rate_y, 0.0)
    flat = (np.abs(R.lerp_half_pixel(R.rms_track(src_c, rate_src), n_y) - np.float32(0.3)) < 1e-12) & \
           (np.abs(R.lerp_half_pixel(R.rms_track(y_c, rate_y), n_y) - np.float32(0.05)) < 1e-12)
    got = R.rms_track(out_c, rate_y)
    L, hop, F = R.rms_frames(n_y, rate_y)
    inner = [f for f in range(F) if f * hop - L // 2 >= 0 and f * hop + L // 2 <= n_y and flat[f * hop - L // 2:f * hop + L // 2].all()]
    assert len(inner) >= 3
    for f in inner:
        assert abs(got[f] - np.float32(0.3)) < 1e-9
    # and in general: the ratio out / y is R_1 / max(R_2, floor), rate 1 is y itself, rate 0.5 lies between
    a = R.lerp_half_pixel(R.rms_track(src, rate_src), n_y)
    b = np.maximum(R.lerp_half_pixel(R.rms_track(y, rate_y), n_y), 1e-6)
    assert np.allclose(out, y.astype(np.float64) * a / b, rtol=1e-12, atol=0)
    assert np.array_equal(R.change_rms(src, rate_src, y, rate_y, 1.0), y.astype(np.float64))
    half = R.change_rms(src, rate_src, y, rate_y, 0.5)
    assert np.allclose(half * half, out * y.astype(np.float64), rtol=1e-10, atol=1e-300)
    assert not np.any(R.change_rms(src, rate_src, np.zeros(n_y, np.float32), rate_y, 0.25)) and not np.any(R.change_rms(np.zeros(n_src, np.float32), rate_src, y, rate_y, 0.25))


def test_float32_recipes_stay_close():
    for kind in R.ENV_KINDS:
        src, y = R.env_case(36000, 5000, kind)
        m64, m32 = R.change_rms(src, 16000, y, 4800, 0.25), R.change_rms(src, 16000, y, 4800, 0.25, np.float32)
        peak = np.abs(m64).max()
        assert m32.dtype == np.float32 and (np.abs(m32 - m64).max() <= 1e-4 * peak or peak == 0), kind
    x = R.resample_signal(5003)
    assert np.abs(R.resample(x, 22050, 16000, np.float32) - R.resample(x, 22050, 16000)).max() < 1e-5


def test_cli_options():
    base = ["in.wav", "-o", "out.wav", "--model", "m"]
    a = parse_args(base)
    assert (a.rms_mix_rate, a.resampler) == (1.0, "blocks")
    a = parse_args(base + ["--rms-mix-rate", "0.25", "--resampler", "device", "--rate", "44100"])
    assert (a.rms_mix_rate, a.resampler, a.rate) == (0.25, "device", 44100)
    for bad in (["--rms-mix-rate", "1.5"], ["--rms-mix-rate", "-0.1"], ["--rms-mix-rate", "nan"], ["--resampler", "host"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    assert index_args(["a.wav", "-o", "x.index"]).resampler == "blocks" and index_args(["a.wav", "-o", "x.index", "--resampler", "device"]).resampler == "device"
    with pytest.raises(SystemExit):
        index_args(["a.wav", "-o", "x.index", "--resampler", "host"])
    # the peak the device reports stands in for the host's pass over the samples
    loud = np.array([0.5, -2.0, 1.0], np.float32)
    assert np.array_equal(normalise_peak(loud, np.float32(2.0)), normalise_peak(loud)) and normalise_peak(loud, 1.0) is not None
    assert np.array_equal(normalise_peak(loud, 0.5), loud)
