"""The file converter's host-only parts: rvc_convert_geometry against the formulas restated in tests/convert_ref.py, its RVC_SHAPE
cases, the self-checks of the fp64 definitions, and the command-line tool's plain functions (argument parsing, WAV writing).  No GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import convert_ref as R
from obs_rvc_amd import _native
from obs_rvc_amd.build_index import read_wav
from obs_rvc_amd.convert import normalise_peak, parse_args, write_wav
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError

KEYS = ("windows", "n", "sample_frame_16k_size", "skip_head", "return_length", "hop", "zc", "output_samples")


def c_geometry(n16k, rate, k, context, crossfade):
    out = (C.c_size_t * 8)()
    rc = _native.lib().rvc_convert_geometry(n16k, rate, k, context, crossfade, out)
    return rc, dict(zip(KEYS, (int(v) for v in out)))


def test_reference_self_checks():
    R.self_check()


@pytest.mark.parametrize("k", [2, 16, 32])
@pytest.mark.parametrize("n16k", [1, 160, 160 * 233 + 77, 9_600_000])
def test_geometry_matches_formulas(k, n16k):
    for rate in (4800, 40000, 48000):
        for context, crossfade in ((3, 1), (3, 2), (0, 0)) if k > 2 else ((3, 1), (3, 2), (28, 3)):
            rc, got = c_geometry(n16k, rate, k, context, crossfade)
            want = R.geometry(n16k, rate, k, context, crossfade)
            assert rc == 0 and got == want, (k, n16k, rate, context, crossfade, got, want)
            assert got["n"] == 5120 * k - 160 and got["return_length"] + 2 * got["skip_head"] == 32 * k - 1
            assert RvcInfer.convert_geometry(n16k, rate, k, context, crossfade) == want


def test_geometry_defaults_and_the_issue_case():
    assert c_geometry(16000, 48000, 0, 0, 0) == c_geometry(16000, 48000, 14, 48, 5)
    rc, g = c_geometry(160 * 233 + 77, 4800, 2, 3, 2)
    assert rc == 0 and g == {"windows": 5, "n": 10080, "sample_frame_16k_size": 5120, "skip_head": 3, "return_length": 57, "hop": 54, "zc": 48,
                             "output_samples": 234 * 48}


@pytest.mark.parametrize("k,context,crossfade,rate", [
    (1, 3, 1, 48000), (33, 3, 1, 48000),      # k outside [2, 32]
    (16, 2, 1, 48000),                        # context below 3
    (2, 28, 4, 48000),                        # H = 63 - 56 - 4 - 1 = 2 < X = 4  (X = 3 gives H = 3 = X, accepted above)
    (2, 0, 0, 48000),                         # the default context of 48 does not fit a 63-frame window
    (16, 3, 1, 48050), (16, 3, 1, 0),         # a rate that is no multiple of 100
    (16, 3, 1, 102400),                       # one frame of the model rate is longer than the SOLA kernels' 1023-sample search
])
def test_geometry_shape_errors(k, context, crossfade, rate):
    assert R.geometry(16000, rate, k, context, crossfade) is None
    assert c_geometry(16000, rate, k, context, crossfade)[0] == 5
    with pytest.raises(RvcInferError):
        RvcInfer.convert_geometry(16000, rate, k, context, crossfade)
    assert _native.lib().rvc_convert_geometry(16000, 48000, 16, 3, 1, None) == 5


def test_cli_parse_args():
    a = parse_args(["in.wav", "-o", "out.wav", "--model", "voice.rvcw"])
    assert (a.input, a.output, a.model, a.version, a.f0, a.index, a.streams, a.window, a.context, a.crossfade, a.highpass, a.rate, a.pitch, a.formant, a.protect) == \
        ("in.wav", "out.wav", "voice.rvcw", 2, "rmvpe", None, 8, 0, 0, 0, True, 0, 0.0, 0.0, 0.5)
    a = parse_args(["in.wav", "-o", "o.wav", "--model", "m", "--data", "d", "--version", "1", "--f0", "yin", "--index", "i.index", "--index-rate", "0.5", "--index-k", "4",
                    "--nprobe", "3", "--pitch", "-7.5", "--formant", "2", "--protect", "0.33", "--streams", "64", "--window", "8", "--context", "24", "--crossfade", "4",
                    "--no-highpass", "--rate", "44100"])
    assert (a.data, a.version, a.f0, a.index, a.index_rate, a.index_k, a.nprobe, a.pitch, a.formant, a.protect, a.streams, a.window, a.context, a.crossfade, a.highpass,
            a.rate) == ("d", 1, "yin", "i.index", 0.5, 4, 3, -7.5, 2.0, 0.33, 64, 8, 24, 4, False, 44100)
    for bad in (["--pitch", "25"], ["--formant", "6"], ["--protect", "0.6"], ["--streams", "0"], ["--window", "33"], ["--window", "1"], ["--context", "2"],
                ["--index-k", "5"], ["--f0", "crepe"], ["--rate", "44150"], ["--nprobe", "65"]):
        with pytest.raises(SystemExit):
            parse_args(["in.wav", "-o", "o.wav", "--model", "m"] + bad)
    with pytest.raises(SystemExit):
        parse_args(["in.wav", "-o", "o.wav"])


def test_wav_round_trip_and_peak_rule(tmp_path):
    r = np.random.default_rng(3)
    x = r.uniform(-0.9, 0.9, 4801).astype(np.float32)
    write_wav(tmp_path / "a.wav", x, 48000)
    y, rate = read_wav(tmp_path / "a.wav")
    # write rounds x * 32767 to the nearest integer, read divides by 32768
    assert rate == 48000 and y.dtype == np.float32 and len(y) == len(x)
    assert np.array_equal(y, (np.rint(x.astype(np.float64) * 32767.0) / 32768.0).astype(np.float32))
    assert np.max(np.abs(y - x)) <= 1.5 / 32768.0      # half a step of rounding, and |x| / 32768 from the two scales
    # a peak of 1 or below is left alone; above 1 the signal is divided by peak / 0.99
    assert normalise_peak(x) is x or np.array_equal(normalise_peak(x), x)
    one = np.array([0.5, -1.0, 0.25], np.float32)
    assert np.array_equal(normalise_peak(one), one)
    loud = np.array([0.5, -2.0, 1.0], np.float32)
    assert np.allclose(normalise_peak(loud), loud * 0.99 / 2.0, rtol=1e-6, atol=0)
    write_wav(tmp_path / "b.wav", loud, 40000)
    z, rate = read_wav(tmp_path / "b.wav")
    assert rate == 40000 and np.allclose(z, [0.2475, -0.99, 0.495], rtol=0, atol=2.0 / 32768.0) and np.max(np.abs(z)) < 1.0
    write_wav(tmp_path / "c.wav", np.zeros(0, np.float32), 16000)
    assert len(read_wav(tmp_path / "c.wav")[0]) == 0


def test_long_window_geometries_of_the_stage_tests():
    # tests/test_gpu_long_windows.py: one window is n = 5120 k - 160 samples, Tm = 32 k f0 frames (n == the f0 frame), T = 16 k - 1 ContentVec frames and
    # R = F - 2 C returned ones -- its table against rvc_convert_geometry, and the far-end row's context C = ceil((F - 351) / 2)
    import long_shapes as LW
    import yin_ref as Y
    rows = dict(LW.GEOMETRIES)
    for k in (31, 32):
        rows[(k, LW.far_end_context(k), 1)] = (32 * k, 16 * k - 1, 351)
    assert LW.far_end_context(31) == 320 and LW.far_end_context(32) == 336 and LW.far_end_context(14) == 48
    for (k, ctx, xf), (Tm, T, R_) in rows.items():
        geo = RvcInfer.convert_geometry(160, 4800, k, ctx, xf)
        F = 32 * k - 1
        assert geo["n"] == 160 * F == 5120 * k - 160 and geo["skip_head"] == ctx and geo["return_length"] == R_ == F - 2 * ctx
        assert geo["sample_frame_16k_size"] == 5120 * (k - 1) and Y.f0_frame(geo["sample_frame_16k_size"]) == geo["n"]      # n == frame
        assert Tm == 32 * k == 1 + geo["n"] // 160 and T == 16 * k - 1 == (F - 1) // 2 and 2 * T + 1 == F
        assert ctx + R_ <= 2 * T + 1 and R_ <= LW.R_MAX
        assert LW.geometry(k, ctx, xf) == (geo["n"], geo["sample_frame_16k_size"], ctx, R_)
    assert RvcInfer.convert_geometry(160, 4800) == RvcInfer.convert_geometry(160, 4800, 14, 48, 5)
