"""Auto-transpose of the file converter (f0_analyze.hip.h, convert.hip.h convert_run) on the tiny zoo with YIN: a harmonic signal at
110 Hz (1.3 s, Nf = 130, k = 2, C = 3, X = 2: three windows, one batch of three streams) is measured and moved onto a target.

Bounds.  The transpose is folded into the factor rvc_set_pitch_semitones folds its own into, so a conversion with the target on equals, bit for bit, one with
the target off and the semitones set to the reported transpose; rvc_convert_f0 equals the target-off curve times (float)2^(a / 12) in one float multiply (the
arithmetic of DESIGN.md section 12); with the target off rvc_convert is the composition of public calls tests/test_gpu_convert.py holds it to, bit for bit."""
from __future__ import annotations

import os

import numpy as np
import pytest

import f0_stats_ref as S
from common import BASELINE_160MS as g160, voice_signal, zoo
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError
from test_gpu_convert import CTX, K, SHIFT, XF, composition, engine, guard, recording, same_bits

pytestmark = pytest.mark.gpu

N = 20800


def harmonic(f0=110.0, n=N):
    t = np.arange(n) / 16000.0
    return (0.3 * sum(np.sin(2 * np.pi * f0 * h * t) / h for h in range(1, 9))).astype(np.float32)


def conv(e, x, shift=0):
    y, _ = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=shift, highpass=False)
    return y


@pytest.fixture(scope="module")
def off():
    """the conversion with the target off, on a fresh engine: (audio, f0, the analysis of the signal)"""
    e = engine(3, "yin")
    x = harmonic()
    with pytest.raises(RvcInferError):
        e.auto_transpose_info()
    assert e.auto_transpose() == {"target_hz": 0.0, "step": 1, "limit": 12.0}
    y, f0 = conv(e, x), e.convert_f0()
    with pytest.raises(RvcInferError):
        e.auto_transpose_info()                    # target off: nothing was analysed
    an = guard(e.analyze_f0, x, K, CTX, XF, highpass=False)
    e.close()
    med, v = S.select(an)
    assert v > 60 and abs(float(med[0]) - 110.0) < 1.0
    return y, f0, an


def test_target_an_octave_up(off):
    y_off, f0_off, an = off
    e = engine(3, "yin")
    e.set_auto_transpose(220.0, 1, 12.0)
    assert e.auto_transpose() == {"target_hz": 220.0, "step": 1, "limit": 12.0}
    y = conv(e, harmonic())
    info = e.auto_transpose_info()
    med, v = S.select(an)
    assert info["semitones"] == 12.0 and info["voiced"] == v and same_bits(info["median_hz"], med[0])
    assert info["ms_analysis"] > 0 and info["ms_select"] > 0
    assert same_bits(e.convert_f0(), f0_off * np.float32(2.0)) and not same_bits(y, y_off)
    # limit 5 clamps
    e.set_auto_transpose(220.0, 1, 5.0)
    conv(e, harmonic())
    assert e.auto_transpose_info()["semitones"] == 5.0
    assert same_bits(e.convert_f0(), f0_off * S.factor(5.0))
    # whole octaves: 12 log2(160 / 110) = 6.49 -> 12
    e.set_auto_transpose(160.0, 12, 12.0)
    conv(e, harmonic())
    assert e.auto_transpose_info()["semitones"] == 12.0
    e.close()


def test_exact_transpose_is_the_semitone_setting(off):
    y_off, f0_off, an = off
    x = harmonic()
    e = engine(3, "yin")
    e.set_auto_transpose(233.0, 0, 24.0)
    y = conv(e, x)
    info, f0 = e.auto_transpose_info(), e.convert_f0()
    a = S.transpose(233.0, float(info["median_hz"]), info["voiced"], 0, 24.0)
    assert info["semitones"] == a and 12.5 < a < 13.5 and a != round(a)
    assert same_bits(f0, f0_off * S.factor(a))
    e.close()
    e = engine(3, "yin")
    e.set_pitch_semitones(a)
    assert same_bits(conv(e, x), y) and same_bits(e.convert_f0(), f0)
    e.close()


def test_silence_and_a_curve(off):
    e = engine(3, "yin")
    z = np.zeros(N, np.float32)
    y0 = conv(e, z)
    e.set_auto_transpose(220.0, 1, 12.0)
    y1 = conv(e, z)
    info = e.auto_transpose_info()
    assert info["voiced"] == 0 and info["semitones"] == 0.0 and info["median_hz"] == 0.0 and same_bits(y1, y0)
    # a curve that overrides every row at 440 Hz: the statistic describes the f0 that will be transposed
    e.set_f0_curve([0.0, 2.0], [440.0, 440.0])
    assert np.all(e.f0_curve_grid(130) == np.float32(440.0))
    conv(e, harmonic())
    info = e.auto_transpose_info()
    assert same_bits(info["median_hz"], np.float32(440.0)) and info["voiced"] == 130 and info["semitones"] == -12.0
    assert same_bits(e.convert_f0(), np.full(130, 220.0, np.float32))
    # ... and one that covers a few rows only leaves the median the tracker's
    e.set_f0_curve([0.5, 0.6], [440.0, 440.0])
    conv(e, harmonic())
    y_off, f0_off, an = off
    grid = e.f0_curve_grid(130)
    med, v = S.select(S.merge(grid, an))
    info = e.auto_transpose_info()
    assert same_bits(info["median_hz"], med[0]) and info["voiced"] == v and info["semitones"] == 12.0 and 5 < np.count_nonzero(~np.isnan(grid)) < 20
    e.close()


def test_a_model_without_pitch_guidance_ignores_the_setting():
    z = zoo("tiny")
    path = os.path.join(os.path.dirname(z["model"]), "model-tiny-nof0-v2.rvcw")
    if not os.path.exists(path):
        W.write_blob(path, *W.make_synth("tiny", 48, f0=False))
    e = RvcInfer(z["data"])
    e.load_contentvec(2); e.load_model(path); e.load_f0_method("yin"); e.set_streams(3); e.set_noise_seed(1234, 0)
    assert not e.model_has_f0()
    y0 = conv(e, harmonic())
    e.set_auto_transpose(220.0, 1, 12.0)
    assert same_bits(conv(e, harmonic()), y0)
    with pytest.raises(RvcInferError):
        e.auto_transpose_info()
    e.close()


def test_the_factor_is_gone_behind_the_call(off):
    y_off, f0_off, an = off
    x = harmonic()
    L, R = g160.input_buffer_16k_size, g160.model_return_length
    chunk = np.stack([voice_signal(L, seed=s + 1) for s in range(3)])
    fresh = engine(3, "yin")
    fresh.set_pitch_semitones(2.0)
    y_fresh, f0_fresh = conv(fresh, x), fresh.convert_f0()
    fresh.reset_state()
    c_fresh = guard(fresh.infer_batch, chunk, g160.sample_frame_16k, 0, g160.skip_head, R)
    fresh.close()
    e = engine(3, "yin")
    e.set_pitch_semitones(2.0)
    e.set_auto_transpose(220.0, 1, 12.0)
    y_on = conv(e, x)
    assert e.auto_transpose_info()["semitones"] == 12.0 and not same_bits(y_on, y_fresh)
    assert same_bits(e.convert_f0(), f0_fresh * np.float32(2.0))          # the user's semitones compose with it
    # streaming calls never read the setting, whether it is on ...
    e.reset_state()
    assert same_bits(guard(e.infer_batch, chunk, g160.sample_frame_16k, 0, g160.skip_head, R), c_fresh)
    # ... and with it off again a conversion is a fresh engine's: the factor left with the call, the semitones are as set
    e.set_auto_transpose(0.0)
    assert same_bits(conv(e, x), y_fresh) and same_bits(e.convert_f0(), f0_fresh)
    # a refused conversion behind the analysis leaves nothing behind either (a short buffer is refused in front of it, a bad geometry too)
    e.set_auto_transpose(220.0, 1, 12.0)
    with pytest.raises(RvcInferError):
        e.convert(x, k=1, context=CTX, crossfade=XF)
    e.set_auto_transpose(0.0)
    assert same_bits(conv(e, x), y_fresh)
    e.close()


def test_target_off_is_the_composition():
    e = engine(3, "rmvpe")
    x = recording()
    e.set_auto_transpose(220.0, 12, 24.0)
    e.set_auto_transpose(0.0, 12, 24.0)          # off again: the launches of the parent, the same bits
    y, _ = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=True)
    off = e.convert_info()["offsets"]
    ref, ref_off = composition(e, guard(e.highpass, x))
    assert same_bits(y, ref) and np.array_equal(off, ref_off)
    e.close()


def test_refusals_leave_the_setting():
    e = engine(1, "yin")
    e.set_auto_transpose(155.0, 12, 7.5)
    want = {"target_hz": 155.0, "step": 12, "limit": 7.5}
    for bad in ((-1.0, 1, 12.0), (20000.5, 1, 12.0), (float("nan"), 1, 12.0), (155.0, 2, 12.0), (155.0, -1, 12.0), (155.0, 1, 24.5), (155.0, 1, -0.5), (155.0, 1, float("nan"))):
        assert not S.check_auto_transpose_args(*bad)
        with pytest.raises(RvcInferError) as ei:
            e.set_auto_transpose(*bad)
        assert ei.value.kind == "NdarrayShapeError" and "auto transpose" in str(ei.value) and e.auto_transpose() == want, bad
    e.set_auto_transpose(20000.0, 0, 24.0); e.set_auto_transpose(0.0, 1, 0.0)          # the edges are legal
    e.close()
