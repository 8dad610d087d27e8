"""Spectral-gate noise reduction on the GPU (DESIGN.md "Spectral-gate noise reduction"): the kernels against the fp64 numpy definition of
tests/denoise_ref.py, state carried across calls, every stream of a batch against its own run, the error paths, and both sides inside the session.

Tolerance of every value check: max-abs <= 2 * delta32 of that input, delta32 being the deviation of the definition evaluated naively in numpy fp32
(unreduced phase) from fp64, with delta32 <= 1e-4 * peak asserted (denoise_ref.bound) so that an input cannot widen its own tolerance.  The session
with a model is judged by the bound the existing native-vs-Python session tests use (2e-5).

Measured on an MI355X (max-abs deviation from fp64 / delta32, worst stream of the call): see DESIGN.md "Spectral-gate noise reduction"."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from common import zoo
from denoise_ref import CASES, SESSION_INPUTS, SHAPES, bound, case_batch, denoise, voiced
from obs_rvc_amd.rvc_common import DENOISE_INPUT, DENOISE_OUTPUT, RvcInferError

pytestmark = pytest.mark.gpu
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def eng():
    from obs_rvc_amd.rvc import RvcInfer
    return RvcInfer(zoo("tiny")["data"])


def _denoiser(eng, rate, streams=1):
    from obs_rvc_amd.denoise import Denoiser
    return Denoiser(eng, rate, streams)


def _case_denoiser(eng, rate):
    d = _denoiser(eng, rate, len(CASES))
    for i, (_, strength, thr) in enumerate(CASES):
        d.set(strength, thr, stream=i)
    return d


@pytest.mark.parametrize("rate,hops", SHAPES)
def test_kernels_match_the_definition(eng, rate, hops):
    x = case_batch(rate, hops)
    d = _case_denoiser(eng, rate)
    assert d.latency == rate // 100
    y = d.process(x)
    assert y.shape == x.shape and y.dtype == np.float32 and np.isfinite(y).all()
    for i, (kind, strength, thr) in enumerate(CASES):
        r64, d32, peak = bound(x[i], rate, strength, thr)
        err = float(np.abs(y[i] - r64).max())
        print("definition %d Hz N=%d hops=%d %s strength %.1f threshold %.1f: delta32=%.3e kernel=%.3e (%.3f x delta32) peak=%.3f"
              % (rate, rate // 50, hops, kind, strength, thr, d32, err, err / d32, peak))
        assert err <= 2.0 * d32, (rate, kind, strength, thr, err, d32)


def test_state_is_carried_across_calls_and_reset(eng):
    rate, zc = 8000, 80
    x = case_batch(rate, 12)
    d = _case_denoiser(eng, rate)
    one = d.process(x)
    for i, (kind, strength, thr) in enumerate(CASES):                   # twelve frames: the mask has left its all-open start
        r64, d32, peak = bound(x[i], rate, strength, thr)
        err = float(np.abs(one[i] - r64).max())
        print("12 hops at 8 kHz, %s strength %.1f threshold %.1f: delta32=%.3e kernel=%.3e (%.3f x delta32)" % (kind, strength, thr, d32, err, err / d32))
        assert err <= 2.0 * d32, (kind, strength, thr, err, d32)
    d.reset()
    again = d.process(x)
    assert (again == one).all()                                          # reset + the same input: the first run, bit for bit
    d.reset()
    cut = np.concatenate([d.process(x[:, :3 * zc]), d.process(x[:, 3 * zc:7 * zc]), d.process(x[:, 7 * zc:])], axis=1)
    assert (cut == one).all()                                            # 3 + 4 + 5 hops = 12 hops in one call, bit for bit


def test_every_stream_of_a_batch_equals_its_own_run(eng):
    rate, hops = 44100, 5
    zc = rate // 100
    settings = [(1.0, 2.0), (0.0, 2.0), (0.6, 0.5)]
    x = np.stack([voiced(hops * zc, rate, 20 + s) for s in range(3)])
    d = _denoiser(eng, rate, 3)
    for s, (strength, thr) in enumerate(settings):
        d.set(strength, thr, stream=s)
    yb = np.concatenate([d.process(x[:, :2 * zc]), d.process(x[:, 2 * zc:])], axis=1)
    assert (yb[1] == x[1]).all()                                         # strength 0: the input, bit for bit and undelayed
    for s, (strength, thr) in enumerate(settings):
        one = _denoiser(eng, rate, 1)
        one.set(strength, thr)
        y1 = np.concatenate([one.process(x[s, :2 * zc]), one.process(x[s, 2 * zc:])])
        assert (y1 == yb[s]).all(), s
    assert (yb[0] != x[0]).any() and (yb[2] != x[2]).any()
    # a stream that was off keeps its (zero) state: switched on later it starts like a fresh denoiser
    d.set(0.6, 0.5, stream=1)
    fresh = _denoiser(eng, rate, 1)
    fresh.set(0.6, 0.5)
    assert (d.process(x)[1] == fresh.process(x[1])).all()


def test_argument_errors(eng):
    L = eng._L
    d = _denoiser(eng, 16000, 2)
    x = np.zeros((2, 320), np.float32)

    def shape_error(call):
        with pytest.raises(RvcInferError) as ei:
            call()
        assert ei.value.code == 5 and len(str(ei.value)) > len("NdarrayShapeError: ") + 8, str(ei.value)
        assert len(L.rvc_last_error_message(eng._h) or b"") > 8
    shape_error(lambda: d.process(np.zeros((2, 161), np.float32)))          # n is no multiple of zc
    shape_error(lambda: _denoiser(eng, 22050 + 1))                           # the sample rate is no multiple of 100
    shape_error(lambda: _denoiser(eng, 200000))                              # a frame beyond the kernels' 3 840 samples
    shape_error(lambda: d.set(float("nan")))
    shape_error(lambda: d.set(1.5))
    shape_error(lambda: d.set(0.5, 17.0))
    shape_error(lambda: d.set(0.5, float("nan")))
    shape_error(lambda: d.set(0.5, 2.0, stream=2))
    shape_error(lambda: d.set(0.5, 2.0, stream=-2))
    out = np.empty_like(x)
    assert L.rvc_denoiser_process(d._h, x.ctypes.data_as(FP), 0, out.ctypes.data_as(FP)) == 5 and b"multiple" in L.rvc_last_error_message(eng._h)
    assert L.rvc_denoiser_set(d._h, 5, 0.5, 2.0) == 5 and b"stream" in L.rvc_last_error_message(eng._h)
    # the errors left the denoiser working and its settings alone (both streams still off)
    assert (d.process(x + np.float32(0.25)) == x + np.float32(0.25)).all()


# ------------------------------------------------------------------------------------------------------------------------------
# sessions
# ------------------------------------------------------------------------------------------------------------------------------
def _pass_through(rate, streams=2):
    from obs_rvc_amd.rvc import RvcInfer
    from obs_rvc_amd.streaming import NativeStreamingSession
    e = RvcInfer(zoo("tiny")["data"])
    e.set_streams(streams)
    return e, (lambda: NativeStreamingSession(e, rate, 0.16, 0.07, 0.5, 40000, 12, 1.0, skip_inference=True))


@pytest.mark.parametrize("rate", [16000, 44100])
def test_session_pass_through(rate):
    chunks, strength, thr = 4, 1.0, 2.0
    e, mk = _pass_through(rate)
    plain, untouched, zero, s_in, s_out, pre = mk(), mk(), mk(), mk(), mk(), mk()
    F = plain.sample_frame_size
    zero.set_noise_reduction(DENOISE_INPUT, 0.0); zero.set_noise_reduction(DENOISE_OUTPUT, 0.0, 3.0); zero.set_noise_reduction(DENOISE_OUTPUT, 0.0, stream=1)
    s_in.set_noise_reduction(DENOISE_INPUT, strength, thr, stream=1)
    s_out.set_noise_reduction(DENOISE_OUTPUT, strength, thr, stream=1)
    assert (rate, F, chunks, 41) in SESSION_INPUTS                       # (tests/test_denoise_ref.py checks the conditioning of stream 1's signal without a GPU)
    x = np.stack([voiced(chunks * F, rate, 40 + s) for s in range(2)])
    r64, d32, peak = bound(x[1], rate, strength, thr)                    # the input side's reference: the denoised signal of stream 1
    x_pre = np.stack([x[0], r64.astype(np.float32)])
    frames = {k: [] for k in ("plain", "in", "out", "pre")}
    for c in range(chunks):
        ch = x[:, c * F:(c + 1) * F]
        y = plain.process_one_frame(ch)
        assert (untouched.process_one_frame(ch) == y).all() and (zero.process_one_frame(ch) == y).all(), c      # never switched on: the parent's bits
        frames["plain"].append(y.copy())
        frames["in"].append(s_in.process_one_frame(ch).copy()); off_in = list(s_in.last_sola_offsets)
        frames["out"].append(s_out.process_one_frame(ch).copy())
        assert s_out.last_sola_offsets == plain.last_sola_offsets, c     # the output side sits behind the offset search
        frames["pre"].append(pre.process_one_frame(x_pre[:, c * F:(c + 1) * F]).copy())
        assert off_in == pre.last_sola_offsets, c
    fr = {k: np.concatenate(v, axis=1) for k, v in frames.items()}
    assert (fr["in"][0] == fr["plain"][0]).all() and (fr["out"][0] == fr["plain"][0]).all()      # the stream at strength 0 keeps its bits
    err_in = float(np.abs(fr["in"][1].astype(np.float64) - fr["pre"][1]).max())
    # the output side: the definition applied to the frames the plain session returned
    o64, od32, opeak = bound(fr["plain"][1], rate, strength, thr)
    err_out = float(np.abs(fr["out"][1] - o64).max())
    print("session %d Hz: input side delta32=%.3e kernel chain=%.3e (%.3f x); output side delta32=%.3e kernel=%.3e (%.3f x)"
          % (rate, d32, err_in, err_in / d32, od32, err_out, err_out / od32))
    assert err_in <= 2.0 * d32 and err_out <= 2.0 * od32
    assert (fr["in"][1] != fr["plain"][1]).any() and (fr["out"][1] != fr["plain"][1]).any()
    # delay and state survive set_params; back at strength 0 the stream passes undelayed again
    s_out.set_params(12, 1.0)
    s_out.set_noise_reduction(DENOISE_OUTPUT, 0.0, stream=1)
    ch = x[:, :F]
    assert (s_out.process_one_frame(ch) == plain.process_one_frame(ch)).all()
    for bad in (lambda: s_in.set_noise_reduction(2, 0.5), lambda: s_in.set_noise_reduction(DENOISE_INPUT, float("nan")),
                lambda: s_in.set_noise_reduction(DENOISE_INPUT, 0.5, 17.0), lambda: s_in.set_noise_reduction(DENOISE_OUTPUT, 0.5, stream=2)):
        with pytest.raises(RvcInferError) as ei:
            bad()
        assert ei.value.code == 5 and len(str(ei.value)) > len("NdarrayShapeError: ") + 8, str(ei.value)


def test_session_with_a_model_both_sides():
    from obs_rvc_amd.rvc import RvcInfer
    from obs_rvc_amd.streaming import NativeStreamingSession
    z = zoo("tiny")

    def engine():
        e = RvcInfer(z["data"]); e.load_contentvec(2); e.load_f0(); e.load_model(z["model"]); e.set_noise_seed(3, 0)
        return e
    e1, e2 = engine(), engine()
    rate, chunks, strength, thr = 48000, 3, 1.0, 2.0
    both = NativeStreamingSession(e1, rate, 0.16, 0.07, 2.0, 4800, 12, 0.6)
    plain = NativeStreamingSession(e2, rate, 0.16, 0.07, 2.0, 4800, 12, 0.6)
    both.set_noise_reduction(DENOISE_INPUT, strength, thr); both.set_noise_reduction(DENOISE_OUTPUT, strength, thr)
    F = both.sample_frame_size
    assert (rate, F, chunks, 60) in SESSION_INPUTS
    x = voiced(chunks * F, rate, 60)
    x_pre = denoise(x, rate, strength, thr).astype(np.float32)          # the input side's definition, on the host in front of a session without the feature
    got, ref_in, offs = [], [], []
    for c in range(chunks):
        got.append(both.process_one_frame(x[c * F:(c + 1) * F]).copy())
        ref_in.append(plain.process_one_frame(x_pre[c * F:(c + 1) * F]).copy())
        offs.append((both.last_sola_offset, plain.last_sola_offset))
    got, ref_in = np.concatenate(got), np.concatenate(ref_in)
    assert got.shape == (chunks * F,) and np.isfinite(got).all()
    assert all(a == b for a, b in offs), offs
    want = denoise(ref_in, rate, strength, thr)                          # the output side's definition on that session's own frames
    err = float(np.abs(got - want).max())
    print("model session, both sides: max-abs deviation %.3e (peak %.3f)" % (err, float(np.abs(want).max())))
    assert err < 2e-5, err                                               # the bound of the native-vs-Python session tests
