"""Phase-vocoder crossfade and input gate on the GPU (DESIGN.md "Phase-vocoder crossfade and input gate"): the kernels against the fp64 numpy
definitions of tests/test_crossfade.py, every stream of a batched session against its own single-stream run, the native session against the
Python state machine, the error paths."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from common import voice_signal, zoo
from obs_rvc_amd.geometry import derive
from obs_rvc_amd.rvc_common import CROSSFADE_LINEAR as LIN, CROSSFADE_PHASE_VOCODER as PV, RvcInferError
from test_crossfade import SEAMS, block_db, gate_signal, input_gate, pv_crossfade, seam_case

pytestmark = pytest.mark.gpu
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def eng():
    from obs_rvc_amd.rvc import RvcInfer
    return RvcInfer(zoo("tiny")["data"])


def _bound(sola, b):
    """-> (fp64 definition, delta32 = what the naive fp32 evaluation of the definition deviates from it, peak); the kernel gets 2 * delta32"""
    r64 = pv_crossfade(sola, b)
    d32 = float(np.abs(pv_crossfade(sola, b, np.float32) - r64).max())
    peak = float(np.abs(r64).max())
    assert d32 <= 1e-4 * peak, (d32, peak)          # an ill-conditioned input must not widen its own tolerance
    return r64, d32, peak


def _check_step(eng, output, sola, search, frame, tag):
    """one step in both modes -> (offset, seam written by the kernel, definition, delta32, peak); everything but the seam must be the linear step's bits"""
    n = len(sola)
    off_l, fr_l, sb_l, out_l = eng.sola_step_full(output, sola, search, frame)
    off, fr, sb, out = eng.sola_step_full(output, sola, search, frame, PV)
    assert off == off_l
    b = output[off:off + n]
    r64, d32, peak = _bound(sola, b)
    seam = out[off:off + n]
    err = float(np.abs(seam - r64).max())
    print("%s n=%d off=%d delta32=%.3e kernel=%.3e (%.2f x delta32) peak=%.3f" % (tag, n, off, d32, err, err / d32, peak))
    assert np.isfinite(out).all() and err <= 2.0 * d32, (tag, n, err, d32)
    assert (out[:off] == output[:off]).all() and (out[off + n:] == output[off + n:]).all()      # untouched outside the seam ...
    assert (out_l[:off] == out[:off]).all() and (out_l[off + n:] == out[off + n:]).all()        # ... as in the linear step
    # frame and saved tail are slices of the blended output, exactly as in the linear step
    assert (fr == out[off:off + frame]).all() and (sb == out[off + frame:off + frame + n]).all()
    assert (fr_l == out_l[off:off + frame]).all() and (sb_l == out_l[off + frame:off + frame + n]).all()
    return off, seam, r64, d32, peak


@pytest.mark.parametrize("n,rate", SEAMS)
def test_kernel_matches_the_definition(eng, n, rate):
    output, sola, search, frame = seam_case(n, rate)
    off, seam, r64, d32, peak = _check_step(eng, output, sola, search, frame, "definition")
    assert frame >= n       # the frame behind the seam and the new tail lie outside it: bitwise the linear step's (checked in _check_step)
    # end samples: the seam starts on the old tail and ends on the new segment
    assert abs(seam[0] - sola[0]) <= 1e-6 * peak and abs(seam[-1] - output[off + n - 1]) <= 1e-6 * peak


def test_frame_shorter_than_the_seam(eng):
    # the saved tail then overlaps the seam: it must hold the blended samples, as the linear step's does
    output, sola, search, frame = seam_case(640, 16000, frame=320)
    _check_step(eng, output, sola, search, frame, "short-frame")


@pytest.mark.parametrize("n,rate", SEAMS)
def test_properties(eng, n, rate):
    # a == b returns a
    output, sola, search, frame = seam_case(n, rate, same=True)
    off, seam, r64, d32, peak = _check_step(eng, output, sola, search, frame, "same")
    assert off == 5 and (output[off:off + n] == sola).all()
    assert np.abs(seam - sola).max() <= 2.0 * d32
    assert abs(seam[0] - sola[0]) <= 1e-6 * peak and abs(seam[-1] - sola[-1]) <= 1e-6 * peak
    # an all-zero tail (the first chunk of every session): finite and equal to the definition
    output, sola, search, frame = seam_case(n, rate, zero_tail=True)
    off, seam, r64, d32, peak = _check_step(eng, output, sola, search, frame, "zero-tail")
    assert seam[0] == 0.0


def test_linear_mode_of_the_extended_step_is_the_plain_step(eng):
    L = eng._L
    for n, rate in SEAMS:
        output, sola, search, frame = seam_case(n, rate)
        off_l, fr_l, sb_l, out_l = eng.sola_step_full(output, sola, search, frame)
        o, sb, fr, off = output.copy(), sola.copy(), np.empty(frame, np.float32), C.c_size_t()
        assert L.rvc_sola_step_x(eng._h, o.ctypes.data_as(FP), len(o), sb.ctypes.data_as(FP), len(sb), search, frame, fr.ctypes.data_as(FP), C.byref(off), LIN) == 0
        assert off.value == off_l and (o == out_l).all() and (sb == sb_l).all() and (fr == fr_l).all()
    # a seam of one sample has nothing to analyse: linear blend in both modes
    output = voice_signal(400, seed=1)
    r0, r1 = eng.sola_step_full(output, output[:1], 160, 200), eng.sola_step_full(output, output[:1], 160, 200, PV)
    assert r0[0] == r1[0] and all((x == y).all() for x, y in zip(r0[1:], r1[1:]))


# ------------------------------------------------------------------------------------------------------------------------------
# sessions
# ------------------------------------------------------------------------------------------------------------------------------
def _pass_through(streams):
    from obs_rvc_amd.rvc import RvcInfer
    from obs_rvc_amd.streaming import NativeStreamingSession
    e = RvcInfer(zoo("tiny")["data"])
    if streams > 1:
        e.set_streams(streams)
    return e, (lambda: NativeStreamingSession(e, 48000, 0.16, 0.07, 0.5, 40000, 12, 1.0, skip_inference=True))


def _stream_audio(S, F, chunks):
    # per stream its own voice with its own slow level change, so that offsets differ between streams and chunks
    return np.stack([np.interp(np.arange(F * chunks) / 48000.0, np.arange(F * chunks // 3 + 8) / 16000.0,
                               voice_signal(F * chunks // 3 + 8, seed=100 + s)).astype(np.float32) * np.float32(0.5 + 0.5 * (s % 5) / 4) for s in range(S)])


@pytest.mark.parametrize("S", [17, 64])
def test_every_stream_of_a_mixed_session_equals_its_own_run(S):
    chunks = 8
    eb, mk = _pass_through(S)
    mixed, linear = mk(), mk()
    assert mixed.sola_buffer_frame_size == 1920
    modes = [PV if s % 3 else LIN for s in range(S)]
    for s, m in enumerate(modes):
        mixed.set_crossfade(m, stream=s)
    F = mixed.sample_frame_size
    audio = _stream_audio(S, F, chunks)
    ys, offs, offs_lin = [], [], []
    for c in range(chunks):
        x = audio[:, c * F:(c + 1) * F]
        ys.append(mixed.process_one_frame(x).copy()); offs.append(list(mixed.last_sola_offsets))
        yl = linear.process_one_frame(x); offs_lin.append(list(linear.last_sola_offsets))
        for s in range(S):
            if modes[s] == LIN:
                assert (ys[-1][s] == yl[s]).all(), (c, s)          # linear streams: the bits of a session that never heard of the setting
    # the saved tail is taken from the unblended output: the offsets do not depend on the blend
    assert offs == offs_lin and len({tuple(o) for o in offs}) > 1
    e1, mk1 = _pass_through(1)
    for s in range(S):                   # EVERY stream against its own single-stream session: the arithmetic per stream does not depend on the batch
        one = mk1()
        one.set_crossfade(modes[s])
        for c in range(chunks):
            y1 = one.process_one_frame(audio[s, c * F:(c + 1) * F])
            assert (y1 == ys[c][s]).all() and one.last_sola_offset == offs[c][s], (s, c)
    # and the phase-vocoder streams do differ from the linear blend
    lin2 = mk()
    differs = 0
    for c in range(chunks):
        yl = lin2.process_one_frame(audio[:, c * F:(c + 1) * F])
        differs += sum(bool((yl[s] != ys[c][s]).any()) for s in range(S) if modes[s] == PV)
    assert differs > 0


def test_native_session_matches_python_state_machine_with_both_stages():
    from obs_rvc_amd.resample import FftFixedInOut
    from obs_rvc_amd.rvc import RvcInfer
    from obs_rvc_amd.streaming import NativeStreamingSession, StreamingSession
    g = derive(48000, 0.16, 0.07, 2.0, 4800)
    z = zoo("tiny")

    def engine():
        e = RvcInfer(z["data"]); e.load_contentvec(2); e.load_f0(); e.load_model(z["model"]); e.set_noise_seed(3, 0)
        return e
    e1, e2 = engine(), engine()
    nat = NativeStreamingSession(e1, 48000, 0.16, 0.07, 2.0, 4800, 12, 0.6)
    pys = StreamingSession(e2, g, 12, 0.6, 4800, lambda ri, ro, n: FftFixedInOut(e2, ri, ro, n))
    for s in (nat, pys):
        s.set_crossfade(PV); s.set_input_gate(-35.0)
    F = 7680
    a = np.interp(np.arange(F * 8) / 48000.0, np.arange(2560 * 8) / 16000.0, voice_signal(2560 * 8, seed=10)).astype(np.float32)
    a[F + 480:F + 480 * 9] *= np.float32(1e-3)          # 80 ms far below the threshold inside the second chunk, the rest far above it
    a[3 * F:3 * F + 480 * 6] *= np.float32(1e-3)
    for c in range(8):
        ch = a[c * F:(c + 1) * F]
        fn, fp = nat.process_one_frame(ch), pys.process_one_frame(ch)
        assert fn.shape == (F,) and nat.last_sola_offset == pys.last_sola_offset, c
        err = float(np.abs(fn - fp).max())
        print("chunk %d offset %d native-vs-python %.3e" % (c, nat.last_sola_offset, err))
        assert err < 2e-5, (c, err)       # the bound tests/test_postprocess.py uses for the same pair of chains
    assert (pys.gate_hist == a[8 * F - 3 * 480:8 * F]).all()
    # the gate did act on what the model saw: the host-rate ring of the Python chain holds zeros where the quiet stretches were
    ring = pys.input_buffer[-8 * F:]
    assert len(ring) == 8 * F and (ring[F + 480 * 4:F + 480 * 9] == 0).all() and (ring[F + 480 * 9:F + 480 * 10] == a[F + 480 * 9:F + 480 * 10]).all()


def test_input_gate_matches_the_definition(eng):
    for rate, thr in ((16000, -30.0), (44100, -25.0), (48000, -40.0)):
        zc = rate // 100
        # blocks alternate in runs of four (the level of a block is that of its 40 ms window) between 15 dB above and 15 dB below the threshold
        x = gate_signal(zc, 24, [thr - 15.0] * 4 + [thr + 15.0] * 4, seed=rate)
        hist = gate_signal(zc, 3, [thr - 15.0], seed=rate + 1)
        db = block_db(hist, x, zc)
        assert (np.abs(db - thr) >= 3.0).all() and (db < thr).any() and (db > thr).any()       # nothing near the decision
        ref, h_ref, is_open = input_gate(hist, x, zc, thr)
        out, h = eng.input_gate(hist, x, rate, thr)
        assert (out == ref).all() and (h == h_ref).all()               # the zeroed set matches, passed samples bit for bit
        assert (h == x[-3 * zc:]).all()
        # chunk by chunk, history carried: the loud block after gated ones opens the gate at the block the definition names
        hh, parts = hist, []
        for c in range(6):
            o, hh = eng.input_gate(hh, x[c * 4 * zc:(c + 1) * 4 * zc], rate, thr)
            parts.append(o)
        got = np.concatenate(parts)
        assert (got == ref).all()
        first_open = int(np.argmax(is_open))
        assert first_open == 4 and (got[:4 * zc] == 0).all() and (got[4 * zc:5 * zc] == x[4 * zc:5 * zc]).all()
        # off: bit for bit
        for off_thr in (-60.0, -90.0):
            o, hh = eng.input_gate(hist, x, rate, off_thr)
            assert (o == x).all() and (hh == x[-3 * zc:]).all()


def test_session_gate(eng):
    e, mk = _pass_through(3)
    plain, gate, off, pre = mk(), mk(), mk(), mk()
    F, zc, thr = plain.sample_frame_size, 480, -30.0
    gate.set_input_gate(thr, stream=0); gate.set_input_gate(thr, stream=2)      # stream 1 stays off
    off.set_input_gate(-60.0)
    chunks = 6
    x = np.stack([gate_signal(zc, chunks * F // zc, [thr - 15.0] * 4 + [thr + 15.0] * 4 + [thr + 15.0, thr - 15.0] * 2, seed=7 + s) for s in range(3)])
    # the definition, chunk by chunk with the ungated history carried, applied on the host in front of a session without a gate
    hist = [np.zeros(3 * zc, np.float32) for _ in range(3)]
    n_zero = 0
    for c in range(chunks):
        ch = x[:, c * F:(c + 1) * F]
        ref = ch.copy()
        for s in (0, 2):
            ref[s], hist[s], is_open = input_gate(hist[s], ch[s], zc, thr)
            n_zero += int((~is_open).sum())
        y_gate, y_pre, y_plain, y_off = gate.process_one_frame(ch), pre.process_one_frame(ref), plain.process_one_frame(ch), off.process_one_frame(ch)
        assert (y_gate == y_pre).all() and gate.last_sola_offsets == pre.last_sola_offsets, c
        assert (y_off == y_plain).all() and (y_gate[1] == y_plain[1]).all(), c     # threshold -60 / a stream with the gate off: the bits of a session that never called the setter
    assert n_zero > 10 and (y_gate[0] != y_plain[0]).any()


def test_errors_leave_the_session_working(eng):
    e, mk = _pass_through(2)
    s = mk()
    L, h = s._L, s._h
    x = _stream_audio(2, s.sample_frame_size, 1)
    y0 = s.process_one_frame(x)
    for call in (lambda: s.set_crossfade(2), lambda: s.set_crossfade(-1), lambda: s.set_crossfade(PV, stream=2), lambda: s.set_crossfade(PV, stream=-1),
                 lambda: s.set_input_gate(float("nan")), lambda: s.set_input_gate(-30.0, stream=2), lambda: s.set_input_gate(float("nan"), stream=0)):
        with pytest.raises(RvcInferError) as ei:
            call()
        assert ei.value.code == 5 and len(str(ei.value)) > len("NdarrayShapeError: ") + 8, str(ei.value)      # the shape error, with a message
    assert L.rvc_session_set_crossfade(h, 7) == 5 and b"crossfade" in L.rvc_last_error_message(e._h)
    assert L.rvc_session_set_input_gate_stream(h, 9, -30.0) == 5 and b"stream" in L.rvc_last_error_message(e._h)
    y1 = s.process_one_frame(x)
    assert y1.shape == y0.shape and np.isfinite(y1).all()
    # the caller-side forms
    output, sola, search, frame = seam_case(160, 16000)
    with pytest.raises(RvcInferError):
        eng.sola_step(output, sola, search, frame, crossfade=3)
    with pytest.raises(RvcInferError):
        eng.input_gate(np.zeros(480, np.float32), np.zeros(1600, np.float32), 16000, float("nan"))
    with pytest.raises(RvcInferError):
        eng.input_gate(np.zeros(480, np.float32), np.zeros(1601, np.float32), 16000, -30.0)     # not a whole number of blocks
    big = np.zeros(3 * 5000, np.float32)
    with pytest.raises(RvcInferError):
        eng.sola_step(big, big[:5000], 100, 5000, crossfade=PV)                               # a seam beyond the kernels' 4096 samples
    assert eng.sola_step(output, sola, search, frame, crossfade=PV)[0] == eng.sola_step(output, sola, search, frame)[0]
