"""Phase-vocoder crossfade and input gate (DESIGN.md "Phase-vocoder crossfade and input gate"): the numpy statements of the two definitions, their
properties, and the CPU-side layers (setters of the Python state machine, the declared entry points).  tests/test_gpu_crossfade.py imports the
definitions and the signal builders from here; nothing in this file needs a GPU."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

from obs_rvc_amd import _native
from obs_rvc_amd.geometry import derive
from obs_rvc_amd.rvc_common import CROSSFADE_LINEAR, CROSSFADE_PHASE_VOCODER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# seam lengths of the 16 / 44.1 / 48 kHz geometries (sola_buffer_frame_size = min(crossfade, 4 zc)), odd and even, and the rate each belongs to
SEAMS = [(160, 16000), (441, 44100), (640, 16000), (1764, 44100), (1920, 48000)]
NEW_ENTRY_POINTS = ["rvc_sola_step_x", "rvc_input_gate", "rvc_session_set_crossfade", "rvc_session_set_crossfade_stream",
                    "rvc_session_set_input_gate", "rvc_session_set_input_gate_stream"]


# ------------------------------------------------------------------------------------------------------------------------------
# the definitions
# ------------------------------------------------------------------------------------------------------------------------------
def windows(n, dt=np.float64):
    """fi = sin^2(pi/2 j/(n-1)), fo = 1 - fi (the linear blend's windows), win = sqrt(fo fi)"""
    x = np.linspace(0.0, 1.0, n).astype(dt)
    fi = np.sin(x * dt(0.5 * np.pi)) ** 2
    fo = 1 - fi
    return fi.astype(dt), fo.astype(dt), np.sqrt(fo * fi).astype(dt)


def pv_crossfade(a, b, dt=np.float64):
    """The blend of the saved tail `a` and the aligned new segment `b` (both length n >= 2), every step evaluated in `dt`.  With dt = float32 this
    is the naive evaluation (the phase 2 pi k j/n + d j/n + pa formed as one unreduced fp32 product) whose deviation from fp64 sets the kernel's
    tolerance."""
    n = len(a)
    cdt = np.complex128 if dt == np.float64 else np.complex64
    a, b = np.asarray(a).astype(dt), np.asarray(b).astype(dt)
    fi, fo, win = windows(n, dt)
    fa, fb = np.fft.rfft(a * win).astype(cdt), np.fft.rfft(b * win).astype(cdt)
    mag = (np.abs(fa) + np.abs(fb)).astype(dt)
    mag[1:(n // 2 if n % 2 == 0 else n // 2 + 1)] *= 2                      # every bin except DC and, n even, Nyquist
    pa = np.where(fa == 0, 0, np.angle(fa)).astype(dt)                      # atan2(0, 0) = 0
    pb = np.where(fb == 0, 0, np.angle(fb)).astype(dt)
    d = pb - pa
    d = (d - dt(2 * np.pi) * np.floor(d / dt(2 * np.pi) + dt(0.5))).astype(dt)   # [-pi, pi)
    w = (dt(2 * np.pi) * np.arange(n // 2 + 1).astype(dt) + d).astype(dt)
    t = (np.arange(n).astype(dt) / dt(n))[:, None]
    syn = np.sum(mag * np.cos(w * t + pa), axis=-1, dtype=dt)
    return (a * fo ** 2 + b * fi ** 2 + syn * win / dt(n)).astype(dt)


def linear_crossfade(a, b):
    fi, fo, _ = windows(len(a))
    return b * fi + a * fo


def input_gate(hist, chunk, zc, threshold_db):
    """-> (gated chunk, next history, open flag per 10 ms block).  hist: the 3 zc UNGATED samples before the chunk."""
    hist, chunk = np.asarray(hist, np.float64), np.asarray(chunk, np.float32)
    assert len(hist) == 3 * zc and len(chunk) % zc == 0
    x = np.concatenate([hist, chunk.astype(np.float64)])
    out = chunk.copy()
    nb = len(chunk) // zc
    is_open = np.ones(nb, bool)
    if threshold_db > -60.0:
        for i in range(nb):
            r = np.sqrt(np.mean(x[i * zc:i * zc + 4 * zc] ** 2))
            is_open[i] = not 20.0 * np.log10(max(r, 1e-5)) < threshold_db
            if not is_open[i]:
                out[i * zc:(i + 1) * zc] = 0.0
    return out, x[len(x) - 3 * zc:].astype(np.float32), is_open


def block_db(hist, chunk, zc):
    x = np.concatenate([np.asarray(hist, np.float64), np.asarray(chunk, np.float64)])
    return np.array([20.0 * np.log10(max(np.sqrt(np.mean(x[i * zc:i * zc + 4 * zc] ** 2)), 1e-5)) for i in range(len(chunk) // zc)])


# ------------------------------------------------------------------------------------------------------------------------------
# signals
# ------------------------------------------------------------------------------------------------------------------------------
def voiced(n, rate, seed, f0=220.0):
    """a voiced signal (two partials) on a broadband noise floor: without the floor some bin has |Fa| ~ 0 next to a large |Fb| and its phase is
    rounding noise at full amplitude"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(rate)
    return 0.3 * np.sin(2 * np.pi * f0 * t) + 0.2 * np.sin(2 * np.pi * 15.0 * f0 * t + 1.0) + 0.05 * rng.standard_normal(n)


def seam_case(n, rate, frame=None, seed=0, zero_tail=False, same=False):
    """One SOLA step: -> (output, sola_buffer, search, frame).  The saved tail is a stretch of the voiced signal; `output` holds a shifted (7 samples +
    whatever the search finds), scaled and re-noised copy of it, followed by more of the same signal for the frame and the next tail."""
    zc = rate // 100
    search = zc
    frame = frame if frame is not None else 2 * n
    total = n + search + frame
    rng = np.random.default_rng(1000 + seed)
    s = voiced(total + n + 64, rate, seed)
    sola = s[:n].astype(np.float32)
    lead = 5
    if same:        # the new segment IS the tail (found at `lead`)
        output = np.concatenate([0.01 * rng.standard_normal(lead), s[:n], s[n:n + total - lead - n]]).astype(np.float32)
    else:
        output = (0.9 * s[7 - lead:7 - lead + total] + 0.02 * rng.standard_normal(total)).astype(np.float32)
    if zero_tail:
        sola = np.zeros(n, np.float32)
    return output, sola, search, frame


def gate_signal(zc, blocks, levels_db, seed=0):
    """noise whose 10 ms blocks carry the given RMS levels (dB), cycled"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(zc * blocks)
    for i in range(blocks):
        seg = x[i * zc:(i + 1) * zc]
        x[i * zc:(i + 1) * zc] = seg / np.sqrt(np.mean(seg ** 2)) * 10.0 ** (levels_db[i % len(levels_db)] / 20.0)
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------
# the definition's properties
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rate", SEAMS)
def test_identical_segments_pass_unchanged(n, rate):
    a = voiced(n, rate, 3).astype(np.float32)
    assert np.abs(pv_crossfade(a, a) - a).max() < 1e-12


@pytest.mark.parametrize("n,rate", SEAMS)
def test_seam_starts_on_the_old_segment_and_ends_on_the_new_one(n, rate):
    out, sola, search, frame = seam_case(n, rate)
    b = out[5:5 + n]
    r = pv_crossfade(sola, b)
    assert abs(r[0] - sola[0]) < 1e-12 and abs(r[-1] - b[-1]) < 1e-12
    # and it is a different blend from the linear one where the two segments disagree in phase
    assert np.abs(r - linear_crossfade(sola.astype(np.float64), b.astype(np.float64))).max() > 1e-3


@pytest.mark.parametrize("n,rate", SEAMS)
def test_zero_tail_is_finite(n, rate):
    out, sola, search, frame = seam_case(n, rate, zero_tail=True)
    r = pv_crossfade(sola, out[:n])
    assert np.isfinite(r).all() and r[0] == 0.0
    # a = 0: pa = 0, d = pb, mag = 2 |Fb|: the new segment fades in with its phase run backwards to zero at the seam's start
    assert np.abs(r).max() <= 2.0 * np.abs(out[:n]).max() + 1e-9


@pytest.mark.parametrize("n,rate", SEAMS)
def test_fp32_reference_is_well_conditioned_on_the_test_inputs(n, rate):
    # the GPU test's tolerance is 2 * delta32 (the naive fp32 evaluation against fp64 on the same input); an ill-conditioned input must not be
    # able to widen it: delta32 <= 1e-4 * peak on every case the GPU test uses
    for kw in ({}, {"zero_tail": True}, {"same": True}):
        out, sola, search, frame = seam_case(n, rate, **kw)
        for off in (0, 5, search):
            b = out[off:off + n]
            r64 = pv_crossfade(sola, b)
            d32 = np.abs(pv_crossfade(sola, b, np.float32) - r64).max()
            peak = np.abs(r64).max()
            assert 0 < d32 <= 1e-4 * peak, (n, kw, off, d32, peak)


def test_phase_difference_is_wrapped_to_minus_pi_pi():
    n = 160
    fi, fo, win = windows(n)
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    pa, pb = np.angle(np.fft.rfft(a * win)), np.angle(np.fft.rfft(b * win))
    d = pb - pa
    d = d - 2 * np.pi * np.floor(d / (2 * np.pi) + 0.5)
    assert (d >= -np.pi).all() and (d < np.pi).all() and np.abs(np.exp(1j * d) - np.exp(1j * (pb - pa))).max() < 1e-12
    assert win[0] == 0.0 and win[-1] < 1e-16 and np.allclose(fo ** 2 + fi ** 2 + 2 * win ** 2, 1.0, atol=1e-15)


# ------------------------------------------------------------------------------------------------------------------------------
# the gate's definition
# ------------------------------------------------------------------------------------------------------------------------------
def test_gate_zeroes_blocks_below_the_threshold_and_keeps_the_history_ungated():
    zc = 160
    # 40 ms windows: the level of block i is that of blocks i-3 .. i together; four quiet then four loud blocks
    x = gate_signal(zc, 16, [-50.0] * 4 + [-10.0] * 4, seed=1)
    hist = np.zeros(3 * zc, np.float32)
    db = block_db(hist, x, zc)
    out, h2, is_open = input_gate(hist, x, zc, -30.0)
    assert (np.abs(db + 30.0) > 3.0).all()                      # nothing near the decision
    assert list(is_open[:8]) == [False] * 4 + [True] * 4        # the first loud block opens the gate at once (it dominates its window)
    assert list(is_open) == list(db >= -30.0)
    for i in range(16):
        blk = slice(i * zc, (i + 1) * zc)
        assert (out[blk] == (x[blk] if is_open[i] else 0)).all()
    assert (h2 == x[-3 * zc:]).all()                            # ungated, whatever was zeroed
    # chunk by chunk with the history carried = in one piece
    h, parts = hist, []
    for c in range(4):
        o, h, _ = input_gate(h, x[c * 4 * zc:(c + 1) * 4 * zc], zc, -30.0)
        parts.append(o)
    assert (np.concatenate(parts) == out).all()
    # a chunk shorter than the history
    o1, h1, _ = input_gate(hist, x[:zc], zc, -30.0)
    assert (h1[:2 * zc] == 0).all() and (h1[2 * zc:] == x[:zc]).all()


def test_gate_off_at_minus_sixty_and_below():
    zc = 441
    x = gate_signal(zc, 6, [-90.0, -70.0], seed=2)
    for thr in (-60.0, -75.0, -200.0, float("-inf")):
        out, h, is_open = input_gate(np.zeros(3 * zc, np.float32), x, zc, thr)
        assert (out == x).all() and is_open.all()
    out, _, is_open = input_gate(np.zeros(3 * zc, np.float32), x, zc, -59.0)
    assert not is_open.any() and (out == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------
# the layers above the kernels, as far as they exist without a GPU
# ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_in_every_layer():
    hdr = open(os.path.join(ROOT, "include", "rvc_mi355x.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "rvc", "src", "ffi.rs")).read()
    for name in NEW_ENTRY_POINTS:
        assert name in _native.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"pub fn %s\s*\(" % name, ffi), name
    assert re.search(r"RVC_CROSSFADE_LINEAR\s*=\s*0\s*,\s*RVC_CROSSFADE_PHASE_VOCODER\s*=\s*1", hdr)
    assert (CROSSFADE_LINEAR, CROSSFADE_PHASE_VOCODER) == (0, 1)
    assert "crossfade.hip.h" in _native.SOURCES and "rvc_session_set_crossfade" in open(os.path.join(ROOT, "examples", "c_smoke.c")).read()


class _FakeEngine:
    """records what the Python state machine asks of its engine"""

    def __init__(self, zc):
        self.zc, self.calls = zc, []

    def input_gate(self, hist, chunk, sample_rate, threshold_db):
        self.calls.append(("gate", threshold_db))
        out, h, _ = input_gate(hist, chunk, sample_rate // 100, threshold_db)
        return out, h

    def sola_step(self, output, sola_buffer, search, frame, **kw):
        self.calls.append(("sola", kw))
        return 0, np.array(output[:frame], np.float32), np.array(output[frame:frame + len(sola_buffer)], np.float32)


def test_python_state_machine_forwards_both_settings():
    from obs_rvc_amd.streaming import StreamingSession
    g = derive(16000, 0.16, 0.07, 0.5, 16000)
    e = _FakeEngine(g.zc)
    s = StreamingSession(e, g, 12, 1.0, None, None, skip_inference=True)
    x = gate_signal(g.zc, g.sample_frame_size // g.zc, [-10.0], seed=3)
    s.process_one_frame(x, x)
    assert e.calls == [("sola", {})]                     # defaults: the engine is called exactly as before
    s.set_crossfade(CROSSFADE_PHASE_VOCODER); s.set_input_gate(-30.0)
    s.process_one_frame(x, x)
    assert e.calls[1:] == [("gate", -30.0), ("sola", {"crossfade": CROSSFADE_PHASE_VOCODER})]
    assert (s.gate_hist == x[-3 * g.zc:]).all()
    s.set_crossfade(CROSSFADE_LINEAR, stream=0); s.set_input_gate(-60.0, stream=0)
    s.process_one_frame(x, x)
    assert e.calls[3:] == [("gate", -60.0), ("sola", {})]     # the history stays current once the gate has been used
    for bad in (lambda: s.set_crossfade(2), lambda: s.set_crossfade(1, stream=1), lambda: s.set_input_gate(float("nan")),
                lambda: s.set_input_gate(-30.0, stream=3)):
        with pytest.raises(ValueError):
            bad()
