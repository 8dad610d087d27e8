"""The pitch controls of DESIGN.md "Pitch controls" restated in numpy from the definition: multiplier, range gate, median filter
(scipy.signal.medfilt, which is what upstream calls), scale snap.  dtype = float64 is the reference of tests/test_gpu_f0cond.py; dtype = float32 runs
the same recipe in single precision (what fp32 costs: that test derives its bound from it).  Also here: the inputs and the settings the GPU tests
use, so that tests/test_f0cond_ref.py can show on the CPU that none of them puts a row on a decision boundary."""
import numpy as np
from scipy.signal import medfilt

import yin_ref as Y

SCALE_CHROMATIC, SCALE_C_MAJOR = 0xFFF, 0xAB5
NEUTRAL = dict(st=0.0, lo=0.0, hi=np.inf, r=0, mask=0, s=0.0)
SNAP_MARGIN, GATE_MARGIN = 1e-3, 1e-4          # semitones; relative


def multiplier(pitch_shift=0, st=0.0, formant=None):
    """step 1: the float32 factor the rows are multiplied by: the octave factor (exact), times (float)2^(-phi / 12) on infer calls (formant = phi,
    None on rvc_pitch), times (float)2^(st / 12) unless st = 0; products rounded to float32"""
    up = np.float32(Y.uppower(pitch_shift))
    if formant is not None:
        up = np.float32(up * np.float32(2.0 ** (-formant / 12.0)))
    if st != 0.0:
        up = np.float32(up * np.float32(2.0 ** (st / 12.0)))
    return up


def allowed_notes(mask, lo, hi):
    return np.array([k for k in range(int(lo), int(hi) + 1) if (mask >> (k % 12)) & 1], dtype=np.int64)


def snap(f, mask, s, dtype=np.float64):
    """step 4 on an array of rows -> (rows, margin in semitones: the distance of n to the nearest midpoint between two allowed notes; 1 on unvoiced rows)"""
    dt = np.dtype(dtype).type
    f = np.asarray(f, dtype)
    out, margin = f.copy(), np.ones(len(f))
    if mask == 0 or s == 0:
        return out, margin
    for i, v in enumerate(f):
        if not v > 0:
            continue
        n = dt(69) + dt(12) * np.log2(v / dt(440))
        notes = allowed_notes(mask, np.floor(n) - 12, np.floor(n) + 13)
        target = notes[np.argmin(np.abs(notes.astype(dtype) - n))]          # argmin takes the first of two equal distances: the lower note
        out[i] = v * np.exp2(dt(s) * (dt(target) - n) / dt(12))
        mids = 0.5 * (notes[:-1] + notes[1:])
        margin[i] = np.min(np.abs(mids - float(n)))
    return out, margin


def gate(f, lo, hi):
    """step 2 -> (rows, margin: the relative distance of a voiced row to lo / hi; 1 on unvoiced rows and with the gate off)"""
    f = np.asarray(f)
    out, margin = f.copy(), np.ones(len(f))
    v = f > 0
    out[v & ((f < lo) | (f > hi))] = 0
    fv = f[v].astype(np.float64)
    m = np.ones(len(fv))
    if lo > 0:
        m = np.minimum(m, np.abs(fv - lo) / lo)
    if np.isfinite(hi):
        m = np.minimum(m, np.abs(fv - hi) / hi)
    margin[v] = m
    return out, margin


def window_min(m, r):
    """a per-row margin seen through the median window: the smallest over rows [i - r, i + r]"""
    m = np.asarray(m, np.float64)
    p = np.concatenate([np.ones(r), m, np.ones(r)])
    return np.array([p[i:i + 2 * r + 1].min() for i in range(len(m))])


def condition(f0, up=1.0, lo=0.0, hi=np.inf, r=0, mask=0, s=0.0, st=None, dtype=np.float64, parts=False):
    """steps 1-4 on the rows f0 [Tm] (Hz, 0 = unvoiced); up = multiplier(...) -> (conditioned rows, decision margin per row).  The margin is the smallest
    of the snap margin (semitones) and the gate margin (relative) of the rows in the row's median window, 1 where neither applies; parts = True
    returns the two separately as well.  (st is accepted and ignored so that a settings dict can be passed whole: it is part of `up`.)"""
    f = np.asarray(f0, dtype) * np.dtype(dtype).type(up)
    f, gm = gate(f, lo, hi)
    if r > 0:
        f = medfilt(f, 2 * r + 1)
        gm = window_min(gm, r)
    f, sm = snap(f, mask, s, dtype)
    margin = np.minimum(gm, sm)
    return (f, margin, gm, sm) if parts else (f, margin)


# ---- what tests/test_gpu_f0cond.py runs: inputs (6000 samples at 16 kHz, the f0 window is the last 4960: 32 rows) and settings ----
def glide_signal(n=6000, lo_hz=131.5, hi_hz=246.0, seed=2):
    """five partials gliding slowly from lo_hz to hi_hz over the whole buffer, on a 1e-3 noise floor: every row voiced, eleven semitones crossed"""
    rng = np.random.default_rng(seed)
    f = lo_hz * (hi_hz / lo_hz) ** np.linspace(0.0, 1.0, n)
    ph = 2.0 * np.pi * np.cumsum(f) / Y.SR
    return (0.2 * sum(np.sin(k * ph) / k for k in range(1, 6)) + 1e-3 * rng.standard_normal(n)).astype(np.float32)


def inputs():
    return {"composite": Y.composite_signal(), "glide": glide_signal()}


CASES = {
    "median1": dict(NEUTRAL, r=1),
    "median3": dict(NEUTRAL, r=3),
    "median7": dict(NEUTRAL, r=7),
    "gate": dict(NEUTRAL, lo=170.0, hi=210.0),
    "chromatic": dict(NEUTRAL, mask=SCALE_CHROMATIC, s=1.0),
    "cmajor": dict(NEUTRAL, mask=SCALE_C_MAJOR, s=1.0),
    "cmajor_half": dict(NEUTRAL, mask=SCALE_C_MAJOR, s=0.5),
    "only_a": dict(NEUTRAL, mask=1 << 9, s=1.0),
    "stream1": dict(NEUTRAL, r=3, mask=SCALE_C_MAJOR, s=0.7),
    "stream2": dict(NEUTRAL, st=-5.0, lo=60.0, hi=340.0),           # with pitch_shift = 12
    "changed": dict(NEUTRAL, st=3.0, r=3, mask=SCALE_C_MAJOR, s=0.7),          # set before the second chunk, with pitch_shift = 12
    "session": dict(NEUTRAL, st=4.0, mask=SCALE_CHROMATIC, s=1.0),
}
# (input, case) pairs of the rvc_pitch tests; the multi-stream and session tests build their chunks from tests/common.py voice_signal and are
# checked in tests/test_f0cond_ref.py the same way
PITCH_CASES = [(i, c) for i in ("composite", "glide") for c in ("median1", "median3", "median7", "gate", "chromatic", "cmajor", "cmajor_half", "only_a")]


def settings(case):
    c = CASES[case]
    return {k: c[k] for k in ("lo", "hi", "r", "mask", "s")}


def stream_chunks():      # (STREAM_SEEDS, STREAM_CASES: below)
    """the two chunks of the three streams of the per-stream test: [chunk][stream][samples]; the interior stream's second chunk ends in the composite
    input's f0 window (unvoiced rows too).  The g2 / session-free tests reuse chunk 0."""
    from common import BASELINE_160MS as g, voice_signal
    xs = [np.stack([voice_signal(g.input_buffer_16k_size, seed=seed) for seed in seeds]) for seeds in STREAM_SEEDS]
    xs[1][1, -4960:] = Y.composite_signal()[-4960:]
    return xs


STREAM_SEEDS = ((1, 3, 4), (6, 8, 9))          # voice_signal seeds whose YIN frames all keep 1e-4 from the voicing threshold
STREAM_CASES = (("neutral", 0), ("stream1", 0), ("stream2", 12))          # per stream: settings, integer pitch_shift
