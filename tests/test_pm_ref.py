"""The float64 restatement of the PM f0 method (tests/pm_ref.py) on inputs whose answer is known, its accuracy on tones (the record
of DESIGN.md section 26, pinned here at twice the recorded value), what single precision costs the same recipe, and the margins of the inputs of
tests/test_gpu_pm.py.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import pm_ref as P
import yin_ref as Y

FRAME16K = 2560
# relative error of the float64 reference on five-partial tones, frames 4 .. 27 (the frames whose 1024 samples hold no reflected sample), without Praat's
# Brent refinement: the vertex of the parabola through three lags is all a candidate's lag gets, so the error grows with the curvature a lag step spans
TONE_ERROR = {62.5: 1.970e-4, 110.0: 2.323e-6, 220.0: 1.829e-5, 440.0: 1.298e-4, 880.0: 9.310e-4}
# float32 numpy against float64 on the three streams of the GPU test (frames outside the left-out set): f relative, s and delta absolute
F32_DEVIATION = {"f": 1.77e-7, "s": 3.31e-7, "delta": 3.40e-7}
CAND_MARGIN = 1e-5          # the candidates' decisions the GPU test relies on: about 70 x the float32 deviation of r
LEFT_OUT = {0: {25}, 1: set(), 2: set()}          # frames of each stream under CAND_MARGIN: the 800 Hz frame whose 14th and 15th candidate score alike


def test_the_window_table():
    rw = P.RW
    assert rw.dtype == np.float32 and rw.shape == (353,) and rw[0] == 1.0 and np.all(np.diff(rw) < 0) and rw[352] > 0.3
    assert P.H.shape == (960,) and abs(P.H.sum() - 480.0) < 1e-9


@pytest.mark.parametrize("f", sorted(TONE_ERROR))
def test_tones(f):
    f0, c, idx, _, _ = P.pm(P.tone(f), FRAME16K)
    inner = f0[4:28]
    assert np.all(inner > 0), f0
    err = float(np.max(np.abs(inner - f) / f))
    print("%.1f Hz: largest relative error on frames 4 .. 27: %.3e (recorded %.3e)" % (f, err, TONE_ERROR[f]))
    assert err <= 2.0 * TONE_ERROR[f]
    assert np.all(c["n"][4:28] >= 1) and np.all(c["n"] <= P.MAXC)
    if f >= 880:          # 17 peaks for 14 places: the selection ran
        assert np.any(c["n"] == P.MAXC)


def test_silence_and_noise_read_unvoiced():
    f0, c, *_ = P.pm(np.zeros(6000, np.float32), FRAME16K)
    assert np.all(f0 == 0) and np.all(c["n"] == 0)          # G == 0
    x = np.zeros(6000, np.float32); x[:1200] = P.tone(200.0, 1200)          # G > 0, later frames all zero: ra(0) == 0
    f0, c, *_ = P.pm(x, FRAME16K)
    assert np.all(c["n"][8:] == 0) and np.all(f0[8:] == 0)
    rng = np.random.default_rng(1)
    f0, _, *_ = P.pm((0.1 * rng.standard_normal(6000)).astype(np.float32), FRAME16K)
    assert np.all(f0 == 0)


def test_a_strong_second_harmonic_reads_the_fundamental():
    """150 Hz with partial amplitudes 0.4, 1, 0.3: the path reads 150 Hz on every frame, the first and last within the 3 % that the reflected samples cost.
    YIN's reference does not jump on this input either -- its cumulative-mean normalisation handles a strong even harmonic -- but it loses the first three
    and the last two frames to its threshold, which the path here carries through"""
    x = P.tone(150.0, weights=[0.4, 1.0, 0.3])
    f0, *_ = P.pm(x, FRAME16K)
    assert np.all(f0 > 0) and np.max(np.abs(f0 - 150.0)) < 4.5 and np.max(np.abs(f0[4:28] - 150.0)) < 0.05
    y, _ = Y.yin(x, FRAME16K)
    print("PM %s\nYIN %s" % (np.round(f0, 1), np.round(y, 1)))
    assert np.sum(y == 0) >= 1 and np.all(np.abs(y[y > 0] - 150.0) < 4.5)


def test_an_onset_inside_the_window():
    x = np.zeros(6000, np.float32); x[3000:] = P.tone(180.0, 3000)
    f0, *_ = P.pm(x, FRAME16K)
    on = int(np.argmax(f0 > 0))
    assert 11 <= on <= 13 and np.all(f0[:on] == 0) and np.all(f0[on:] > 0) and np.max(np.abs(f0[on + 2:28] - 180.0)) < 0.2


def test_path_costs():
    # two candidates an octave apart, the upper slightly stronger on one frame only: the octave-jump cost keeps the path on the lower one
    Tm = 8
    n = np.full(Tm, 2)
    f = np.zeros((Tm, P.NC)); f[:, 1], f[:, 2] = 100.0, 200.0
    d = np.zeros((Tm, P.NC)); d[:, 0] = 0.3; d[:, 1], d[:, 2] = 0.9, 0.8
    d[4, 1], d[4, 2] = 0.8, 0.9
    idx, f0, margin, terms = P.path(n, f, d)
    assert np.all(idx == 1) and np.all(f0 == 100.0) and np.all(margin > 0) and abs(terms - (7 * 0.9 + 0.8)) < 1e-12
    assert abs(margin[4] - (P.OJ - 0.1 + 3 * 0.1)) < 1e-12          # the best alternative: jump up there and stay up for the last three frames
    # ties go to the lowest index
    d[:, 1] = d[:, 2] = 0.9
    f[:, 2] = 100.0
    assert np.all(P.path(n, f, d)[0] == 1)


def test_the_gpu_tests_inputs_keep_their_margins():
    X = P.stream_signals()
    assert X.shape == (3, 6000) and X.dtype == np.float32
    dev = {"f": 0.0, "s": 0.0, "delta": 0.0}
    for s in range(3):
        f0, c, idx, pmargin, terms = P.pm(X[s], FRAME16K)
        c32 = P.candidates(X[s], FRAME16K, np.float32)
        out = set(np.where(c["margin"] < CAND_MARGIN)[0].tolist())
        print("stream %d: frames under the candidate margin %s, smallest margin elsewhere %.3e; smallest path margin %.3e against %.3e" %
              (s, sorted(out), np.min(c["margin"][c["margin"] >= CAND_MARGIN]), pmargin.min(), 4 * 32 * 2.0 ** -24 * terms))
        assert out == LEFT_OUT[s] and len(out) <= 2          # at most 2 of 32: a condition
        assert np.sum(pmargin >= 4 * 32 * 2.0 ** -24 * terms) >= 30
        keep = np.array([t not in out for t in range(32)])
        # the same recipe in float32 makes the same decisions on the kept frames ...
        assert np.array_equal(c["n"][keep], c32["n"][keep]) and np.array_equal(c["lag"][keep], c32["lag"][keep])
        # ... and deviates by what the GPU test multiplies by 8
        a, b = c["f"][keep], c32["f"][keep].astype(np.float64)
        dev["f"] = max(dev["f"], float(np.max(np.abs(a - b)[a > 0] / a[a > 0])))
        for k in ("s", "delta"):
            dev[k] = max(dev[k], float(np.max(np.abs(c[k][keep] - c32[k][keep].astype(np.float64)))))
    print("float32 numpy against float64:", dev)
    for k in dev:
        assert dev[k] <= 1.05 * F32_DEVIATION[k], (k, dev[k])
    # the composite exercises what it is meant to: unvoiced frames, a frame with more peaks than places, voiced runs
    f0, c, *_ = P.pm(X[0], FRAME16K)
    assert np.sum(f0 > 0) >= 12 and np.sum(f0 == 0) >= 8 and np.any(c["n"] == P.MAXC) and np.any(c["n"] == 0) and f0[0] == 0.0


def test_the_synthetic_candidates_of_the_longest_window():
    Tm = 1024
    n, f, d = P.synthetic_candidates(Tm)
    idx, f0, margin, terms = P.path(n, f.astype(np.float32), d.astype(np.float32))
    thr = 4 * Tm * 2.0 ** -24 * terms
    print("Tm 1024: %d frames over the path margin %.3e, voiced %d" % (np.sum(margin >= thr), thr, np.sum(f0 > 0)))
    assert np.sum(margin >= thr) >= 0.9 * Tm and np.sum(f0 > 0) > 500 and np.sum(f0 == 0) > 200 and n.max() == P.MAXC and n.min() >= 2
