"""tests/yin_ref.py, the float64 restatement of the YIN f0 method that tests/test_gpu_yin.py holds the kernel against, on
signals whose answer is known.  No GPU."""
import numpy as np

import yin_ref as Y


def _tone(hz, n=6000, amp=0.3):
    return (amp * np.sin(2.0 * np.pi * hz * np.arange(n) / Y.SR)).astype(np.float32)


def test_geometry_is_the_mel_front_end():
    assert Y.f0_frame(2560) == 4960 and Y.frames(np.zeros(6000, np.float32), 2560).shape == (32, 1024)
    assert Y.f0_frame(5120) == 10080 and Y.N == 704
    x = np.arange(6000, dtype=np.float32)
    F = Y.frames(x, 2560)
    sig = x[6000 - 4960:]
    assert np.array_equal(F[4], sig[4 * 160 - 512:4 * 160 + 512])            # an interior frame: centred on sample 160 t of the window
    assert np.array_equal(F[0][:512], sig[1:513][::-1]) and np.array_equal(F[0][512:], sig[:512])
    assert np.array_equal(F[31][-512:], sig[-513:-1][::-1])


def test_pad_reflect_unit_vectors():
    # the two cases of the reference's own unit test of pad_reflect
    assert np.array_equal(Y.pad_reflect(np.array([1.0, 2.0, 3.0]), 2), [3.0, 2.0, 1.0, 2.0, 3.0, 2.0, 1.0])
    assert np.array_equal(Y.pad_reflect(np.array([4.0, 5.0]), 1), [5.0, 4.0, 5.0, 4.0])


def test_harmonic_glide_tracks_the_instantaneous_f0():
    # five partials, 110 -> 440 Hz over 10240 samples, 1e-3 noise floor; 64 frames.  The integration window [0, 704 + tau) starts at the frame's
    # first sample, so its centre sits in front of the frame's centre and the estimate lags a rising glide: 1.8 % at most here; 5 % asserted
    rng = np.random.default_rng(0)
    n, s = 10240, 5120
    f = 110.0 * 2.0 ** np.linspace(0.0, 2.0, n)
    ph = 2.0 * np.pi * np.cumsum(f) / Y.SR
    x = (0.2 * sum(np.sin(k * ph) / k for k in range(1, 6)) + 1e-3 * rng.standard_normal(n)).astype(np.float32)
    f0, _ = Y.yin(x, s)
    assert f0.shape == (64,)
    c = np.arange(64) * 160 + (n - Y.f0_frame(s))          # the sample a frame is centred on
    inner = (c >= 512) & (c + 512 <= n)                    # frames without reflected samples
    assert inner.sum() == 57 and np.all(f0[inner] > 0)
    assert np.max(np.abs(f0[inner] - f[c[inner]]) / f[c[inner]]) < 0.05


def test_silence_and_noise_are_unvoiced():
    z, margin = Y.yin(np.zeros(6000, np.float32), 2560)
    assert np.all(z == 0.0) and np.allclose(margin, 0.85)          # S = 0 everywhere: d' = 1
    w, _ = Y.yin((0.1 * np.random.default_rng(1).standard_normal(6000)).astype(np.float32), 2560)
    assert np.all(w == 0.0)


def test_tones_at_the_edges_of_the_lag_range():
    # 1100 Hz is a period of 14.5 samples: the search starts under the threshold at tau = 14, walks to 15, and the parabola lands within 0.1 %
    hi, _ = Y.yin(_tone(1100.0), 2560)
    assert np.all(np.abs(hi[4:28] - 1100.0) < 1.1)
    # 50 Hz is a period of 320 samples, one past the last lag searched.  The definition does NOT read it as unvoiced: d' is already under the
    # threshold on the way down to its minimum, the walk stops at tau = 319 with d'(320) < d'(319), and the parabola through 318, 319, 320 has
    # its vertex at 320: 50 Hz.  A tone of 45 Hz (355 samples) has no lag under the threshold in the range and reads 0.
    lo, _ = Y.yin(_tone(50.0), 2560)
    assert np.all(np.abs(lo[4:28] - 50.0) < 0.05)
    dp = Y.cmnd(Y.frames(_tone(50.0), 2560)[10])
    assert dp[320] < dp[319] < dp[318] < Y.THRESHOLD
    assert np.all(Y.yin(_tone(45.0), 2560)[0][4:28] == 0.0)


def test_composite_input_of_the_gpu_test():
    # what tests/test_gpu_yin.py relies on, from the reference alone: the input has unvoiced and voiced frames of every segment, at most 10 % of
    # its frames sit within 1e-4 of the threshold, and single precision changes no voicing decision outside those
    x = Y.composite_signal()
    f0, margin = Y.yin(x, 2560)
    assert f0.shape == (32,) and f0[0] == 0.0 and margin[0] == 0.85           # the all-zero frame
    assert np.sum(margin < 1e-4) <= 3
    assert np.sum(f0 > 0) >= 12
    assert np.any(np.abs(f0 - 100.0) < 0.01) and np.any(np.abs(f0 - 800.0) < 2.0) and np.any(np.abs(f0 - 200.0) < 0.5)
    assert np.any((f0 > 125.0) & (f0 < 165.0))
    f32, _ = Y.yin(x, 2560, np.float32)
    ok = margin >= 1e-4
    assert np.array_equal(f32[ok] > 0, f0[ok] > 0)
    v = ok & (f0 > 0)
    assert np.max(np.abs(f32[v].astype(np.float64) - f0[v]) / f0[v]) < 1e-6


def test_uppower_truncates_towards_zero():
    assert [Y.uppower(s) for s in (12, 0, -7, -12, 13, -13, 24)] == [2.0, 1.0, 1.0, 0.5, 2.0, 0.5, 4.0]


def test_whole_window_input_of_the_gpu_test():
    # what tests/test_gpu_yin.py's whole-window cases rely on (n == frame: the f0 window is the whole buffer), from the reference alone: at most 10 % of
    # the frames within 1e-4 of the threshold, an end frame that is voiced (else the reflected edge is not tested), float32 changes no sure decision
    for frame16k, Tm in ((5120, 64), (5120 * 13, 448)):
        x = Y.whole_window_signal(frame16k)
        assert len(x) == Y.f0_frame(frame16k) == 160 * (Tm - 1)
        assert abs(float(np.mean(x[:512])) - 0.05) < 0.02 and abs(float(np.mean(x[-512:])) + 0.04) < 0.02          # the DC steps
        F = Y.frames(x, frame16k)
        assert F.shape == (Tm, 1024)
        assert np.array_equal(F[0][:512], x[1:513][::-1]) and np.array_equal(F[0][512:], x[:512])           # reflected about sample 0 of the buffer
        assert np.array_equal(F[Tm - 1][-512:], x[-513:-1][::-1])                                           # ... and about its last sample
        f0, margin = Y.yin(x, frame16k)
        assert f0.shape == (Tm,) and np.sum(margin < 1e-4) <= 0.10 * Tm
        assert np.any(f0[:4] > 0) or np.any(f0[-4:] > 0)
        assert np.sum(f0 > 0) >= Tm // 2 and np.sum(f0 == 0) >= 8                                            # the composite's unvoiced stretches
        f32, _ = Y.yin(x, frame16k, np.float32)
        ok = margin >= 1e-4
        assert np.array_equal(f32[ok] > 0, f0[ok] > 0)
        v = ok & (f0 > 0)
        assert np.max(np.abs(f32[v].astype(np.float64) - f0[v]) / f0[v]) < 1e-6
