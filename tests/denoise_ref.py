"""Streaming spectral-gate noise reduction (DESIGN.md "Spectral-gate noise reduction"): the definition in fp64 numpy, frame by frame, and the "naive
fp32" evaluation of the same formulas (np.float32 throughout, np.fft replaced by an explicit fp32 DFT matrix product whose phase 2 pi k j / N is formed
unreduced) whose deviation from fp64, delta32, sets the kernels' tolerance.  Also the test signals.  tests/test_denoise_ref.py and
tests/test_gpu_denoise.py import from here; nothing in this file needs a GPU."""
from __future__ import annotations

import numpy as np

SOFT, FLOOR_MS, RELEASE_MS, SMOOTH, EPS = 0.1, 200.0, 50.0, 10, 1e-8
A = np.float32(np.exp(-10.0 / FLOOR_MS))            # noise-floor smoothing per 10 ms frame
B = np.float32(np.exp(-10.0 / RELEASE_MS))          # release hold per 10 ms frame
# the four shapes of the standalone GPU test: (sample rate, hops per call)
SHAPES = [(8000, 6), (16000, 4), (44100, 3), (48000, 2)]
# (signal, strength, threshold) of the streams of one call
CASES = [("voiced", 1.0, 2.0), ("voiced", 0.6, 0.5), ("onset", 1.0, 0.5), ("onset", 0.6, 2.0)]
# the session tests' denoised inputs: (sample rate, samples per chunk at 160 ms, chunks, seed of `voiced`), strength 1, threshold 2
SESSION_INPUTS = [(16000, 2560, 4, 41), (44100, 7056, 4, 41), (48000, 7680, 3, 60)]


class RefDenoiser:
    """One stream.  dt = np.float64: the definition (np.fft); dt = np.float32: the naive evaluation.  mask_override: a value every g[k] is forced to
    (steps 2-5 still run and keep their state).  self.gains holds G[k] of every frame processed so far."""

    def __init__(self, sample_rate, strength=0.0, threshold=2.0, dt=np.float64, mask_override=None):
        assert sample_rate % 100 == 0
        self.dt, self.zc = dt, sample_rate // 100
        self.N, self.K = 2 * self.zc, self.zc + 1
        self.strength, self.threshold, self.mask_override = strength, threshold, mask_override
        N, K = self.N, self.K
        self.w = np.sin(dt(np.pi) * (np.arange(N).astype(dt) + dt(0.5)) / dt(N)).astype(dt)
        if dt == np.float32:
            ph = (dt(2.0 * np.pi) * np.arange(K).astype(dt)[:, None] * np.arange(N).astype(dt)[None, :] / dt(N)).astype(dt)     # [K][N], unreduced
            self.c, self.s = np.cos(ph).astype(dt), np.sin(ph).astype(dt)
        self.reset()

    def reset(self):
        dt = self.dt
        self.S, self.g = np.zeros(self.K, dt), np.zeros(self.K, dt)
        self.prev, self.tail = np.zeros(self.zc, dt), np.zeros(self.zc, dt)
        self.gains = []

    def set(self, strength, threshold=2.0):
        self.strength, self.threshold = strength, threshold

    def _rfft(self, v):
        if self.dt == np.float64:
            X = np.fft.rfft(v)
            return X.real, X.imag
        return (self.c @ v).astype(np.float32), (-(self.s @ v)).astype(np.float32)

    def _irfft(self, yr, yi):
        if self.dt == np.float64:
            return np.fft.irfft(yr + 1j * yi, self.N)
        dt, K = self.dt, self.K
        sign = np.where(np.arange(self.N) % 2 == 0, dt(1), dt(-1)).astype(dt)
        inner = (yr[1:K - 1] @ self.c[1:K - 1] - yi[1:K - 1] @ self.s[1:K - 1]).astype(dt)
        return ((yr[0] + sign * yr[K - 1] + dt(2) * inner) / dt(self.N)).astype(dt)

    def _frame(self, frame):
        dt, K = self.dt, self.K
        xr, xi = self._rfft((self.w * frame).astype(dt))
        M = np.sqrt(xr * xr + xi * xi).astype(dt)
        slope = ((M - self.S) / np.maximum(self.S, dt(EPS))).astype(dt)
        self.S = (dt(A) * self.S + (dt(1) - dt(A)) * M).astype(dt)
        with np.errstate(over="ignore"):
            g0 = (dt(1) / (dt(1) + np.exp(-(slope - dt(self.threshold)) / dt(SOFT)))).astype(dt)
        num, den = np.zeros(K, dt), np.zeros(K, dt)
        for d in range(-SMOOTH, SMOOTH + 1):
            tw, lo, hi = dt(SMOOTH + 1 - abs(d)), max(0, -d), min(K, K - d)
            num[lo:hi] += tw * g0[lo + d:hi + d]
            den[lo:hi] += tw
        self.g = np.maximum((num / den).astype(dt), dt(B) * self.g).astype(dt)
        g = self.g if self.mask_override is None else np.full(K, self.mask_override, dt)
        G = (dt(self.strength) * g + (dt(1) - dt(self.strength))).astype(dt)
        self.gains.append(G.copy())
        return (self.w * self._irfft((G * xr).astype(dt), (G * xi).astype(dt))).astype(dt)

    def process(self, x):
        """n = a multiple of zc samples in -> n samples out (delayed by zc); strength 0: the input itself, state untouched"""
        x = np.asarray(x)
        assert x.ndim == 1 and len(x) % self.zc == 0 and len(x) > 0
        if self.strength == 0:
            return x.copy()
        dt, H = self.dt, self.zc
        out = np.empty(len(x), dt)
        for m in range(len(x) // H):
            blk = x[m * H:(m + 1) * H].astype(dt)
            f = self._frame(np.concatenate([self.prev, blk]))
            out[m * H:(m + 1) * H] = self.tail + f[:H]
            self.prev, self.tail = blk, f[H:].copy()
        return out


def denoise(x, sample_rate, strength, threshold, dt=np.float64):
    return RefDenoiser(sample_rate, strength, threshold, dt).process(x)


def bound(x, sample_rate, strength, threshold):
    """-> (fp64 definition, delta32, peak): the kernels get 2 * delta32; an input must not widen its own tolerance: delta32 <= 1e-4 * peak"""
    r64 = denoise(x, sample_rate, strength, threshold)
    d32 = float(np.abs(denoise(x, sample_rate, strength, threshold, np.float32) - r64).max())
    peak = float(np.abs(r64).max())
    assert 0 < d32 <= 1e-4 * peak, (sample_rate, strength, threshold, d32, peak)
    return r64, d32, peak


# ------------------------------------------------------------------------------------------------------------------------------
# signals
# ------------------------------------------------------------------------------------------------------------------------------
def voiced(n, sample_rate, seed, f0=170.0):
    """a voiced harmonic signal (six partials below Nyquist, peak about 0.5) on a white floor 40 dB below that peak"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(sample_rate)
    amps = [1.0, 0.6, 0.45, 0.3, 0.2, 0.12]
    x = sum(a * np.sin(2 * np.pi * (h + 1) * f0 * t + 0.7 * h) for h, a in enumerate(amps) if (h + 1) * f0 < 0.45 * sample_rate)
    x = 0.5 * x / np.abs(x).max()
    return (x + 0.005 * rng.standard_normal(n)).astype(np.float32)


def onset(n, sample_rate, seed):
    """silence (exact zeros), then the voiced signal: a hop and a half of silence (the first frame is then all zeros: M = S = 0), half a hop when the
    signal has fewer than four hops (the output, one hop late, would hold nothing else)"""
    zc = sample_rate // 100
    x = voiced(n, sample_rate, seed + 50)
    x[:3 * zc // 2 if n >= 4 * zc else zc // 2] = 0
    return x


def case_signal(kind, n, sample_rate, seed):
    return voiced(n, sample_rate, seed) if kind == "voiced" else onset(n, sample_rate, seed)


def case_batch(sample_rate, hops, seed=0):
    """the streams of one standalone call: -> x [len(CASES)][hops * zc] float32"""
    n = hops * (sample_rate // 100)
    return np.stack([case_signal(kind, n, sample_rate, seed + 7 * i) for i, (kind, _, _) in enumerate(CASES)])
