"""fp64 numpy definitions of the whole-signal sample-rate converter and of the whole-file volume envelope (include/rvc_mi355x.h:
rvc_resample, rvc_change_rms), each with a float32-numpy evaluation of the same recipe (the yardstick of the GPU tests' tolerances) and the inputs of
tests/test_gpu_convert_file.py.  No GPU, no library."""
from __future__ import annotations

import math

import numpy as np

RMS_FLOOR = 1e-6


# ------------------------------------------------------------------------------------------------------------------------------
# the converter
# ------------------------------------------------------------------------------------------------------------------------------
def geometry(rate_in: int, rate_out: int, n_in: int):
    """-> {o, n, w, n_out}, or None where the engine answers RVC_SHAPE"""
    if rate_in <= 0 or rate_out <= 0:
        return None
    g = math.gcd(rate_in, rate_out)
    o, n = rate_in // g, rate_out // g
    if o > 2048 or n > 2048 or n_in <= 0 or n_in > 1 << 40:
        return None
    w = math.ceil(6 * o / (0.99 * min(o, n)))
    return {"o": o, "n": n, "w": w, "n_out": -(-n_in * n // o)}


def table(o: int, n: int) -> np.ndarray:
    """h[j][k], j < n, k < K = 2 w + o: Hann-windowed sinc of width 6 and rolloff 0.99, evaluated in fp64 and rounded once to fp32"""
    b = 0.99 * min(o, n)
    w = math.ceil(6 * o / b)
    k = np.arange(2 * w + o, dtype=np.float64)
    j = np.arange(n, dtype=np.float64)[:, None]
    t = np.clip(((k - w) / o - j / n) * b, -6.0, 6.0)
    return (np.sinc(t) * np.cos(np.pi * t / 12.0) ** 2 * b / o).astype(np.float32)


def resample(x, rate_in: int, rate_out: int, dtype=np.float64, taps=None, sequential=False) -> np.ndarray:
    """y[i n + j] = sum_k h[j][k] x[i o + k - w], x zero outside its range, N_out = ceil(N_in n / o); products and sums in `dtype` with the fp32 taps
    (taps: the engine's own table [n][K], where a test has read it).  o == n: a copy.  The sums are numpy's matrix product, which adds in blocks;
    sequential=True adds every row's products one after the other over ascending k, as the definition's chain does: over a row of tens of thousands of
    taps that is what decides the float32 error."""
    geo = geometry(rate_in, rate_out, len(x))
    o, n, w, n_out = geo["o"], geo["n"], geo["w"], geo["n_out"]
    x = np.asarray(x)
    if o == n:
        return x.astype(dtype)
    h = (table(o, n) if taps is None else np.asarray(taps, np.float32)).astype(dtype)
    K = h.shape[1]
    assert h.shape == (n, 2 * w + o)
    blocks = -(-n_out // n)
    xp = np.concatenate([np.zeros(w, dtype), x.astype(dtype), np.zeros(max(0, (blocks - 1) * o + K - w - len(x)), dtype)])
    y = np.empty(blocks * n, dtype)
    for i in range(blocks):
        seg = xp[i * o:i * o + K]
        y[i * n:(i + 1) * n] = np.cumsum(h * seg[None, :], axis=1, dtype=dtype)[:, -1] if sequential else h @ seg
    return y[:n_out]


def resample_signal(n: int, period: float = 20.0) -> np.ndarray:
    """a sine of `period` samples, one unit impulse at index 7 and a non-zero last sample: both edges and the zero extension are exercised"""
    x = 0.4 * np.sin(2 * np.pi * np.arange(n) / period + 0.3)
    if n > 7:
        x[7] += 1.0
    x[-1] = 0.7
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------
# the volume envelope
# ------------------------------------------------------------------------------------------------------------------------------
def rms_frames(n: int, rate: int):
    """-> (L, hop, F)"""
    hop = rate // 2
    return 2 * hop, hop, 1 + n // hop


def rms_track(x, rate: int, dtype=np.float64) -> np.ndarray:
    """r[f] = sqrt(mean(xpad[f hop .. f hop + L)^2)) over the signal zero-padded by L / 2 on both sides (librosa's center=True, constant pad)"""
    L, hop, F = rms_frames(len(x), rate)
    p = np.concatenate([np.zeros(L // 2, dtype), np.asarray(x).astype(dtype), np.zeros(L // 2 + hop, dtype)])
    p = p * p
    return np.array([np.sqrt(p[f * hop:f * hop + L].sum(dtype=dtype) / dtype(L)) for f in range(F)], dtype)


def half_pixel_positions(F: int, size: int, dtype=np.float64):
    """-> (u, i0, i1) of F.interpolate(mode="linear", align_corners=False) from F points to `size`"""
    u = np.maximum((np.arange(size).astype(dtype) + dtype(0.5)) * dtype(F) / dtype(size) - dtype(0.5), dtype(0))
    i0 = np.minimum(np.floor(u).astype(np.int64), F - 1)
    return u, i0, np.minimum(i0 + 1, F - 1)


def lerp_half_pixel(r, size: int, dtype=np.float64) -> np.ndarray:
    r = np.asarray(r).astype(dtype)
    u, i0, i1 = half_pixel_positions(len(r), size, dtype)
    fr = (u - i0.astype(dtype)).astype(dtype)
    return (r[i0] * (dtype(1) - fr) + r[i1] * fr).astype(dtype)


def change_rms(src, rate_src: int, y, rate_y: int, rate: float, dtype=np.float64) -> np.ndarray:
    """out[i] = y[i] R_1[i]^(1 - rate) max(R_2[i], 1e-6)^(rate - 1); rate = 1: y itself"""
    y = np.asarray(y)
    if rate == 1:
        return y.astype(dtype)
    a = lerp_half_pixel(rms_track(src, rate_src, dtype), len(y), dtype)
    b = np.maximum(lerp_half_pixel(rms_track(y, rate_y, dtype), len(y), dtype), dtype(RMS_FLOOR))
    return (y.astype(dtype) * np.power(a, dtype(1 - rate)) * np.power(b, dtype(rate - 1))).astype(dtype)


ENV_KINDS = ("plain", "silent_out", "silent_src", "loud_quiet")


def level_signal(n: int, seed: int, level: float) -> np.ndarray:
    """samples of random sign whose magnitude stays within [0.5, 1.5] level times a slow swell (tests/post_ref.py: level_signal)"""
    rng = np.random.default_rng(seed)
    swell = 1.0 + 0.5 * np.sin(2 * np.pi * (np.arange(n) / max(n, 2) * 1.5 + 0.1 * seed))
    return (rng.choice([-1.0, 1.0], n) * (0.5 + rng.random(n)) * level * swell).astype(np.float32)


def env_case(n_src: int, n_y: int, kind: str):
    """-> (source [n_src], converted [n_y]).  plain; silent_out (zeros: the 1e-6 floor is active everywhere, the result is zero); silent_src (the result is
    zero below rate 1); loud_quiet (both are loud in their first half and 200 times quieter in the second)"""
    src, y = level_signal(n_src, 3 * n_src + 1, 0.1), level_signal(n_y, 5 * n_y + 2, 0.2)
    if kind == "silent_out":
        y = np.zeros(n_y, np.float32)
    elif kind == "silent_src":
        src = np.zeros(n_src, np.float32)
    elif kind == "loud_quiet":
        src[n_src // 2:] *= np.float32(0.005)
        y[n_y // 2:] *= np.float32(0.005)
        src, y = src * np.float32(4), y * np.float32(2)
    else:
        assert kind == "plain"
    return src.astype(np.float32), y.astype(np.float32)


def self_check() -> None:
    assert geometry(44100, 16000, 4410) == {"o": 441, "n": 160, "w": 17, "n_out": 1600}
    assert geometry(0, 16000, 5) is None and geometry(16000, 16000, 0) is None and geometry(4099, 1, 5) is None
    h = table(441, 160)
    assert h.shape == (160, 2 * 17 + 441) and np.abs(h.astype(np.float64).sum(1) - 1.0).max() < 2e-3      # every phase is a low-pass of DC gain 1
    assert rms_frames(7, 2) == (2, 1, 8) and rms_frames(99, 201) == (200, 100, 1)
    assert np.allclose(rms_track(np.ones(8), 4), [np.sqrt(0.5), 1, 1, 1, np.sqrt(0.5)], rtol=0, atol=1e-15)
