"""fp64 numpy definitions of the file converter's host-visible arithmetic: the window geometry, the 48 Hz zero-phase high-pass and
the chained SOLA stitch, with their own self-checks (self_check(), run by tests/test_convert_ref.py).  No GPU, no library."""
from __future__ import annotations

import numpy as np

HP_M = 1024


def geometry(n16k: int, sample_rate: int, k: int = 0, context: int = 0, crossfade: int = 0):
    """the formulas of include/rvc_mi355x.h restated -> dict, or None where the engine answers RVC_SHAPE"""
    k, C, X, Q = k or 14, context or 48, crossfade or 5, 1
    if not 2 <= k <= 32 or C < 3 or X < 1 or sample_rate <= 0 or sample_rate % 100:
        return None
    F = 32 * k - 1
    H = F - 2 * C - X - Q
    zc = sample_rate // 100
    if H < X or Q * zc > 1023:
        return None
    Nf = -(-n16k // 160)
    return {"windows": -(-Nf // H), "n": 160 * F, "sample_frame_16k_size": 5120 * (k - 1), "skip_head": C, "return_length": H + X + Q, "hop": H, "zc": zc,
            "output_samples": Nf * zc}


def front_end_frames(sample_frame_16k_size: int) -> int:
    """the f0 front end's window in samples: fr = 5120 ((sf + 799) // 5120 + 1) - 160 (rmvpe.rs:256)"""
    return 5120 * ((sample_frame_16k_size + 799) // 5120 + 1) - 160


def gather_windows(x: np.ndarray, geo: dict) -> np.ndarray:
    """(windows, n): window w = samples [160 (w H - C), + n) of x, zero outside"""
    n, H, C, W = geo["n"], geo["hop"], geo["skip_head"], geo["windows"]
    xp = np.concatenate([np.zeros(160 * C, x.dtype), x, np.zeros(n + 160 * H, x.dtype)])
    return np.stack([xp[160 * w * H: 160 * w * H + n] for w in range(W)])


def highpass_taps64() -> np.ndarray:
    j = np.arange(2 * HP_M + 1, dtype=np.float64)
    fc = 48.0 / 16000.0
    lp = 2 * fc * np.sinc(2 * fc * (j - HP_M)) * (0.42 - 0.5 * np.cos(2 * np.pi * j / (2 * HP_M)) + 0.08 * np.cos(4 * np.pi * j / (2 * HP_M)))
    lp /= lp.sum()
    h = -lp
    h[HP_M] += 1.0
    return h


def highpass_taps() -> np.ndarray:
    """the taps the engine uses: the fp64 definition rounded once to fp32"""
    return highpass_taps64().astype(np.float32)


def highpass(x) -> np.ndarray:
    """y[i] = sum_j h[j] x[i + M - j] over the zero-extended signal, in fp64 with the fp32 taps; output length len(x)"""
    x = np.asarray(x, np.float64)
    return np.convolve(x, highpass_taps().astype(np.float64))[HP_M: HP_M + len(x)]


def highpass_f32(x) -> np.ndarray:
    """the same recipe with every product and sum in float32"""
    x = np.asarray(x, np.float32)
    return np.convolve(x, highpass_taps())[HP_M: HP_M + len(x)]


def sola_offset(seg, tail, search: int) -> int:
    """get_sola_offset (rt_utils.rs:60-90): cor[l] = <seg[l:], tail> / sqrt(<seg[l:], seg[l:]> + 1e-8), the LAST maximum wins"""
    seg, tail = np.asarray(seg, np.float64), np.asarray(tail, np.float64)
    L = len(tail)
    cor = np.array([seg[l: l + L] @ tail / np.sqrt(seg[l: l + L] @ seg[l: l + L] + 1e-8) for l in range(search + 1)])
    return int(search - np.argmax(cor[::-1]))


def fade_in(sola_len: int) -> np.ndarray:
    x = np.arange(sola_len, dtype=np.float64) / (sola_len - 1) if sola_len > 1 else np.zeros(1)
    return np.sin(0.5 * np.pi * x) ** 2


def stitch(windows, sola_len: int, search: int, frame: int, offsets=None):
    """the chained LINEAR SOLA step over windows (W, window_len), the tail starting as zeros -> (audio (W frame,), offsets (W,)).  offsets given: blend at
    those offsets instead of searching (the samples of a run whose offsets are known)"""
    y = np.asarray(windows, np.float64)
    assert y.ndim == 2 and frame >= sola_len >= 1 and y.shape[1] >= search + frame + sola_len
    fi = fade_in(sola_len)
    tail = np.zeros(sola_len)
    out, offs = [], []
    for w in range(y.shape[0]):
        off = sola_offset(y[w], tail, search) if offsets is None else int(offsets[w])
        seg = y[w, off: off + frame + sola_len].copy()
        seg[:sola_len] = seg[:sola_len] * fi + tail * (1.0 - fi)
        tail = seg[frame: frame + sola_len].copy()
        out.append(seg[:frame]); offs.append(off)
    return np.concatenate(out), np.array(offs, np.int32)


def self_check() -> None:
    t = np.arange(6000) / 16000.0
    mid = slice(HP_M, 6000 - HP_M)
    # a unit sine at 1 kHz, far inside the pass band, comes through unchanged; DC does not come through
    s = np.sin(2 * np.pi * 1000.0 * t)
    assert np.max(np.abs(highpass(s)[mid] - s[mid])) < 1e-4
    assert np.max(np.abs(highpass(np.ones(6000))[mid])) < 1e-3
    assert abs(float(highpass_taps64().sum())) < 1e-12 and np.allclose(highpass_taps64(), highpass_taps64()[::-1], rtol=0, atol=1e-15)      # zero at DC, zero phase
    assert len(highpass([1.0])) == 1 and abs(highpass([1.0])[0] - float(highpass_taps()[HP_M])) == 0.0
    # one window: every lag ties against the zero tail (offset = search) and the frame is the faded-in segment
    r = np.random.default_rng(5)
    w = r.uniform(-1, 1, (1, 8 + 4 + 16))
    a, o = stitch(w, 8, 4, 16)
    exp = w[0, 4: 20].copy()
    exp[:8] *= fade_in(8)
    assert o.tolist() == [4] and np.allclose(a, exp, rtol=0, atol=1e-15)
    # a second window that repeats the first one's tail at lag 2 is found there, and the seam is then the tail itself
    w2 = r.uniform(-1, 1, (2, 28))
    w2[1, 2: 10] = w2[0, 20: 28]
    a, o = stitch(w2, 8, 4, 16)
    assert o.tolist() == [4, 2] and np.allclose(a[16: 24], w2[0, 20: 28], rtol=0, atol=1e-15)
    assert fade_in(8)[0] == 0.0 and abs(fade_in(8)[-1] - 1.0) < 1e-15
    # the front end's window is the converter's window
    for k in (2, 16, 32):
        g = geometry(1, 48000, k, 3, 1)
        assert front_end_frames(g["sample_frame_16k_size"]) == g["n"] == 160 * (32 * k - 1)
