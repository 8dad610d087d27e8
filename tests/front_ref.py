"""float64 definitions of the head and the tail of the f0 branch and of ContentVec's first layer, for tests/test_gpu_front.py (pinned against
independent implementations by tests/test_front_ref.py).  Plain numpy, written from the definitions -- the reference's RMVPE front end and decode,
its pitch cache and coarse pitch, the upstream synthesizer's SineGen -- not from the kernels' indexing."""
import numpy as np
from scipy.special import erf

from oracle import oracle as O

N_FFT, HOP, N_MELS, N_BINS = 1024, 160, 128, 360
CENTS0 = 1997.3794084376191


def mel_basis():
    return O.mel_filterbank().astype(np.float64)                  # [128][513]


def mel_linear(audio, frame):
    """the last `frame` samples of audio -> (s [128][Tm] mel energies before the floor and the logarithm, 2-norm of every windowed frame [Tm])"""
    sig = np.asarray(audio, np.float64)[len(audio) - frame:]
    Tm = 1 + frame // HOP
    padded = np.pad(sig, N_FFT // 2, mode="reflect")
    win = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT))
    frames = np.lib.stride_tricks.sliding_window_view(padded, N_FFT)[::HOP][:Tm] * win
    mag = np.abs(np.fft.rfft(frames, axis=1))                     # [Tm][513]
    return mel_basis() @ mag.T, np.sqrt(np.sum(frames * frames, axis=1))


def logmel(audio, frame):
    return np.log(np.maximum(mel_linear(audio, frame)[0], 1e-5))


def gelu(v):
    return 0.5 * v * (1.0 + erf(v / np.sqrt(2.0)))


def conv0_raw(x, w, stride):
    """x [B][L], w [C][K] -> Conv1d(1 -> C, K taps, stride, no padding, no bias) [B][C][To]"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    K = w.shape[1]
    To = (x.shape[1] - K) // stride + 1
    win = np.lib.stride_tricks.sliding_window_view(x, K, axis=1)[:, ::stride][:, :To]
    return np.einsum("btk,ck->bct", win, w)


def conv0_gn_gelu(x, w, stride, gamma, beta):
    """conv0_raw + GroupNorm with one group per channel (two-pass mean / variance over time, eps 1e-5) + exact-erf GELU"""
    y = conv0_raw(x, w, stride)
    mean = y.mean(axis=2, keepdims=True)
    var = ((y - mean) ** 2).mean(axis=2, keepdims=True)
    g, b = np.asarray(gamma, np.float64)[None, :, None], np.asarray(beta, np.float64)[None, :, None]
    return gelu((y - mean) / np.sqrt(var + 1e-5) * g + b)


def decode_pitch(sal, threshold=0.03, uppower=1.0):
    """sal [360][T] -> (f0 [T] in Hz, panic [T]).  The reference takes the argmax of every row zero-padded by 4 on both sides (the first maximum; index 0
    when nothing is positive), `starts`, and then reads the nine salience values at starts .. starts + 8 of the UNPADDED row against the cents of the
    padded table at the same indices: the window sits 4 bins above the peak.  starts + 8 >= 360 is an out-of-bounds panic there.  The average cents
    are zeroed where the row maximum is not above the threshold; 10 * 2^(cents / 1200) Hz, and exactly 10 Hz means unvoiced (0)."""
    sal = np.asarray(sal, np.float64)
    T = sal.shape[1]
    padded = np.zeros((N_BINS + 8, T))
    padded[4:4 + N_BINS] = sal
    starts = np.argmax(padded, axis=0)
    starts[np.max(padded, axis=0) <= 0.0] = 0
    panic = starts + 8 >= N_BINS
    s0 = np.where(panic, 0, starts)
    idx = s0[None, :] + np.arange(9)[:, None]
    sv = np.take_along_axis(sal, idx, axis=0)
    cm = (idx - 4.0) * 20.0 + CENTS0
    with np.errstate(invalid="ignore", divide="ignore"):
        cents = np.sum(sv * cm, axis=0) / np.sum(sv, axis=0)
    cents = np.where(np.max(sal, axis=0) > threshold, cents, 0.0)
    hz = 10.0 * 2.0 ** (cents / 1200.0)
    hz = np.where(hz == 10.0, 0.0, hz)
    return np.where(panic, 0.0, hz * uppower), panic


def argmax_margin(sal):
    """per column: the maximum minus the largest value at any other bin"""
    s = np.sort(np.asarray(sal, np.float64), axis=0)
    return s[-1] - s[-2]


def update_cache(cache, f0, shift, cache_start, read_start, R):
    """-> (new cache [1024], pitchf [R]): the cache moves down by `shift` (its tail keeps the old values), f0[3 : len - 1] is written from cache_start on,
    R values are read from read_start on"""
    c = np.array(cache, np.float64)
    if shift < 1024:
        c[:1024 - shift] = c[shift:].copy()
    n = len(f0) - 4
    c[cache_start:cache_start + n] = np.asarray(f0, np.float64)[3:3 + n]
    return c, c[read_start:read_start + R].copy()


def coarse_x(f):
    """the mel-scale position of f before rounding: 1 .. 255 (f0_mel_min / max = 50 / 500 Hz), 1 where the mel value is not positive"""
    f = np.asarray(f, np.float64)
    lo, hi = np.log(50.0 / 700.0 + 1.0) * 1127.0, np.log(500.0 / 700.0 + 1.0) * 1127.0
    x = np.log(f / 700.0 + 1.0) * 1127.0
    x = np.where(x > 0.0, (x - lo) * 254.0 / (hi - lo) + 1.0, x)
    return np.clip(x, 1.0, 255.0)


def coarse_pitch(f):
    """-> (integers 1 .. 255, rounding half away from zero; distance of x from the nearest .5 boundary)"""
    x = coarse_x(f)
    return np.floor(x + 0.5).astype(np.int64), np.abs(x - np.floor(x) - 0.5)


def sine_phase(f0, upp, sr, dtype=np.float64):
    """SineGen's phase (in turns) per sample: the per-frame increments f0 / sr mod 1, their cumulative sum times upp interpolated linearly (align corners)
    to the sample rate and taken mod 1; a sample where that falls is a wrap, and the phase is the running sum of (increment of the sample's frame - wraps).
    dtype = float32 restates the same sequential recipe in single precision (the measure of what fp32 costs on a track, test_gpu_front.py)."""
    f = np.asarray(f0, dtype)
    T, N = len(f), len(f) * upp
    rad = np.fmod(f / dtype(sr), dtype(1.0))
    cum = np.cumsum(rad, dtype=dtype) * dtype(upp)
    pos = (np.arange(N, dtype=dtype) * dtype(T - 1) / dtype(N - 1)) if N > 1 else np.zeros(N, dtype)
    j0 = np.minimum(np.floor(pos).astype(np.int64), T - 1)
    j1 = np.minimum(j0 + 1, T - 1)
    w = pos - j0.astype(dtype)
    tmp = np.fmod(cum[j0] * (dtype(1.0) - w) + cum[j1] * w, dtype(1.0))
    wrap = np.zeros(N, dtype)
    wrap[1:] = np.where(np.diff(tmp) < 0, dtype(-1.0), dtype(0.0))
    return np.cumsum(rad[np.arange(N) // upp] + wrap, dtype=dtype)


def nsf_source(f0, upp, sr, lin_w, lin_b, noise):
    """harmonic source of the upstream synthesizer (SineGen with no overtones + Linear(1, 1) + tanh): f0 [T] -> [T upp]; noise: standard normals [T upp]"""
    f = np.asarray(f0, np.float64)
    uv = np.repeat((f > 0).astype(np.float64), upp)
    sine = np.sin(2.0 * np.pi * sine_phase(f, upp, sr)) * 0.1
    namp = uv * 0.003 + (1.0 - uv) * 0.1 / 3.0
    return np.tanh(lin_w * (sine * uv + namp * np.asarray(noise, np.float64)) + lin_b)
