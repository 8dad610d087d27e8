"""The streaming post-processing chain and the resamplers as plain numpy, float64 by default (DESIGN.md "Post-processing and resamplers: what is tested").

Written from the reference project's text -- obs-rvc/src/rt_utils.rs:60-132 (SOLA offset, RMS, align-corners interpolation, envelope mixing) and
obs-rvc/src/lib.rs:661-679, 758-794 (the two rings, the SOLA blend / tail / frame) -- and, for the converters, from the header comment of
obs_rvc_amd/csrc/resample.hip.h (rubato's synchronous-FFT algorithm); not from the kernels.  Every function takes `dtype`: float64 is the definition,
float32 the naive single-precision evaluation whose deviation from the definition (delta32) sets the kernels' tolerance, as pv_crossfade(..., np.float32)
does in tests/test_crossfade.py.  The constants the reference writes as f32 literals (1e-3, 1e-8) are those f32 values in both evaluations.

The second half builds the test inputs of tests/test_gpu_post.py; tests/test_post_ref.py asserts their conditions (delta32 <= 1e-4 peak, arg-max lead, floor
margin, converter geometry) without a GPU."""
from __future__ import annotations

from math import gcd

import numpy as np
import scipy.fft as sfft

from oracle import resample_oracle as RO

FLOOR = float(np.float32(1e-3))          # rt_utils.rs:126  f32::max(x, 1e-3)
GUARD = float(np.float32(1e-8))          # rt_utils.rs:76   (x + 1e-8).sqrt()


# ------------------------------------------------------------------------------------------------------------------------------
# envelope mixing (rt_utils.rs:93-132)
# ------------------------------------------------------------------------------------------------------------------------------
def rms(y, frame, hop, dtype=np.float64):
    """zero-pad frame // 2 per side, square, mean over windows of `frame` every `hop`, sqrt"""
    y = np.asarray(y).astype(dtype)
    pad = frame // 2
    p = np.concatenate([np.zeros(pad, dtype), y, np.zeros(pad, dtype)])
    p = p * p
    nf = (len(p) - frame) // hop + 1
    return np.array([np.sqrt(p[f * hop:f * hop + frame].sum(dtype=dtype) / dtype(frame)) for f in range(nf)], dtype)


def lerp_align_corners(v, size, dtype=np.float64):
    v = np.asarray(v).astype(dtype)
    n = len(v)
    step = dtype(n - 1) / dtype(size - 1)
    idx = (np.arange(size).astype(dtype) * step).astype(dtype)
    fl = np.clip(np.floor(idx).astype(np.int64), 0, n - 1)
    ce = np.clip(np.ceil(idx).astype(np.int64), 0, n - 1)
    fr = (idx - fl.astype(dtype)).astype(dtype)
    return (v[fl] * (dtype(1) - fr) + v[ce] * fr).astype(dtype)


def envelop_mix(inp, out, zc, exponent, dtype=np.float64):
    """-> (mixed output, RMS track of the input, RMS track of the output); exponent = 1 - mix_rate"""
    out = np.asarray(out).astype(dtype)
    n = len(out)
    r1, r2 = rms(np.asarray(inp)[:n], 4 * zc, zc, dtype), rms(out, 4 * zc, zc, dtype)
    a = lerp_align_corners(r1, n + 1, dtype)[:n]
    b = np.maximum(lerp_align_corners(r2, n + 1, dtype), dtype(FLOOR))[:n]
    return (out * np.power(a / b, dtype(exponent))).astype(dtype), r1, r2


def floor_margin(out, zc):
    """the smallest distance of the interpolated output RMS from the 1e-3 floor over the samples that are mixed"""
    n = len(out)
    return float(np.abs(lerp_align_corners(rms(out, 4 * zc, zc), n + 1)[:n] - FLOOR).min())


# ------------------------------------------------------------------------------------------------------------------------------
# SOLA (rt_utils.rs:60-90, lib.rs:768-794)
# ------------------------------------------------------------------------------------------------------------------------------
def last_max(cor):
    """rt_utils.rs:80-88: the fold keeps the running maximum only while it is strictly greater"""
    best, bv = 0, cor[0]
    for l in range(1, len(cor)):
        if not bv > cor[l]:
            best, bv = l, cor[l]
    return best


def sola_cor(output, sola, search, dtype=np.float64):
    """-> (the search + 1 normalised correlations <out[l..], sola> / sqrt(<out[l..], out[l..]> + 1e-8), the offset by the last-maximum rule)"""
    o, s = np.asarray(output).astype(dtype), np.asarray(sola).astype(dtype)
    n = len(s)
    cor = np.empty(search + 1, dtype)
    for l in range(search + 1):
        w = o[l:l + n].copy()            # (a fresh array per lag: equal windows give equal bits whatever their alignment was)
        cor[l] = (w * s).sum(dtype=dtype) / np.sqrt((w * w).sum(dtype=dtype) + dtype(GUARD))
    return cor, last_max(cor)


def fade_in(n, dtype=np.float64):
    """lib.rs:231-232: sin^2(x pi / 2) over linspace(0, 1, n)"""
    x = np.linspace(0.0, 1.0, n).astype(dtype) if n > 1 else np.zeros(1, dtype)
    return (np.sin(x * dtype(0.5) * dtype(np.pi)) ** 2).astype(dtype)


def sola_step(output, sola, search, frame, dtype=np.float64, off=None):
    """-> (offset, output with the seam blended, the frame, the new tail).  off: take this offset instead of searching (the fp32 evaluation of a case is
    made on the seam the definition chose)"""
    o, s = np.asarray(output).astype(dtype), np.asarray(sola).astype(dtype)
    n = len(s)
    if off is None:
        off = sola_cor(o, s, search, dtype)[1]
    fi = fade_in(n, dtype)
    o = o.copy()
    o[off:off + n] = o[off:off + n] * fi + s * (dtype(1) - fi)
    return off, o, o[off:off + frame].copy(), o[off + frame:off + frame + n].copy()


# ------------------------------------------------------------------------------------------------------------------------------
# converters (resample.hip.h header comment; oracle/resample_oracle.py for the taps)
# ------------------------------------------------------------------------------------------------------------------------------
def taps32(fft_in, fft_out):
    """the filter as the crate computes it, in f32: window^2 * sinc, unit sum, / (2 fft_in)"""
    return (RO.make_sinc(fft_in, RO.cutoff(fft_in, fft_out)) / np.float32(2 * fft_in)).astype(np.float32)


def taps64(fft_in, fft_out):
    """the same formula with every step in float64"""
    c = 0.4 ** (16.0 / fft_in)
    if fft_in > fft_out:
        c = c * fft_out / fft_in
    x = np.arange(fft_in, dtype=np.float64)
    w = 0.35875 - 0.48829 * np.cos(2 * np.pi * x / fft_in) + 0.14128 * np.cos(4 * np.pi * x / fft_in) - 0.01168 * np.cos(6 * np.pi * x / fft_in)
    t = (x - fft_in // 2) * c
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(t == 0, 1.0, np.sin(t * np.pi) / (t * np.pi))
    h = w * w * s
    return h / h.sum() / (2 * fft_in)


def _fft(dtype):
    return np.fft if dtype == np.float64 else sfft          # scipy keeps single precision


def resample_chunk(x, taps, fft_in, fft_out, dtype=np.float64):
    """the 2 fft_out samples of one chunk before overlap-add: zero-pad to 2 fft_in, DFT, * DFT of the taps, keep new_len bins, inverse real DFT of length 2 fft_out"""
    F = _fft(dtype)
    cdt = np.complex128 if dtype == np.float64 else np.complex64
    buf, filt = np.zeros(2 * fft_in, dtype), np.zeros(2 * fft_in, dtype)
    buf[:fft_in] = np.asarray(x).astype(dtype)
    filt[:fft_in] = np.asarray(taps).astype(dtype)
    spec = (F.rfft(buf).astype(cdt) * F.rfft(filt).astype(cdt)).astype(cdt)
    new_len = fft_in + 1 if fft_in < fft_out else fft_out
    out_f = np.zeros(fft_out + 1, cdt)
    out_f[:new_len] = spec[:new_len]
    return (F.irfft(out_f, n=2 * fft_out).astype(dtype) * dtype(2 * fft_out)).astype(dtype)       # (the crate's inverse is unnormalised)


def resample_chunk_brute(x, taps, fft_in, fft_out):
    """the same definition as two O(N^2) sums in float64 (no FFT)"""
    Lin, Lout = 2 * fft_in, 2 * fft_out
    new_len = fft_in + 1 if fft_in < fft_out else fft_out
    n, k = np.arange(fft_in)[None, :], np.arange(new_len)[:, None]
    E = np.exp(-2j * np.pi * ((k * n) % Lin) / Lin)
    S = (E @ np.asarray(x, np.float64)) * (E @ np.asarray(taps, np.float64))
    m = np.arange(Lout)[:, None]
    w = np.where(np.arange(new_len) == 0, 1.0, 2.0)
    return (np.exp(2j * np.pi * ((m * k.T) % Lout) / Lout) * (w * S)[None, :]).real.sum(axis=1)


class Resampler:
    """FftFixedInOut of one channel: process = resample_chunk + overlap-add, reset forgets the overlap"""

    def __init__(self, rate_in, rate_out, chunk, dtype=np.float64, taps=None):
        self.fft_in, self.fft_out = RO.fft_sizes(rate_in, rate_out, chunk)
        self.dtype = dtype
        self.taps = taps32(self.fft_in, self.fft_out) if taps is None else taps
        self.overlap = np.zeros(self.fft_out, dtype)

    def reset(self):
        self.overlap[:] = 0

    def process(self, x):
        assert len(x) == self.fft_in
        y = resample_chunk(x, self.taps, self.fft_in, self.fft_out, self.dtype)
        out = (y[:self.fft_out] + self.overlap).astype(self.dtype)
        self.overlap = y[self.fft_out:].copy()
        return out


def resample_run(x, rate_in, rate_out, chunk, chunks, reset_then=0, dtype=np.float64, taps=None):
    """`chunks` chunks of x, then -- reset_then -- a reset and that many chunks from the start of x again -> [chunks + reset_then][fft_out]"""
    r = Resampler(rate_in, rate_out, chunk, dtype, taps)
    fi = r.fft_in
    out = [r.process(x[c * fi:(c + 1) * fi]) for c in range(chunks)]
    if reset_then:
        r.reset()
        out += [r.process(x[c * fi:(c + 1) * fi]) for c in range(reset_then)]
    return np.stack(out)


def resample_bound(x, rate_in, rate_out, chunk, chunks, reset_then=0):
    """-> (fp64 definition with the crate's f32 taps, delta32 + tap32, peak).  tap32: what the definition moves by when the taps are evaluated in float64 (the
    engine computes its taps with the host's libm, which may differ from numpy's f32 in the last bits)"""
    fi, fo = RO.fft_sizes(rate_in, rate_out, chunk)
    r64 = resample_run(x, rate_in, rate_out, chunk, chunks, reset_then)
    d32 = float(np.abs(resample_run(x, rate_in, rate_out, chunk, chunks, reset_then, np.float32) - r64).max())
    t32 = float(np.abs(resample_run(x, rate_in, rate_out, chunk, chunks, reset_then, taps=taps64(fi, fo)) - r64).max())
    return r64, d32 + t32, float(np.abs(r64).max())


def resampler_geometry(rate_in, rate_out, chunk):
    """what a converter call launches (the arithmetic of resampler_launch, resample.hip.h, restated so that the tests can say which edges a case reaches):
    -> dict(fft_in, fft_out, P, Q, splits, n_t = outputs per residue class, per = outputs per split and class)"""
    fi, fo = RO.fft_sizes(rate_in, rate_out, chunk)
    g = gcd(rate_in, rate_out)
    P, Q = rate_in // g, rate_out // g
    Lout = 2 * fo
    per_class = (Lout + Q - 1) // Q
    per_target = 32 if Q == 1 else 64
    splits = max(1, (per_class + per_target - 1) // per_target)
    while splits > 1 and splits * Q > 4096:
        splits = (splits + 1) // 2
    n_t = [(Lout - a + Q - 1) // Q if a < Lout else 0 for a in range(Q)]
    per = [(t + splits - 1) // splits for t in n_t]
    return dict(fft_in=fi, fft_out=fo, P=P, Q=Q, splits=splits, n_t=n_t, per=per)


# ------------------------------------------------------------------------------------------------------------------------------
# rings (lib.rs:661-665, 669-679)
# ------------------------------------------------------------------------------------------------------------------------------
def ring_shift_append(ring, chunk):
    f = len(chunk)
    return np.concatenate([ring[f:], chunk])


def ring16_update(ring, res, f, skip, copy_begin):
    out = np.concatenate([ring[f:], np.zeros(f, ring.dtype)])
    out[copy_begin:] = res[skip:skip + len(ring) - copy_begin]
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_post.py
# ------------------------------------------------------------------------------------------------------------------------------
ENV_ZC = (1, 7, 16, 65)


def env_lengths(zc):
    return (zc, 5 * zc + 3, 40 * zc + 1)


def level_signal(n, seed, level=0.1):
    """samples of random sign whose magnitude stays within [0.5, 1.5] level times a slow swell: every RMS window, however short, is far from the 1e-3 floor"""
    rng = np.random.default_rng(seed)
    swell = 1.0 + 0.5 * np.sin(2 * np.pi * (np.arange(n) / max(n, 2) * 1.5 + 0.1 * seed))
    return (rng.choice([-1.0, 1.0], n) * (0.5 + rng.random(n)) * level * swell).astype(np.float32)


def env_case(zc, n, kind="plain", streams=1):
    """-> (inputs [streams][n], model outputs [streams][n]).  kind: plain; silent_out (zeros: the result is zero whatever the ratio); quiet_out (1e-5: the
    floor is active everywhere); silent_in (ratio 0); loud_quiet (stream 0 loud, the others 200 times quieter, all above the floor)"""
    xs, ys = [], []
    for s in range(streams):
        x, y = level_signal(n, 10 * zc + s, 0.1 + 0.05 * s), level_signal(n, 1000 + 10 * zc + s, 0.2 - 0.04 * s)
        if kind == "silent_out":
            y = np.zeros(n, np.float32)
        elif kind == "quiet_out":
            y = (y * np.float32(1e-4)).astype(np.float32)
        elif kind == "silent_in":
            x = np.zeros(n, np.float32)
        elif kind == "loud_quiet":
            x, y = ((x * np.float32(8), y * np.float32(4)) if s == 0 else (x * np.float32(0.5), y * np.float32(0.04)))
        xs.append(x.astype(np.float32)); ys.append(y.astype(np.float32))
    return np.stack(xs), np.stack(ys)


def env_bound(x, y, zc, exponent):
    """one stream -> (definition, r1, r2, delta32 of the result, delta32 of the tracks, peak)"""
    m64, a64, b64 = envelop_mix(x, y, zc, exponent)
    m32, a32, b32 = envelop_mix(x, y, zc, exponent, np.float32)
    return m64, a64, b64, float(np.abs(m32 - m64).max()), float(max(np.abs(a32 - a64).max(), np.abs(b32 - b64).max())), float(np.abs(m64).max())


# (sola_len, search, frame)
SOLA_CASES = [(1, 0, 1), (5, 3, 2), (63, 16, 100), (64, 1023, 64), (200, 481, 77), (1100, 30, 1025)]


def sola_case(n, search, frame, stream=0):
    """-> (output [search + frame + n], tail [n], the lag the tail's copy sits at).  Noise with a scaled, re-noised copy of the tail planted at one lag"""
    rng = np.random.default_rng(7000 + 13 * n + search + 100 * stream)
    lead = (search * (2 + stream)) // 5
    sola = (0.1 * rng.standard_normal(n)).astype(np.float32)
    if n == 1:
        sola = np.abs(sola) + np.float32(0.05)
    out = 0.05 * rng.standard_normal(search + frame + n)
    out[lead:lead + n] = 0.9 * sola + 0.004 * rng.standard_normal(n)
    return out.astype(np.float32), sola, lead


def sola_bound(output, sola, search, frame):
    """-> dict: the definition (cor, off, out, frame, tail), delta32 / peak of the correlations and of the seam, the lead of the best lag over the runner-up"""
    cor, off = sola_cor(output, sola, search)
    cor32, _ = sola_cor(output, sola, search, np.float32)
    _, out, fr, tail = sola_step(output, sola, search, frame)
    _, out32, _, _ = sola_step(output, sola, search, frame, np.float32, off=off)
    n = len(sola)
    others = np.delete(cor, off)
    return dict(cor=cor, off=off, out=out, frame=fr, tail=tail, d_cor=float(np.abs(cor32 - cor).max()), p_cor=float(np.abs(cor).max()),
                d_seam=float(np.abs(out32 - out)[off:off + n].max()), p_seam=float(np.abs(out[off:off + n]).max()),
                lead=float(cor[off] - others.max()) if len(others) else np.inf)


def sola_periodic():
    """an output of exact period 16: the windows at lags 5, 21 and 37 hold the same floats, which are 1.25 times the tail's -> three exactly equal maxima, the
    last one wins.  -> (output, tail, search, frame, the tied lags)"""
    rng = np.random.default_rng(77)
    p = (0.1 * rng.standard_normal(16)).astype(np.float32)
    n, search, frame = 48, 40, 30
    out = np.tile(p, (search + frame + n) // 16 + 1)[:search + frame + n].astype(np.float32)
    sola = (out[5:5 + n] * np.float32(0.8)).astype(np.float32)
    return out, sola, search, frame, (5, 21, 37)


def sola_zero_window(n=40, search=12, frame=50, dead=4):
    """output zero over the whole windows of the first `dead` lags (0 / sqrt(1e-8) = 0), the tail's copy behind them"""
    out, sola, lead = sola_case(n, search, frame, stream=3)
    out[:n + dead - 1] = 0
    lead = dead + 5
    out[lead:lead + n] = (np.float32(0.9) * sola).astype(np.float32)
    out[:n + dead - 1] = 0
    return out, sola, search, frame, dead


# (rate_in, rate_out, chunk).  What resampler_launch makes of each (resampler_geometry; asserted in tests/test_post_ref.py).  fft_out = chunks * Q, so the
# 2 fft_out outputs split evenly over the Q residue classes: n_t = 2 * chunks for EVERY class (n_t cannot differ between classes), and a class has fewer than 4
# outputs only when one minimal chunk is converted (RESAMPLE_MINIMAL).  splits = ceil(n_t / 64) (Q = 1: / 32), halved only further, and per = ceil(n_t / splits)
# give (splits - 1) * per < n_t: the last split can be short but never empty.
#   (300, 100, 30)     fft 30 -> 10,    P/Q 3/1, splits 1,  n_t 20
#   (100, 300, 10)     fft 10 -> 30,    P/Q 1/3, splits 1,  n_t 20
#   (100, 100, 33)     fft 33 -> 33,    P/Q 1/1, splits 3,  n_t 66,  per 22                (odd fft_in; 22 = 5 groups of 4 + 2: the t1 - 1 clamp)
#   (700, 300, 21)     fft 21 -> 9,     P/Q 7/3, splits 1,  n_t 6                          (odd fft_in; 6 = 4 + 2)
#   (300, 700, 9)      fft 9 -> 21,     P/Q 3/7, splits 1,  n_t 6                          (odd fft_in)
#   (700, 300, 280)    fft 280 -> 120,  P/Q 7/3, splits 2,  n_t 80,  per 40
#   (100, 100, 200)    fft 200 -> 200,  P/Q 1/1, splits 13, n_t 400, per 31: the last split has 28
#   (1600, 4800, 400)  fft 400 -> 1200, P/Q 1/3, splits 13, n_t 800, per 62: the last split has 56
# RESAMPLE_MINIMAL:
#   (700, 300, 7)      fft 7 -> 3,      P/Q 7/3, splits 1,  n_t 2                          (classes of 2 outputs; odd fft_in)
#   (300, 700, 3)      fft 3 -> 7,      P/Q 3/7, splits 1,  n_t 2
RESAMPLE_CASES = [(300, 100, 30), (100, 300, 10), (100, 100, 33), (700, 300, 21), (300, 700, 9), (700, 300, 7 * 40), (100, 100, 200), (1600, 4800, 400)]
RESAMPLE_MINIMAL = [(700, 300, 7), (300, 700, 3)]


def resample_signal(fft_in, chunks, seed=5):
    """voice-like, with a step inside chunk 1 (the filter's tails and the overlap carry it into chunk 2)"""
    rng = np.random.default_rng(seed)
    n = fft_in * chunks
    t = np.arange(n)
    x = 0.1 * np.sin(2 * np.pi * t / 23.0 + seed) + 0.05 * np.sin(2 * np.pi * t / 7.3) + 0.01 * rng.standard_normal(n)
    a = fft_in + fft_in // 4
    x[a:a + max(1, fft_in // 3)] += 0.5
    return x.astype(np.float32)
