"""Formant shift (the plugin's resonance shift): the host-side pieces of the definition in DESIGN.md "Formant shift" -- the geometry
(rvc_formant_geometry), the resampler's filter table (rvc_debug_formant_table) and the numpy restatements the GPU tests
(test_gpu_formant.py) compare the device against.  No GPU needed."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest
import torch

from obs_rvc_amd import _native
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError


# ---- numpy restatements of the definition (also used by tests/test_gpu_formant.py) ----------------------------------------------
def geometry(R: int, sr: int, phi: float):
    f = 2.0 ** (phi / 12.0)
    return math.ceil(R * f), math.floor(f * sr / 100)


def table(o: int, n: int):
    """h[j][k] of the resampler o -> n (fp64 arithmetic, fp32 result), its left width w and row length K."""
    b = 0.99 * min(o, n)
    w = math.ceil(6 * o / b)
    K = 2 * w + o
    k = np.arange(K, dtype=np.float64)
    j = np.arange(n, dtype=np.float64)[:, None]
    t = np.clip(((k - w) / o - j / n) * b, -6.0, 6.0)
    h = np.sinc(t) * np.cos(np.pi * t / 12.0) ** 2 * b / o
    return h.astype(np.float32), w, K


def resample(x, o: int, n: int, nout: int) -> np.ndarray:
    """y[q n + j] = sum_k h[j][k] x[q o + k - w], x zero outside its range (fp64 sums of the fp32 table)."""
    h, w, K = table(o, n)
    h = h.astype(np.float64)
    x = np.asarray(x, np.float64)
    qmax = (nout + n - 1) // n
    xp = np.concatenate([np.zeros(w), x, np.zeros(max(0, qmax * o + K - w - len(x)))])
    y = np.empty(qmax * n)
    for q in range(qmax):
        y[q * n:(q + 1) * n] = h @ xp[q * o:q * o + K]
    return y[:nout]


def back_to_model_rate(y2, R: int, upp: int, upp_res: int) -> np.ndarray:
    """Step 6 of the definition: the decoder output y2 (R2 upp samples) -> R upp samples."""
    if upp_res == upp:
        return np.asarray(y2[:R * upp], np.float64)
    g = math.gcd(upp_res, upp)
    return resample(np.asarray(y2[:R * upp_res]), upp_res // g, upp // g, R * upp)


def interp(x: np.ndarray, nout: int, dtype=np.float32) -> np.ndarray:
    """Linear interpolation along the last axis, F.interpolate(mode="linear", align_corners=False), in `dtype` (the device: fp32)."""
    dt = dtype
    x = np.asarray(x, dt)
    nin = x.shape[-1]
    s = dt(nin) / dt(nout)
    i = np.arange(nout, dtype=dt)
    xs = np.maximum(s * (i + dt(0.5)) - dt(0.5), dt(0))
    i0 = np.minimum(xs.astype(np.int64), nin - 1)
    i1 = i0 + (i0 < nin - 1)
    lam = np.clip(xs - i0.astype(dt), dt(0), dt(1))
    return (dt(1) - lam) * x[..., i0] + lam * x[..., i1]


# ---- the library's host-side entry points -------------------------------------------------------------------------------------
def _lib_geometry(R, sr, phi):
    L = _native.lib()
    out = (C.c_size_t * 2)()
    rc = L.rvc_formant_geometry(R, sr, phi, out)
    return rc, (int(out[0]), int(out[1]))


def test_geometry_matches_formula_over_the_grid():
    phis = np.round(np.arange(-500, 501) / 100.0, 2)
    for sr in (48000, 40000, 32000, 6400, 4800):
        for R in (1, 16, 21, 37, 512):
            for phi in phis:
                rc, got = _lib_geometry(R, sr, float(phi))
                assert rc == 0 and got == geometry(R, sr, float(phi)), (R, sr, phi, got)
            assert _lib_geometry(R, sr, 0.0)[1] == (R, sr // 100)


@pytest.mark.parametrize("phi,R2,upp_res", [(0.07, 22, 481), (-0.07, 21, 478), (0.01, 22, 480), (3.5, 26, 587), (5, 29, 640), (-5, 16, 359)])
def test_geometry_examples(phi, R2, upp_res):
    assert _lib_geometry(21, 48000, phi) == (0, (R2, upp_res))
    assert RvcInfer.formant_geometry(21, 48000, phi) == (R2, upp_res)


@pytest.mark.parametrize("phi", [5.01, -5.01, float("nan"), float("inf")])
def test_geometry_rejects_out_of_range(phi):
    assert _lib_geometry(21, 48000, phi)[0] == 5          # RVC_SHAPE
    with pytest.raises(RvcInferError):
        RvcInfer.formant_geometry(21, 48000, phi)


@pytest.mark.parametrize("o,n", [(481, 480), (4, 3), (359, 480), (587, 480), (83, 96)])
def test_filter_table_matches_restatement(o, n):
    L = _native.lib()
    ref, w, K = table(o, n)
    width = C.c_size_t()
    assert L.rvc_debug_formant_table(o, n, None, 0, C.byref(width)) == 1 and width.value == K
    out = np.zeros(n * K, np.float32)
    assert L.rvc_debug_formant_table(o, n, out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(width)) == 0
    assert np.abs(out.reshape(n, K) - ref).max() <= 1e-7
    # the rows are normalised low-pass filters: each phase sums to ~1 (DC gain)
    assert np.abs(ref.astype(np.float64).sum(1) - 1.0).max() < 2e-3


@pytest.mark.parametrize("o,n", [(481, 480), (4, 3), (359, 480), (587, 480), (83, 96)])
def test_resampler_restatement_reproduces_a_bandlimited_signal(o, n):
    # pins the formula by what it must do, independently of any memory of torchaudio: a multi-sine sampled at rate o, resampled to
    # rate n, equals the same signal sampled at rate n away from the ends.  The Hann window of width 6 has a wide transition band:
    # partials up to 0.2 min(o, n) stay within 1e-3 (at 0.45 min(o, n) the error is ~7 %, the filter's own roll-off).
    units = max(3, 4000 // max(o, n))
    rng = np.random.default_rng(o * 1000 + n)
    fr = np.linspace(0.02, 0.2, 7) * min(o, n)
    ph = rng.uniform(0, 2 * np.pi, 7)

    def sig(t):
        return sum(np.sin(2 * np.pi * f * t + p) for f, p in zip(fr, ph)) / 7

    y = resample(sig(np.arange(units * o) / o), o, n, units * n)
    ref = sig(np.arange(units * n) / n)
    lo, hi = int(0.2 * len(y)), int(0.8 * len(y))
    assert np.abs(y - ref)[lo:hi].max() < 1e-3


@pytest.mark.parametrize("nin,nout", [(21, 22), (21, 29), (21, 16), (10080, 10560), (10080, 7680), (7, 7), (1, 5)])
def test_interpolation_restatement_matches_torch(nin, nout):
    x = np.random.default_rng(nin + nout).standard_normal((3, nin))
    ref = torch.nn.functional.interpolate(torch.from_numpy(x)[None], size=nout, mode="linear", align_corners=False)[0].numpy()
    assert np.abs(interp(x, nout, np.float64) - ref).max() <= 1e-7
    # in fp32 both round the source position s (i + 1/2) - 1/2 in their own way: equal in the small, a few 1e-4 apart at sample ~10^4 of
    # white noise (the latent and the source are smooth, and the GPU test compares at 1e-4 relative RMS)
    x32 = x.astype(np.float32)
    ref32 = torch.nn.functional.interpolate(torch.from_numpy(x32)[None], size=nout, mode="linear", align_corners=False)[0].numpy()
    assert np.sqrt(np.mean((interp(x32, nout) - ref32).astype(np.float64) ** 2)) <= 1e-4 * max(1e-12, np.sqrt(np.mean(ref32.astype(np.float64) ** 2)))
