"""The numpy definitions behind DESIGN.md section 28: exact order statistics of the voiced rows of an f0 track, the auto-transpose rule, the merge of a curve
into the tracked rows, and the inputs of the select kernel's GPU tests (tests/test_gpu_f0_stats.py).  No GPU, no project import."""
from __future__ import annotations

import math

import numpy as np

QUANTILES = (0.0, 0.05, 0.5, 0.95, 1.0)


def voiced_mask(x):
    x = np.asarray(x, np.float32)
    return np.isfinite(x) & (x > 0)


def select(x, quantiles=(0.5,)):
    """-> (float32 [len(quantiles)], v): quantile p of the v voiced rows is sorted[floor(p (v - 1))], the product in double; zeros when v = 0"""
    x = np.asarray(x, np.float32)
    s = np.sort(x[voiced_mask(x)])
    v = len(s)
    if v == 0:
        return np.zeros(len(quantiles), np.float32), 0
    return np.array([s[int(math.floor(float(p) * float(v - 1)))] for p in quantiles], np.float32), v


def round_clamp(a, step=1, limit=12.0):
    """step > 0: step * rint(a / step), ties to even; then clamped to [-limit, limit]"""
    a = float(a)
    if step > 0:
        a = step * float(np.rint(a / step))
    return min(max(a, -float(limit)), float(limit))


def transpose(target, median, voiced, step=1, limit=12.0):
    """a = 12 log2(target / median) in double, through round_clamp; no voiced row: 0"""
    if voiced == 0 or not median > 0:
        return 0.0
    return round_clamp(12.0 * math.log2(float(target) / float(median)), step, limit)


def factor(a):
    """the multiplier a transpose of a semitones adds: (float)2^(a / 12), nothing (None) at a = 0"""
    return None if a == 0 else np.float32(2.0 ** (a / 12.0))


def merge(curve, tracked):
    """row j = isnan(curve j) ? tracked j : curve j"""
    curve, tracked = np.asarray(curve, np.float32), np.asarray(tracked, np.float32)
    return np.where(np.isnan(curve), tracked, curve).astype(np.float32)


def check_auto_transpose_args(target_hz, step, limit):
    """what rvc_set_auto_transpose accepts"""
    return bool(0.0 <= target_hz <= 20000.0 and step in (0, 1, 12) and 0.0 <= limit <= 24.0)


def select_inputs(n, seed=0):
    """the select kernel's test inputs at n rows -> {name: float32 [n]}"""
    r = np.random.default_rng(1000 + n + seed)
    out = {}
    out["all unvoiced"] = np.zeros(n, np.float32)
    one = np.zeros(n, np.float32); one[n // 2] = np.float32(220.5)
    out["one voiced row"] = one
    out["all rows equal"] = np.full(n, np.float32(311.127), np.float32)
    a = np.float32(196.0); b = np.nextafter(a, np.float32(np.inf))
    two = np.where(np.arange(n) % 2 == 0, b, a).astype(np.float32)
    if n % 2:
        two[-1] = 0.0          # equal counts
    out["two values one ulp apart"] = r.permutation(two)
    den = r.uniform(80.0, 400.0, n).astype(np.float32); den[r.integers(0, n)] = np.float32(1e-41)
    assert 0 < np.float32(1e-41) < np.finfo(np.float32).tiny
    out["a positive denormal among normal values"] = den
    mix = r.uniform(80.0, 400.0, n).astype(np.float32)
    kinds = r.integers(0, 5, n)
    mix[kinds == 0] = np.nan; mix[kinds == 1] = np.inf; mix[kinds == 2] = -mix[kinds == 2]
    if n >= 4:
        mix[:4] = (np.nan, np.inf, -np.inf, -0.0)
    out["NaN, +inf and negative rows"] = mix
    lu = np.exp(r.uniform(np.log(50.0), np.log(1100.0), n)).astype(np.float32)
    lu[r.random(n) < 0.4] = 0.0
    out["log-uniform 50-1100 Hz, 40 % zeros"] = lu
    return out
