"""Hybrid f0 (include/rvc_mi355x.h rvc_load_f0_hybrid) as a numpy float32 definition: what f0_hybrid_kernel must produce, bit for bit.

rows: (n, ...) float32, one row per member in the caller's order, rows[0] the lead's; n = 1..4.  A member is VOICED on a frame iff its value is > 0 (NaN and
negative values are unvoiced).  With v of the n members voiced on a frame:
  VOTE (0)    voiced iff 2 v > n, or 2 v == n and the lead is voiced; an unvoiced frame gives 0, a voiced one the median of the v voiced values
  MEDIAN (1)  the median of all n values, unvoiced ones entering as 0
The median of an even count is float32(0.5) * (a + b) of the two middle values, a <= b, the sum rounded to float32 first.
Written frame by frame with Python's sorted(): slow and plain on purpose; the tests use at most a few thousand frames."""
from __future__ import annotations

import numpy as np

VOTE, MEDIAN = 0, 1
MAX_MEMBERS = 4


def median32(vals) -> np.float32:
    """the median of 1 or more float32 values (no NaN among them) under the even rule above"""
    s = sorted(np.float32(v) for v in vals)
    c = len(s)
    if c % 2:
        return s[c // 2]
    return np.float32(np.float32(0.5) * np.float32(s[c // 2 - 1] + s[c // 2]))


def combine_frame(vals, mode: int) -> np.float32:
    vals = [np.float32(v) for v in vals]
    n = len(vals)
    assert 1 <= n <= MAX_MEMBERS and mode in (VOTE, MEDIAN)
    voiced = [bool(v > 0) for v in vals]          # (NaN > 0 is False)
    v = sum(voiced)
    if mode == MEDIAN:
        return median32([x if on else np.float32(0) for x, on in zip(vals, voiced)])
    if 2 * v > n or (2 * v == n and voiced[0]):
        return median32([x for x, on in zip(vals, voiced) if on])
    return np.float32(0)


def combine(rows, mode: int = VOTE) -> np.ndarray:
    """rows (n, ...) -> (...) float32"""
    rows = np.asarray(rows, np.float32)
    n, shape = rows.shape[0], rows.shape[1:]
    flat = rows.reshape(n, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.array([combine_frame(flat[:, i], mode) for i in range(flat.shape[1])], np.float32)
    return out.reshape(shape)


def frame_class(vals) -> str:
    """the case a frame of n member values falls in (the GPU test asserts that its hand-built rows reach every one)"""
    vals = [np.float32(v) for v in vals]
    n, voiced = len(vals), [bool(v > 0) for v in vals]
    v = sum(voiced)
    if v == n:
        return "all_voiced_odd" if n % 2 else "all_voiced_even"
    if v == 0:
        return "all_unvoiced"
    if 2 * v == n:
        return "tie_lead_voiced" if voiced[0] else "tie_lead_unvoiced"
    return "majority_voiced" if 2 * v > n else "majority_unvoiced"
