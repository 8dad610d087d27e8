"""Consonant protection (rvc_set_protect, csrc/protect.hip.h) restated in float64 numpy.

Per stream, p = (float)protect in [0, 0.5], 0.5 = off.  Row r of a call is unvoiced iff pitchf[r] < 1.0f.  On unvoiced rows, for every channel c,
    phone[c][r] = p * phone[c][r] + (1 - p) * raw[c][r],
where raw[c][r] is the ContentVec feature the row had before the retrieval blended into it: column min((skip_head + r) / 2, T - 1) of the ContentVec output
[C][T] (integer division; the feature sequence is every column twice plus the last column once more, 2 T + 1 rows, and the call takes rows
skip_head .. skip_head + R).  Voiced rows and streams at 0.5 keep their values.  The column rule is restated here from that text, not taken from the engine."""
from __future__ import annotations

import numpy as np

OFF = 0.5
# The device forms p * blend, q * raw, their sum and q = 1 - p in float: four roundings of 2^-24 relative each, bounded by 4 * 2^-24 of the term magnitudes;
# a factor 2 on top covers a contracted (fma) against an uncontracted evaluation.
BOUND_FACTOR = 2.0 ** -21


def src_col(skip_head: int, r: int, T: int) -> int:
    """the ContentVec column behind row r of a call's phone rows"""
    return min((skip_head + r) // 2, T - 1)


def raw_rows(cv, skip_head: int, R: int):
    """cv [C][T] -> the raw phone rows [C][R] of a call"""
    cv = np.asarray(cv)
    T = cv.shape[1]
    assert skip_head >= 0 and R >= 1 and skip_head + R <= 2 * T + 1
    return cv[:, [src_col(skip_head, r, T) for r in range(R)]]


def unvoiced(pitchf):
    return np.asarray(pitchf, np.float32) < np.float32(1.0)


def protect_mix(phone, cv, pitchf, p, skip_head: int):
    """phone [C][R] (blended), cv [C][T], pitchf [R], p -> (expected phone [C][R] in float64, per-element bound [C][R], unvoiced mask [R]).
    Elements the definition leaves alone come back as they went in, with bound 0."""
    phone = np.asarray(phone)
    C, R = phone.shape
    out = phone.astype(np.float64)
    bound = np.zeros((C, R))
    uv = unvoiced(pitchf)
    assert uv.shape == (R,)
    pf = float(np.float32(p))
    if not pf < OFF:
        return out, bound, np.zeros(R, bool)
    raw = raw_rows(cv, skip_head, R).astype(np.float64)
    a, b = pf * out[:, uv], (1.0 - pf) * raw[:, uv]
    out[:, uv] = a + b
    bound[:, uv] = BOUND_FACTOR * (np.abs(a) + np.abs(b))
    return out, bound, uv
