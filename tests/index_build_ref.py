"""The windowing of the index builder (obs_rvc_amd/csrc/retrieval.hip index_build_add) restated in numpy / plain Python, for
tests/test_index_build_ref.py (CPU) and tests/test_gpu_index_build.py.

Definition.  A recording of n samples at 16 kHz and a window of w samples: runs (start, length) = (0, w), (w, w), ... for every full window, then the tail
(n - n % w, n % w) when n % w > 0.  A run of L samples yields ContentVec's frame count: seven valid convolutions, kernels (10, 3, 3, 3, 3, 2, 2) and strides
(5, 2, 2, 2, 2, 2, 2), L <- (L - k) // s + 1 each, 0 as soon as L < k.  That is 0 below the receptive field of 400 samples and (L - 400) // 320 + 1 from
there on.  A tail with 0 frames is dropped silently; a run contributes its frames as rows in time order; nothing carries from one recording to the next."""
from __future__ import annotations

import numpy as np

CONV_K = (10, 3, 3, 3, 3, 2, 2)
CONV_S = (5, 2, 2, 2, 2, 2, 2)
RECEPTIVE_FIELD = 400
HOP = 320
DEFAULT_WINDOW = 48000


def frames(length: int) -> int:
    """ContentVec's frame rule (ModelCV::out_frames)"""
    t = int(length)
    for k, s in zip(CONV_K, CONV_S):
        if t < k:
            return 0
        t = (t - k) // s + 1
    return t


def runs(n: int, w: int = DEFAULT_WINDOW):
    """-> (list of (start, length, frames) of the runs that contribute rows, length of the dropped tail or None)"""
    assert w >= RECEPTIVE_FIELD and n >= 0
    out = [(s, w, frames(w)) for s in range(0, n - w + 1, w)]
    tail = n % w
    if tail == 0:
        return out, None
    if frames(tail) < 1:
        return out, tail
    return out + [(n - tail, tail, frames(tail))], None


def total_rows(lengths, w: int = DEFAULT_WINDOW) -> int:
    return sum(f for n in lengths for _, _, f in runs(n, w)[0])


def rows_of(recordings, w, hubert):
    """the rows a build holds after adding `recordings` (1-D arrays), from a hubert(x) -> (1, C, T) callable: [rows][C]"""
    out = []
    for x in recordings:
        for s, ln, f in runs(len(x), w)[0]:
            h = np.asarray(hubert(x[s:s + ln]))
            assert h.shape[0] == 1 and h.shape[2] == f
            out.append(np.ascontiguousarray(h[0].T))
    return np.concatenate(out, axis=0)
