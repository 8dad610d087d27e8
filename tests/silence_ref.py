"""The definition of the file converter's silence gate (obs_rvc_amd/csrc/silence.hip.h) in numpy / float64.

All lengths in 10 ms frames of 160 samples at 16 kHz.  x is the signal the model sees, zero-extended beyond [0, N); Nf = ceil(N / 160).
  loud[i]    sumsq(x[160 i, 160 i + 640)) >= 640 max(10^(threshold_db / 10), 1e-10)      (= 20 log10(max(rms, 1e-5)) >= threshold_db, the session gate's measure)
  kept[i]    some loud j with |i - j| <= hang
  active[w]  a kept frame in [w H, w H + H + X + Q) n [0, Nf), W = ceil(Nf / H), H = 32 k - 1 - 2 C - X - Q, Q = 1
  place[w]   the rank of w among the active windows (-1: skipped): the j-th active window runs on stream j % S of batch j / S
A skipped window enters the stitch as (H + X + Q) zc zeros."""
from __future__ import annotations

import numpy as np

FRAME, SPAN, Q = 160, 640, 1


def n_frames(n: int) -> int:
    return -(-int(n) // FRAME)


def threshold_linear(threshold_db: float) -> float:
    return 640.0 * max(10.0 ** (float(threshold_db) / 10.0), 1e-10)


def frame_energy(x) -> np.ndarray:
    """sumsq of the 640 samples from each frame's start on, float64 (160-sample block sums, four of them per frame)"""
    x = np.asarray(x, np.float64)
    nf = n_frames(len(x))
    pad = np.zeros((nf + 3) * FRAME, np.float64)
    pad[: len(x)] = x
    bs = (pad.reshape(nf + 3, FRAME) ** 2).sum(axis=1)
    return bs[0:nf] + bs[1: nf + 1] + bs[2: nf + 2] + bs[3: nf + 3]


def loud_frames(x, threshold_db: float) -> np.ndarray:
    return frame_energy(x) >= threshold_linear(threshold_db)


def margin(x, threshold_db: float) -> float:
    """the smallest relative distance of a frame's energy from the threshold: exact comparison of two float64 evaluations is fair when this is far above 1e-16"""
    t = threshold_linear(threshold_db)
    return float(np.min(np.abs(frame_energy(x) - t)) / t)


def kept_frames(loud, hang: int) -> np.ndarray:
    loud = np.asarray(loud, bool)
    nf = len(loud)
    cnt = np.concatenate([[0], np.cumsum(loud)])                     # cnt[i] = loud frames in [0, i)
    i = np.arange(nf)
    hi = np.minimum(i + hang, nf - 1) + 1
    lo = np.maximum(i - hang, 0)
    return (cnt[hi] - cnt[lo]) > 0


def hop(k: int, context: int, crossfade: int) -> int:
    return 32 * k - 1 - 2 * context - crossfade - Q


def active_windows(kept, H: int, R: int) -> np.ndarray:
    kept = np.asarray(kept, bool)
    nf = len(kept)
    W = -(-nf // H)
    return np.array([bool(kept[w * H: min(w * H + R, nf)].any()) for w in range(W)], bool)


def places(active) -> np.ndarray:
    active = np.asarray(active, bool)
    p = np.cumsum(active) - 1
    return np.where(active, p, -1).astype(np.int32)


def analyze(x, threshold_db: float, hang: int, k: int, context: int, crossfade: int) -> dict:
    H = hop(k, context, crossfade)
    R = H + crossfade + Q
    loud = loud_frames(x, threshold_db)
    kept = kept_frames(loud, hang)
    act = active_windows(kept, H, R)
    return {"loud": loud, "kept": kept, "active": act, "place": places(act), "H": H, "R": R, "windows": len(act)}


def analyze_flags(loud, hang: int, H: int, X: int) -> dict:
    """the same from loud flags alone (the invariants do not need a signal)"""
    kept = kept_frames(loud, hang)
    act = active_windows(kept, H, H + X + Q)
    return {"loud": np.asarray(loud, bool), "kept": kept, "active": act, "place": places(act)}


def insert_zero_windows(y_active, place, window_len: int) -> np.ndarray:
    """the stitch's input: row w = the output of active window w (row place[w] of y_active), or zeros for a skipped one"""
    place = np.asarray(place)
    out = np.zeros((len(place), window_len), np.float32)
    for w, p in enumerate(place):
        if p >= 0:
            out[w] = y_active[p]
    return out


def check_args(threshold_db: float, hang: int) -> bool:
    return threshold_db == threshold_db and 0 <= int(hang) <= 1000


def is_on(threshold_db: float) -> bool:
    return threshold_db > -60.0
