"""numpy definitions of the host-visible arithmetic of rvc_convert_many: the packing of the windows of several recordings into
batches, the per-file window gather and the per-file SOLA stitch, on top of tests/convert_ref.py.  No GPU, no library."""
from __future__ import annotations

import numpy as np

import convert_ref as R

MAX_FILES = 65536
MAX_WINDOWS = 1 << 30
MAX_OUT = 1 << 40


def geometry(lengths, sample_rate: int, k: int = 0, context: int = 0, crossfade: int = 0):
    """the packing rule of include/rvc_mi355x.h restated -> dict, or None where the engine answers RVC_SHAPE"""
    lengths = [int(n) for n in lengths]
    if not 1 <= len(lengths) <= MAX_FILES or any(n < 1 for n in lengths):
        return None
    per = [R.geometry(n, sample_rate, k, context, crossfade) for n in lengths]
    if any(g is None for g in per):
        return None
    out = {"windows": [g["windows"] for g in per], "output_samples": [g["output_samples"] for g in per]}
    out["windows_total"], out["output_total"] = sum(out["windows"]), sum(out["output_samples"])
    if out["windows_total"] > MAX_WINDOWS or out["output_total"] > MAX_OUT:
        return None
    return out


def packing(windows, S: int):
    """the batches of a call: windows = W_f per file, S streams -> list of batches, each the list of (f, w) its streams 0 .. run, in order.  Global window
    g = P_f + w; batch i holds globals [i S, min((i + 1) S, Wtot)): only the last one is short"""
    order = [(f, w) for f, W in enumerate(windows) for w in range(W)]
    return [order[i: i + S] for i in range(0, len(order), S)]


def gather_windows_many(signals, sample_rate: int, k: int, context: int, crossfade: int):
    """per file, the (W_f, n) windows of convert_ref.gather_windows: zeros outside the file, whatever lies next to it"""
    return [R.gather_windows(np.asarray(x, np.float32), R.geometry(len(x), sample_rate, k, context, crossfade)) for x in signals]


def stitch_many(windows, windows_per_file, sola_len: int, search: int, frame: int, offsets=None):
    """the chained LINEAR SOLA step per file over windows (Wtot, window_len) laid end to end, every file's tail starting as zeros ->
    (audio (Wtot frame,), offsets (Wtot,)); offsets given: blend at those"""
    y = np.asarray(windows, np.float64)
    assert y.ndim == 2 and sum(windows_per_file) == y.shape[0] and all(w >= 1 for w in windows_per_file)
    fi = R.fade_in(sola_len)
    out, offs, g = [], [], 0
    for W in windows_per_file:
        tail = np.zeros(sola_len)
        for _ in range(W):
            off = R.sola_offset(y[g], tail, search) if offsets is None else int(offsets[g])
            seg = y[g, off: off + frame + sola_len].copy()
            seg[:sola_len] = seg[:sola_len] * fi + tail * (1.0 - fi)
            tail = seg[frame: frame + sola_len].copy()
            out.append(seg[:frame]); offs.append(off)
            g += 1
    return np.concatenate(out), np.array(offs, np.int32)


def self_check() -> None:
    # the issue's case: W = {1, 3, 1, 2} at S = 3 is three batches, the second with three files in it, the last with one window
    assert packing([1, 3, 1, 2], 3) == [[(0, 0), (1, 0), (1, 1)], [(1, 2), (2, 0), (3, 0)], [(3, 1)]]
    assert packing([1, 3, 1, 2], 1) == [[p] for p in [(0, 0), (1, 0), (1, 1), (1, 2), (2, 0), (3, 0), (3, 1)]]
    assert [len(b) for b in packing([3] * 64, 32)] == [32] * 6 and [len(b) for b in packing([3] * 64, 8)] == [8] * 24
    g = geometry([1, 320 * 54 + 1, 160 * 54, 160 * 54 + 1], 4800, 2, 3, 2)
    assert g == {"windows": [1, 3, 1, 2], "output_samples": [48, 109 * 48, 54 * 48, 55 * 48], "windows_total": 7, "output_total": 219 * 48}
    # a neighbour never leaks into a gather: the windows of a file are those of the file alone
    a, b = np.full(700, 5.0, np.float32), np.full(300, -7.0, np.float32)
    wa, wb = gather_windows_many([a, b], 4800, 2, 3, 2)
    assert wa.shape == (1, 10080) and set(np.unique(wa)) == {0.0, 5.0} and set(np.unique(wb)) == {0.0, -7.0}
    assert np.all(wa[0, 480: 1180] == 5.0) and np.all(wa[0, 1180:] == 0.0) and np.all(wb[0, :480] == 0.0)
