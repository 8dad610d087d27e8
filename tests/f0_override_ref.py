"""f0 from outside restated in numpy: the definition the kernels of obs_rvc_amd/csrc/f0_override.hip.h are held against.

Override rows.  ov[0 .. Tm) per stream and call, NaN = "keep the tracker's value": f[t] = ov[t] if ov[t] is not NaN else f[t], in front of step 1 of section 12.
A stream hands in n <= Tm rows for the END of the window: row i of n is window row Tm - n + i, the rows in front of them are NaN.

Curve -> grid.  n >= 1 breakpoints (t_i seconds strictly increasing, hz_i = 0 or in (0, 20000]); grid row j stands for j / 100 s.  Times are compared as
T_i = 100 t_i (one rounded double product).  If T_0 <= j <= T_{n-1}, with i the last index with T_i <= j: the last breakpoint gives hz_i; next to a 0 the row is
the nearer breakpoint's value, (j - T_i) <= (T_{i+1} - j) choosing i (both differences in double); else
    u = (float)(j - T_i) / (float)(T_{i+1} - T_i),   row = fma(hz_{i+1} - hz_i, u, hz_i)          (differences of times in double, everything else in float)
Every other row is NaN.  `dtype` is the precision of u and of the lerp: float64 is the reference, float32 the same recipe as numpy rounds it (no fma).

Windows of a conversion (geometry k, C, X of section 19: F = 32 k - 1, H = F - 2 C - X - 1, Tm = 32 k, window w reads samples [160 (w H - C), + 160 F)): the f0
front end takes all 160 F samples and reflect-pads them by 512, frame t covers padded samples [160 t, 160 t + 1024), so row t is centred on sample 160 t of the
window = sample 160 (w H - C + t) of the recording = grid row w H - C + t; NaN outside [0, Nf).  A window's pitch rows [C, C + H) are the hop it contributes: grid
frame g is row C + g mod H of window g div H."""
from __future__ import annotations

import numpy as np

MAX_HZ = 20000.0
MAX_ROWS = 1024


def check_values(hz, nan_ok):
    """-> None, or what is wrong with override / curve values"""
    hz = np.asarray(hz, np.float64)
    if not nan_ok and np.any(np.isnan(hz)):
        return "NaN"
    v = hz[~np.isnan(hz)]
    if np.any(~np.isfinite(v)) or np.any(v < 0) or np.any(v > MAX_HZ):
        return "a value is negative, infinite or above 20000 Hz"
    return None


def check_curve(t, hz):
    t = np.asarray(t, np.float64)
    if len(t) < 1 or len(t) != len(hz):
        return "needs n >= 1 pairs"
    if not np.all(np.isfinite(t)):
        return "a time is not finite"
    if np.any(np.diff(t) <= 0):
        return "times must be strictly increasing"
    return check_values(hz, False)


def align_end(rows, Tm):
    """n override rows for the end of a window of Tm rows -> ov [Tm]"""
    rows = np.asarray(rows, np.float32)
    assert len(rows) <= Tm
    ov = np.full(Tm, np.nan, np.float32)
    if len(rows):
        ov[Tm - len(rows):] = rows
    return ov


def select(f, ov):
    """pure selection, bit for bit"""
    f, ov = np.asarray(f, np.float32), np.asarray(ov, np.float32)
    return np.where(np.isnan(ov), f, ov).astype(np.float32)


def curve_grid(t, hz, Nf, dtype=np.float64):
    t = np.asarray(t, np.float64)
    hz = np.asarray(hz, np.float32)
    assert check_curve(t, hz) is None
    T = 100.0 * t
    out = np.full(Nf, np.nan, dtype)
    for j in range(Nf):
        x = float(j)
        if not (T[0] <= x <= T[-1]):
            continue
        i = int(np.searchsorted(T, x, side="right")) - 1          # the last index with T_i <= j
        if i == len(T) - 1:
            out[j] = hz[i]
            continue
        h0, h1 = hz[i], hz[i + 1]
        a, b = x - T[i], T[i + 1] - x
        if h0 == 0 or h1 == 0:
            out[j] = h0 if a <= b else h1
        else:
            u = dtype(a) / dtype(T[i + 1] - T[i])
            out[j] = dtype(h0) + (dtype(h1) - dtype(h0)) * u
    return out


def grid_margin(t, Nf):
    """the smallest relative distance |j - T_i| / max(j, 1) between a grid time and a breakpoint time that is not exactly on it (inf if none)"""
    T = 100.0 * np.asarray(t, np.float64)
    j = np.arange(Nf, dtype=np.float64)
    d = np.abs(j[:, None] - T[None, :])
    rel = d / np.maximum(j, 1.0)[:, None]
    rel = rel[d > 0]
    return float(rel.min()) if rel.size else float("inf")


def geometry(k, C, X, Nf):
    """the window geometry of a conversion in frames (section 19) -> dict"""
    F = 32 * k - 1
    H = F - 2 * C - X - 1
    assert k >= 2 and C >= 3 and H >= X
    return {"k": k, "C": C, "X": X, "F": F, "H": H, "Tm": 32 * k, "Nf": Nf, "W": -(-Nf // H)}


def row_frame(g, w, t):
    """the grid frame row t of window w is centred on (may lie outside [0, Nf))"""
    return w * g["H"] - g["C"] + t


def window_override(grid, g, w):
    """the override rows [Tm] of window w; a window at or beyond W (padding) gets NaN rows"""
    ov = np.full(g["Tm"], np.nan, np.float32)
    if w >= g["W"]:
        return ov
    fr = row_frame(g, w, np.arange(g["Tm"]))
    ok = (fr >= 0) & (fr < g["Nf"])
    ov[ok] = np.asarray(grid, np.float32)[fr[ok]]
    return ov


def export(rows, g):
    """rows [W][Tm], the conditioned rows of every window -> the grid [Nf], and how often each frame was written"""
    rows = np.asarray(rows, np.float32)
    out = np.full(g["Nf"], np.nan, np.float32)
    hits = np.zeros(g["Nf"], np.int64)
    for w in range(rows.shape[0]):
        for h in range(g["H"]):
            fr = w * g["H"] + h
            if fr < g["Nf"]:
                out[fr] = rows[w, g["C"] + h]
                hits[fr] += 1
    return out, hits


def gpu_curves():
    """the curves of tests/test_gpu_f0_override.py: (t, hz) of 1, 2 and 40 breakpoints, zeros among them; times that are not dyadic sit well off the grid"""
    one = (np.array([0.5]), np.array([220.0], np.float32))
    two = (np.array([0.25, 2.75]), np.array([110.0, 330.0], np.float32))
    rng = np.random.default_rng(27)
    t = np.cumsum(rng.uniform(0.031, 0.123, 40)) + 0.0137
    t[7] = 0.5; t[20] = 1.75          # breakpoints exactly on grid times
    t = np.sort(t)
    hz = rng.uniform(80.0, 600.0, 40).astype(np.float32)
    hz[[3, 4, 11, 25, 39]] = 0.0
    assert np.all(np.diff(t) > 0)
    return [one, two, (t, hz)]
