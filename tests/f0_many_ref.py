"""numpy / float64 definitions behind DESIGN.md section 31: where the f0 rows of many recordings land (the grid arena and the per-file export), the segmented
select, the per-file semitone rule and which stream of which batch takes which file's transpose, on top of tests/convert_many_ref.py and tests/f0_stats_ref.py.
No GPU, no library."""
from __future__ import annotations

import numpy as np

import convert_many_ref as M
import convert_ref as R
import f0_stats_ref as S


def grid_offsets(lengths):
    """prefix sums [F + 1] of Nf_f = ceil(N_f / 160): file f's rows are [off[f], off[f + 1]) of the arena"""
    off = [0]
    for n in lengths:
        off.append(off[-1] + -(-int(n) // 160))
    return off


def export_map(lengths, sample_rate: int, k: int = 0, context: int = 0, crossfade: int = 0):
    """for every (global window g, hop row h) in packed order the arena row it is written to, or -1 (a row at or beyond the file's Nf_f: the partial last hop)
    -> int64 array (Wtot, H)"""
    geo = M.geometry(lengths, sample_rate, k, context, crossfade)
    H = R.geometry(int(lengths[0]), sample_rate, k, context, crossfade)["hop"]
    off = grid_offsets(lengths)
    rows = []
    for f, W in enumerate(geo["windows"]):
        nf = off[f + 1] - off[f]
        for w in range(W):
            j = w * H + np.arange(H)
            rows.append(np.where(j < nf, off[f] + j, -1))
    return np.array(rows, np.int64)


def scatter(lengths, window_rows, sample_rate: int, k: int = 0, context: int = 0, crossfade: int = 0, active=None):
    """the export: window_rows (Wtot, H) = the hop rows of every global window -> list of per-file arrays; windows whose `active` entry is False write nothing and
    their rows stay 0 (the silence gate)"""
    emap = export_map(lengths, sample_rate, k, context, crossfade)
    off = grid_offsets(lengths)
    arena = np.zeros(off[-1], np.float32)
    for g in range(len(emap)):
        if active is not None and not active[g]:
            continue
        keep = emap[g] >= 0
        arena[emap[g][keep]] = np.asarray(window_rows[g], np.float32)[keep]
    return [arena[off[f]: off[f + 1]] for f in range(len(lengths))]


def select_many(rows_list, quantiles=(0.5,)):
    """f0_stats_ref.select per segment -> (float32 (F, nq), list of voiced counts)"""
    res = [S.select(x, quantiles) for x in rows_list]
    return np.array([r[0] for r in res], np.float32).reshape(len(rows_list), len(quantiles)), [r[1] for r in res]


def check_pitch_list(semitones) -> bool:
    """what rvc_set_convert_many_pitch accepts as a list: every entry finite and in [-24, 24]"""
    return all(bool(np.isfinite(v)) and -24.0 <= float(v) <= 24.0 for v in semitones)


def file_semitones(listed, target, medians, voiced, step=0, limit=12.0):
    """t_f = listed[f] + a_f, a_f = f0_stats_ref.transpose(target, m_f, v_f, step, limit), 0 with the target off (0) or no voiced row; listed None = zeros
    -> (a [F], t [F]) as float64"""
    F = len(medians)
    a = np.array([S.transpose(target, float(medians[f]), int(voiced[f]), step, limit) if target > 0 else 0.0 for f in range(F)], np.float64)
    lst = np.zeros(F) if listed is None else np.asarray(listed, np.float64)
    return a, lst + a


def stream_semitones(windows, n_streams: int, t, active=None):
    """per batch the transpose of every stream: stream s of batch i holds the (i S + s)-th window that runs (all windows in global order; under the silence gate
    the active ones, compacted) and takes its file's t_f; streams beyond the last window (the padding of the last batch) take 0 -> list of lists of S floats"""
    order = [f for f, W in enumerate(windows) for _ in range(W)]
    if active is not None:
        order = [f for f, on in zip(order, active) if on]
    out = []
    for i in range(0, len(order), n_streams):
        fs = order[i: i + n_streams]
        out.append([float(t[f]) for f in fs] + [0.0] * (n_streams - len(fs)))
    return out


def self_check() -> None:
    H = 54
    lengths = [1, 320 * H + 1, 160 * H, 160 * H + 1]
    assert grid_offsets(lengths) == [0, 1, 110, 164, 219]
    emap = export_map(lengths, 4800, 2, 3, 2)
    assert emap.shape == (7, H)
    assert emap[0].tolist() == [0] + [-1] * (H - 1)                         # the one-row file: nothing spills into file 1
    assert emap[3, 0] == 1 + 2 * H and emap[3, 1] == -1                     # file 1's third window holds one row
    assert emap[4].tolist() == list(range(110, 164))                        # a file of exactly one hop
    written = emap[emap >= 0]
    assert sorted(written.tolist()) == list(range(219))                     # every row exactly once
    assert stream_semitones([1, 3, 1, 2], 3, [0, 3, -5, 12]) == [[0, 3, 3], [3, -5, 12], [12, 0, 0]]
    assert stream_semitones([1, 3, 1, 2], 3, [0, 3, -5, 12], active=[True, True, False, True, True, False, True]) == [[0, 3, 3], [-5, 12, 0]]
