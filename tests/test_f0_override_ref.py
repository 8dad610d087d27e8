"""tests/f0_override_ref.py on answers known by hand, and the margins tests/test_gpu_f0_override.py relies on.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import f0_override_ref as O

nan = np.nan


def _eq(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_select_and_end_alignment():
    f = np.array([100.0, 0.0, nan, 250.0, 300.0], np.float32)
    ov = O.align_end([nan, 0.0, 440.0], 5)
    assert _eq(ov, [nan, nan, nan, 0.0, 440.0])
    assert _eq(O.select(f, ov), [100.0, 0.0, nan, 0.0, 440.0])
    assert _eq(O.select(f, O.align_end([], 5)), f)
    assert _eq(O.select(f, O.align_end([1, 2, 3, 4, 5], 5)), [1, 2, 3, 4, 5])
    assert O.select(f, ov).dtype == np.float32


def test_curve_of_one_point():
    g = O.curve_grid([0.5], [220.0], 100)
    want = np.full(100, nan); want[50] = 220.0
    assert _eq(g, want)
    assert _eq(O.curve_grid([0.505], [220.0], 100), np.full(100, nan))          # a single point off the grid covers no row


def test_two_voiced_points_and_the_rows_outside():
    g = O.curve_grid([0.25, 0.75], [100.0, 300.0], 100)
    assert np.all(np.isnan(g[:25])) and np.all(np.isnan(g[76:]))          # in front of t_0 and behind t_{n-1}
    assert g[25] == 100.0 and g[75] == 300.0 and g[50] == 200.0           # the ends are copied, the midpoint is the mean
    assert np.allclose(g[25:76], 100.0 + 4.0 * np.arange(51), rtol=0, atol=1e-12)
    g = O.curve_grid([0.013, 0.047], [100.0, 300.0], 10)                  # breakpoints between grid times
    assert np.all(np.isnan(g[:2])) and np.all(np.isnan(g[5:]))
    assert g[2] == pytest.approx(100.0 + 200.0 * (2 - 1.3) / 3.4, rel=1e-12)


def test_no_glide_into_zero():
    # voiced -> 0 -> voiced: every row takes the nearer breakpoint, the tie goes to the earlier one
    g = O.curve_grid([0.0, 0.04, 0.08], [200.0, 0.0, 400.0], 10)
    assert _eq(g, [200, 200, 200, 0, 0, 0, 0, 400, 400, nan])          # row 2: |2 - 0| == |4 - 2| -> 200; row 6: tie -> 0
    assert set(np.unique(g[:9])) == {0.0, 200.0, 400.0}


def test_breakpoints_on_grid_times():
    t = np.array([0.0, 0.25, 0.5, 1.0])          # exact in binary: 100 t is the integer
    hz = np.array([100.0, 0.0, 300.0, 500.0], np.float32)
    g = O.curve_grid(t, hz, 101)
    assert g[0] == 100.0 and g[25] == 0.0 and g[50] == 300.0 and g[100] == 500.0 and g[75] == 400.0
    assert not np.any(np.isnan(g))
    assert O.grid_margin(t, 101) >= 1e-2


def test_refusals():
    assert O.check_curve([0.0, 0.0], [1.0, 1.0]) and O.check_curve([0.1, 0.0], [1.0, 1.0]) and O.check_curve([], [])
    assert O.check_curve([0.0, np.inf], [1.0, 1.0]) and O.check_curve([0.0], [nan]) and O.check_curve([0.0], [-1.0]) and O.check_curve([0.0], [20001.0])
    assert O.check_curve([0.0, 1.0], [0.0, 20000.0]) is None
    assert O.check_values([nan, 0.0, 20000.0], True) is None and O.check_values([np.inf], True) and O.check_values([-0.5], True)


def test_window_rows_and_grid_frames():
    """k = 2, C = 3, X = 1: F = 63, H = 63 - 6 - 1 - 1 = 55, Tm = 64; 1.3 s = 130 frames = 3 windows"""
    g = O.geometry(2, 3, 1, 130)
    assert (g["F"], g["H"], g["Tm"], g["W"]) == (63, 55, 64, 3)
    # first window: it starts 3 frames in front of the recording, row t is frame t - 3
    assert [O.row_frame(g, 0, t) for t in (0, 3, 57, 63)] == [-3, 0, 54, 60]
    # last window: frames 107 .. 170, of which the recording has 107 .. 129
    assert [O.row_frame(g, 2, t) for t in (0, 3, 22, 23, 63)] == [107, 110, 129, 130, 170]
    grid = np.arange(130, dtype=np.float32) + 1000
    ov0, ov2 = O.window_override(grid, g, 0), O.window_override(grid, g, 2)
    assert np.all(np.isnan(ov0[:3])) and ov0[3] == 1000 and ov0[63] == 1060
    assert ov2[0] == 1107 and ov2[22] == 1129 and np.all(np.isnan(ov2[23:]))
    assert np.all(np.isnan(O.window_override(grid, g, 3)))          # a padding window


@pytest.mark.parametrize("W", [1, 2, 5])
def test_export_covers_every_frame_once(W):
    g0 = O.geometry(2, 3, 1, 1)
    for Nf in ((W - 1) * g0["H"] + 1, W * g0["H"] - 7 if W * g0["H"] - 7 > (W - 1) * g0["H"] else W * g0["H"], W * g0["H"]):
        g = O.geometry(2, 3, 1, Nf)
        assert g["W"] == W
        rows = (np.arange(W)[:, None] * 1000 + np.arange(g["Tm"])[None, :]).astype(np.float32)
        out, hits = O.export(rows, g)
        assert np.all(hits == 1)
        fr = np.arange(Nf)
        assert np.array_equal(out, (fr // g["H"]) * 1000 + g["C"] + fr % g["H"])
        # the export is the inverse of the window map on the hop
        assert np.array_equal(O.row_frame(g, fr // g["H"], g["C"] + fr % g["H"]), fr)


def test_margins_of_the_gpu_curves():
    """no grid time of the GPU test's curves lies within 1e-6 (relative) of a breakpoint time other than exactly on it; the curves reach every branch"""
    curves = O.gpu_curves()
    assert [len(t) for t, _ in curves] == [1, 2, 40]
    for t, hz in curves:
        assert O.check_curve(t, hz) is None
        for Nf in (1, 2, 333):
            assert O.grid_margin(t, Nf) >= 1e-6
    t, hz = curves[2]
    g = O.curve_grid(t, hz, 333)
    T = 100.0 * t
    assert np.isnan(g[0]) and np.isnan(g[332]) and np.sum(g == 0) >= 5 and np.sum(g > 0) > 200
    assert T[7] == 50.0 or 50.0 in T          # breakpoints exactly on grid times are among them
    assert 175.0 in T
    g32 = O.curve_grid(t, hz, 333, np.float32)
    ok = ~np.isnan(g)
    assert np.array_equal(np.isnan(g32), ~ok) and np.array_equal(g32[ok] == 0, g[ok] == 0)
