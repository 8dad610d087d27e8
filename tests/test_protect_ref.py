"""tests/protect_ref.py (the float64 restatement of consonant protection) on rows whose answer is known, and the mirrors of the
new entry points (header, Python, Rust, the library's source list)."""
from __future__ import annotations

import os
import re

import numpy as np

import protect_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case():
    # C = 2, T = 3 -> 7 feature rows (columns 0 0 1 1 2 2 2); the call takes rows 2 .. 6
    cv = np.array([[1.0, 2.0, 3.0], [10.0, 20.0, 30.0]], np.float32)
    phone = np.array([[5.0, 6.0, 7.0, 8.0, 9.0], [50.0, 60.0, 70.0, 80.0, 90.0]], np.float32)
    pitchf = np.array([0.0, 220.0, 0.5, 1.0, 0.0], np.float32)
    return phone, cv, pitchf


def test_hand_made_rows():
    phone, cv, pitchf = _case()
    assert np.array_equal(P.raw_rows(cv, 2, 5), [[2, 2, 3, 3, 3], [20, 20, 30, 30, 30]])
    out, bound, uv = P.protect_mix(phone, cv, pitchf, 0.25, 2)
    # 0.5 counts as unvoiced, exactly 1.0 as voiced
    assert np.array_equal(uv, [True, False, True, False, True])
    want = phone.astype(np.float64)
    want[:, 0] = 0.25 * phone[:, 0] + 0.75 * np.array([2.0, 20.0])
    want[:, 2] = 0.25 * phone[:, 2] + 0.75 * np.array([3.0, 30.0])
    want[:, 4] = 0.25 * phone[:, 4] + 0.75 * np.array([3.0, 30.0])
    assert np.array_equal(out, want)
    assert np.array_equal(out[:, ~uv], phone[:, ~uv]) and np.all(bound[:, ~uv] == 0) and np.all(bound[:, uv] > 0)
    assert np.allclose(bound[:, 0], 2.0 ** -21 * (0.25 * phone[:, 0] + 0.75 * np.array([2.0, 20.0])), rtol=1e-15)


def test_p_zero_gives_raw_and_off_gives_the_input():
    phone, cv, pitchf = _case()
    out, _, uv = P.protect_mix(phone, cv, pitchf, 0.0, 2)
    assert np.array_equal(out[:, uv], P.raw_rows(cv, 2, 5)[:, uv]) and np.array_equal(out[:, ~uv], phone[:, ~uv])
    for off in (0.5, 0.75):
        out, bound, uv = P.protect_mix(phone, cv, pitchf, off, 2)
        assert np.array_equal(out, phone) and not uv.any() and not bound.any()
    # p is the float the engine stores: 0.33 is (float)0.33, and 1 - p is exact in float64
    out, _, _ = P.protect_mix(phone, cv, pitchf, 0.33, 2)
    p = float(np.float32(0.33))
    assert p != 0.33 and out[0, 0] == p * 5.0 + (1.0 - p) * 2.0


def test_column_rule_at_the_last_row():
    # the feature sequence has 2 T + 1 rows: every column twice, the last one three times
    for T in (1, 2, 7):
        cols = [P.src_col(0, r, T) for r in range(2 * T + 1)]
        assert cols == sorted(cols) and cols[-1] == cols[-2] == cols[-3] == T - 1 and cols[0] == 0
        assert all(cols.count(c) == 2 for c in range(T - 1))
    assert P.src_col(3, 4, 7) == 3 and P.src_col(4, 4, 7) == 4 and P.src_col(13, 1, 7) == 6
    cv = np.arange(14, dtype=np.float32).reshape(2, 7)
    assert np.array_equal(P.raw_rows(cv, 12, 3), [[6, 6, 6], [13, 13, 13]])          # rows 12, 13, 14 = 2 T: the repeated last column
    assert np.array_equal(P.raw_rows(cv, 11, 3), [[5, 6, 6], [12, 13, 13]])


def test_entry_points_are_mirrored():
    from obs_rvc_amd import _native
    from obs_rvc_amd.rvc import RvcInfer
    hdr = open(os.path.join(ROOT, "include", "rvc_mi355x.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "rvc", "src", "ffi.rs")).read()
    shim = open(os.path.join(ROOT, "bindings", "rust", "rvc", "src", "rvc.rs")).read()
    for name in ("rvc_set_protect", "rvc_set_protect_stream"):
        assert name in _native.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr) and re.search(r"pub fn %s\s*\(" % name, ffi), name
    assert re.search(r"pub fn set_protect\s*\(", shim) and hasattr(RvcInfer, "set_protect")
    # the header is hashed into the library, and into the object of every unit that reaches it through its #include lines: the unit that builds the plan op for one
    assert "protect.hip.h" in _native.SOURCES
    reach = [src for src, _, _ in _native.UNITS if "protect.hip.h" in _native._include_closure(src)]
    assert reach and "engine.hip" in reach
    assert all("protect.hip.h" in deps for src, _, deps in _native.UNITS if src in reach)
    dbg = open(os.path.join(ROOT, "include", "rvc_mi355x_debug.h")).read()
    assert re.search(r"\brvc_debug_protect\s*\(", dbg)
