"""tests/f0_stats_ref.py against first principles, and the front ends' argument checks for auto-transpose.  No GPU."""
from __future__ import annotations

import math
import os
import re

import numpy as np
import pytest

import f0_stats_ref as S
from common import ROOT


def test_select_is_the_sorted_element():
    x = np.float32([0.0, 300.0, np.nan, 100.0, -5.0, np.inf, 200.0, 400.0, 0.0])
    got, v = S.select(x, S.QUANTILES)
    assert v == 4
    # sorted voiced rows 100 200 300 400: floor(p * 3) = 0 0 1 2 3
    assert got.tolist() == [100.0, 100.0, 200.0, 300.0, 400.0] and got.dtype == np.float32
    assert S.select(x)[0].tolist() == [200.0]                       # the lower median of an even count
    assert S.select(np.float32([3.0, 1.0, 2.0]))[0].tolist() == [2.0]
    z, v0 = S.select(np.float32([0.0, -1.0, np.nan, np.inf, -np.inf]), S.QUANTILES)
    assert v0 == 0 and not np.any(z) and z.shape == (5,)
    den = np.float32(1e-41)
    assert S.select(np.float32([den, 5.0]), (0.0,))[0][0] == den and den > 0          # a denormal is voiced
    # the result is an element of the input, bit for bit
    r = np.random.default_rng(1)
    x = np.exp(r.uniform(np.log(50.0), np.log(1100.0), 999)).astype(np.float32)
    got, v = S.select(x, S.QUANTILES)
    assert v == 999 and all(np.any(x.view(np.uint32) == g.view(np.uint32)) for g in got)
    assert got[0] == x.min() and got[-1] == x.max() and got[2] == np.sort(x)[499]


def test_select_inputs_cover_the_cases():
    for n in (1, 2, 63, 1025):
        ins = S.select_inputs(n)
        assert len(ins) == 7 and all(a.shape == (n,) and a.dtype == np.float32 for a in ins.values())
        assert S.select(ins["all unvoiced"])[1] == 0
        assert S.select(ins["one voiced row"])[1] == 1
        assert S.select(ins["all rows equal"], (0.0, 1.0))[0].tolist() == [np.float32(311.127)] * 2
        two = ins["two values one ulp apart"]
        vals = np.unique(two[two > 0])
        if n >= 2:
            assert len(vals) == 2 and vals[1] == np.nextafter(vals[0], np.float32(np.inf)) and (two == vals[0]).sum() == (two == vals[1]).sum()
        bad = ins["NaN, +inf and negative rows"]
        if n >= 63:
            assert np.isnan(bad).any() and np.isposinf(bad).any() and (bad < 0).any()
    assert S.select(S.select_inputs(1025)["a positive denormal among normal values"], (0.0,))[0][0] == np.float32(1e-41)


def test_transpose_rule():
    assert S.transpose(220.0, 110.0, 10, step=1) == 12.0
    assert S.transpose(110.0, 220.0, 10, step=1) == -12.0
    exact = S.transpose(233.0, 110.0, 10, step=0, limit=24.0)
    assert exact == 12.0 * math.log2(233.0 / 110.0) and 12.9 < exact < 13.1
    # ties go to even, on the semitone value itself (a tie rarely survives the logarithm: the rule is rint's)
    for a, want in ((0.5, 0.0), (1.5, 2.0), (2.5, 2.0), (-0.5, 0.0), (-1.5, -2.0), (0.4999, 0.0), (0.5001, 1.0)):
        assert S.round_clamp(a, 1, 24.0) == want, a
    for a, want in ((6.0, 0.0), (18.0, 24.0), (-6.0, 0.0), (-18.0, -24.0), (6.01, 12.0), (5.99, 0.0)):
        assert S.round_clamp(a, 12, 24.0) == want, a
    assert S.round_clamp(7.3, 0, 24.0) == 7.3 and S.round_clamp(18.0, 12, 12.0) == 12.0
    assert S.transpose(440.0, 110.0, 5, step=12, limit=24.0) == 24.0
    # the clamp, both ways, behind the rounding
    assert S.transpose(220.0, 110.0, 5, step=1, limit=5.0) == 5.0
    assert S.transpose(110.0, 220.0, 5, step=12, limit=5.0) == -5.0
    assert S.transpose(220.0, 110.0, 5, step=0, limit=0.0) == 0.0
    # nothing voiced
    assert S.transpose(220.0, 0.0, 0) == 0.0 and S.transpose(220.0, 110.0, 0) == 0.0
    assert S.factor(0.0) is None and S.factor(12.0) == np.float32(2.0) and S.factor(-12.0) == np.float32(0.5)
    assert S.factor(3.0) == np.float32(2.0 ** 0.25)


def test_merge():
    nan = np.float32(np.nan)
    curve = np.float32([nan, 440.0, 0.0, nan])
    tracked = np.float32([100.0, 110.0, 120.0, 0.0])
    assert S.merge(curve, tracked).tolist() == [100.0, 440.0, 0.0, 0.0]
    assert S.select(S.merge(np.full(5, 440.0, np.float32), np.float32([1, 2, 3, 4, 5])))[0][0] == np.float32(440.0)


def test_argument_checks():
    assert S.check_auto_transpose_args(0.0, 1, 12.0) and S.check_auto_transpose_args(20000.0, 12, 24.0) and S.check_auto_transpose_args(155.0, 0, 0.0)
    for bad in ((-1.0, 1, 12.0), (20000.5, 1, 12.0), (float("nan"), 1, 12.0), (155.0, 2, 12.0), (155.0, -1, 12.0), (155.0, 1, 24.5), (155.0, 1, -0.1), (155.0, 1, float("nan"))):
        assert not S.check_auto_transpose_args(*bad), bad
    from obs_rvc_amd.convert import AUTO_PITCH_STEPS, parse_args
    base = ["in.wav", "-o", "out.wav", "--model", "m.rvcw"]
    a = parse_args(base)
    assert a.auto_pitch == 0.0 and a.auto_pitch_from is None and a.auto_pitch_step == 1 and a.auto_pitch_limit == 12.0 and not a.analyze_only
    a = parse_args(base + ["--auto-pitch", "255", "--auto-pitch-step", "12", "--auto-pitch-limit", "24"])
    assert (a.auto_pitch, a.auto_pitch_step, a.auto_pitch_limit) == (255.0, 12, 24.0) and AUTO_PITCH_STEPS == (0, 1, 12)
    assert parse_args(base + ["--auto-pitch-from", "ref.wav", "--auto-pitch-step", "0"]).auto_pitch_from == "ref.wav"
    for bad in (["--auto-pitch-step", "2"], ["--auto-pitch", "-155"], ["--auto-pitch", "20001"], ["--auto-pitch-limit", "24.5"], ["--auto-pitch-limit", "-1"],
                ["--auto-pitch", "155", "--auto-pitch-from", "ref.wav"], ["--analyze-only"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    with pytest.raises(SystemExit):
        parse_args(["in.wav", "--analyze-only"])                     # ... without --f0-out
    a = parse_args(["in.wav", "--analyze-only", "--f0-out", "f0.csv", "--f0", "yin"])
    assert a.analyze_only and a.model is None and a.output is None and a.f0_out == "f0.csv"
    for missing in (["in.wav", "-o", "out.wav"], ["in.wav", "--model", "m.rvcw"]):          # a conversion still needs both
        with pytest.raises(SystemExit):
            parse_args(missing)


def test_every_front_end_declares_the_entry_points():
    from obs_rvc_amd import _native
    from obs_rvc_amd.rvc import RvcInfer
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    hdr = re.sub(r"/\*.*?\*/", "", read("include", "rvc_mi355x.h"), flags=re.S)
    ffi = read("bindings", "rust", "rvc", "src", "ffi.rs")
    for name in ("rvc_analyze_f0", "rvc_analyze_f0_device", "rvc_f0_stats", "rvc_f0_stats_stream", "rvc_set_auto_transpose", "rvc_auto_transpose", "rvc_auto_transpose_info"):
        assert name in _native.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr) and re.search(r"pub fn %s\s*\(" % name, ffi), name
    for method in ("analyze_f0", "f0_stats", "f0_stats_stream", "set_auto_transpose", "auto_transpose", "auto_transpose_info"):
        assert callable(getattr(RvcInfer, method)), method
    # the select kernel is integer arithmetic on the bit patterns: no float type in its body but the quantile itself
    src = read("obs_rvc_amd", "csrc", "f0_select.hip.h")
    body = src[src.index("void f0_select_kernel"):src.index("// tracked[j]")]
    assert "float" not in body and body.count("double") == 1 and "atomicAdd" in body
