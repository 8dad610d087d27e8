"""Hybrid f0 without a device: the float32 definition of tests/f0_hybrid_ref.py against brute-force enumeration and np.median, the --f0 "hybrid[...]" parser
of obs_rvc_amd.convert, and the argument checks RvcInfer.load_f0_hybrid makes before it calls the library."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import f0_hybrid_ref as H
from obs_rvc_amd import rvc_common as RC
from obs_rvc_amd.convert import f0_arg, parse_args
from obs_rvc_amd.rvc import RvcInfer

VOICED = [np.float32(v) for v in (100.0, 220.0, 220.0, 441.5, 1.0e-3)]          # (220 twice: equal values among members)
UNVOICED = [np.float32(v) for v in (0.0, -0.0, -50.0, float("nan"))]


def _brute(vals, mode):
    """the definition once more, by numpy sorting on arrays instead of Python lists: counts and order statistics spelled out"""
    a = np.asarray(vals, np.float32)
    n = len(a)
    with np.errstate(invalid="ignore"):
        on = a > 0
    v = int(on.sum())
    if mode == H.MEDIAN:
        s = np.sort(np.where(on, a, np.float32(0)))
        c = n
    else:
        if not (2 * v > n or (2 * v == n and bool(on[0]))):
            return np.float32(0)
        s = np.sort(a[on])
        c = v
    return s[c // 2] if c % 2 else np.float32(0.5) * (s[c // 2 - 1] + s[c // 2])


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", [H.VOTE, H.MEDIAN])
def test_reference_against_enumeration(n, mode):
    """every voicing pattern of n members, the voiced and the unvoiced places each running over their value sets"""
    seen = set()
    count = 0
    for mask in range(1 << n):
        pools = [VOICED if (mask >> i) & 1 else UNVOICED for i in range(n)]
        for vals in itertools.product(*pools):
            got, want = H.combine_frame(vals, mode), _brute(vals, mode)
            assert got.dtype == np.float32 and _bits(got) == _bits(want), (vals, mode, got, want)
            assert not np.isnan(got) and got >= 0
            seen.add(H.frame_class(vals))
            count += 1
    assert count == sum(len(VOICED) ** bin(m).count("1") * len(UNVOICED) ** (n - bin(m).count("1")) for m in range(1 << n))
    want_classes = {1: {"all_voiced_odd", "all_unvoiced"}, 2: {"all_voiced_even", "all_unvoiced", "tie_lead_voiced", "tie_lead_unvoiced"},
                    3: {"all_voiced_odd", "all_unvoiced", "majority_voiced", "majority_unvoiced"},
                    4: {"all_voiced_even", "all_unvoiced", "majority_voiced", "majority_unvoiced", "tie_lead_voiced", "tie_lead_unvoiced"}}[n]
    assert seen == want_classes


def test_stated_cases():
    c = lambda vals, mode=H.VOTE: float(H.combine_frame(vals, mode))
    # the lead breaks an exact tie, and only an exact tie
    assert c([100, 0]) == 100 and c([0, 100]) == 0
    assert c([100, 200, 0, 0]) == 150 and c([0, 0, 100, 200]) == 0 and c([0, 100, 200, 0]) == 0 and c([100, 0, 0, 200]) == 150
    assert c([0, 100, 200]) == 150 and c([100, 0, 0]) == 0
    # > 0 is the voicing test: NaN, negative values and both zeros are unvoiced
    assert c([float("nan"), 100, 200]) == 150 and c([-5, 100, 200]) == 150 and c([-0.0, 7]) == 0 and c([float("nan")]) == 0 and c([-3.0], H.MEDIAN) == 0
    # the median: the middle value, or half the sum of the two middle ones
    assert c([300, 100, 200]) == 200 and c([400, 100, 300, 200]) == 250 and c([100, 100, 300]) == 100
    # MEDIAN is the plain median with unvoiced members as 0: it halves f0 where two members disagree on voicing, VOTE does not
    assert c([200, 0], H.MEDIAN) == 100 and c([0, 200], H.MEDIAN) == 100 and c([200, 0]) == 200
    assert c([200, 0, 0], H.MEDIAN) == 0 and c([200, 210, 0], H.MEDIAN) == 200 and c([200, 210, 0, 0], H.MEDIAN) == 100
    # a hybrid of one member is that member (negative values and NaN become 0: no tracker of the engine produces them)
    x = np.array([0.0, 55.5, 440.0, 1e-30], np.float32)
    for mode in (H.VOTE, H.MEDIAN):
        assert np.array_equal(_bits(H.combine(x[None], mode)), _bits(x))
    # the even rule is computed in float32: the sum is rounded before the halving
    a, b = np.float32(16777216.0), np.float32(16777218.0)
    assert H.combine_frame([a, np.float32(1.0), b, np.float32(3e7)], H.VOTE) == np.float32(0.5) * np.float32(a + b)
    big = np.float32(3e38)
    with np.errstate(over="ignore"):
        assert np.isinf(H.combine_frame([big, big], H.VOTE))          # (the sum overflows first, as 0.5f * (a + b) does on the device)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_median_mode_is_np_median(n):
    """MEDIAN on finite non-negative rows is np.median over the members in float32, bit for bit (np.median halves the float32 sum of the two middle values;
    dividing by 2 and multiplying by 0.5 round alike).  Shapes (n, B, Tm) as the kernel sees them"""
    rng = np.random.default_rng(40 + n)
    rows = rng.uniform(50.0, 1100.0, size=(n, 3, 33)).astype(np.float32)
    rows[rng.random(rows.shape) < 0.3] = 0.0
    rows[0, 0, :5] = rows[n - 1, 0, :5]                     # equal values
    got = H.combine(rows, H.MEDIAN)
    want = np.median(rows, axis=0)
    assert got.shape == (3, 33) and want.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
    # ... and VOTE where every member is voiced
    rows = np.maximum(rows, np.float32(50.0))
    assert np.array_equal(_bits(H.combine(rows, H.VOTE)), _bits(np.median(rows, axis=0)))


def test_f0_argument_parser():
    base = ["in.wav", "-o", "o.wav", "--model", "m"]
    a = parse_args(base + ["--f0", "hybrid[rmvpe+fcpe+crepe-tiny]"])
    assert a.f0 == "hybrid[rmvpe+fcpe+crepe-tiny]" and a.f0_hybrid_mode == "vote"
    a = parse_args(base + ["--f0", "Hybrid[ YIN + fcpe ]", "--f0-hybrid-mode", "median"])
    assert a.f0 == "hybrid[yin+fcpe]" and a.f0_hybrid_mode == "median"
    assert parse_args(base + ["--f0", "hybrid[yin]"]).f0 == "hybrid[yin]"
    assert parse_args(base + ["--f0", "hybrid[fcpe+crepe-full+yin+rmvpe]"]).f0 == "hybrid[fcpe+crepe-full+yin+rmvpe]"          # the order is the caller's
    assert parse_args(base).f0 == "rmvpe" and parse_args(base + ["--f0", "fcpe"]).f0 == "fcpe"
    for bad in ("hybrid", "hybrid[]", "hybrid[rmvpe", "hybrid rmvpe+fcpe", "hybrid[rmvpe+rmvpe]", "hybrid[rmvpe+harvest]", "hybrid[rmvpe+]",
                "hybrid[crepe+yin]", "hybrid[rmvpe+yin+fcpe+crepe-tiny+crepe-full]", "hybrid[hybrid[yin]]", "crepe", "harvest", "rmvpe+fcpe"):
        with pytest.raises(SystemExit):
            parse_args(base + ["--f0", bad])
    with pytest.raises(SystemExit):
        parse_args(base + ["--f0", "hybrid[yin+fcpe]", "--f0-hybrid-mode", "mean"])
    assert f0_arg("hybrid[rmvpe+fcpe]") == "hybrid[rmvpe+fcpe]" and f0_arg("yin") == "yin"
    # the shared parser: None for what is no hybrid form at all, the members in order otherwise
    names = RvcInfer._F0_NAMES
    assert RC.parse_f0_hybrid("rmvpe", names) is None and RC.parse_f0_hybrid("harvest", names) is None
    assert RC.parse_f0_hybrid("hybrid[crepe+yin]", names) == ["crepe", "yin"]
    with pytest.raises(ValueError):
        RC.parse_f0_hybrid("hybrid[harvest]", names)


def test_wrapper_validates_before_the_call():
    """RvcInfer.load_f0_hybrid checks its arguments through _hybrid_args first (a classmethod: no engine, no device)"""
    assert (RC.F0_HYBRID, RC.HYBRID_VOTE, RC.HYBRID_MEDIAN, RC.HYBRID_MAX_MEMBERS) == (8, 0, 1, 4) and (H.VOTE, H.MEDIAN, H.MAX_MEMBERS) == (0, 1, 4)
    ok = RvcInfer._hybrid_args
    assert ok(["rmvpe", "fcpe"], "vote") == ([RC.F0_RMVPE, RC.F0_FCPE], 0)
    assert ok(("FCPE", RC.F0_YIN, "crepe-tiny", "crepe"), "Median") == ([RC.F0_FCPE, RC.F0_YIN, RC.F0_CREPE_TINY, RC.F0_CREPE], 1)
    assert ok([RC.F0_YIN], RC.HYBRID_MEDIAN) == ([2], 1)
    for methods, mode in (([], "vote"), (["rmvpe"] * 2, "vote"), (["rmvpe", RC.F0_RMVPE], "vote"), (["yin", "fcpe", "rmvpe", "crepe", "crepe-tiny"], "vote"),
                          (["harvest"], "vote"), ([0], "vote"), ([3], "vote"), ([6], "vote"), ([8], "vote"), ([-1], "vote"), ("rmvpe", "vote"),
                          (["crepe", "crepe-full"], "vote"), (["yin"], "mean"), (["yin"], 2), (["yin"], -1)):
        with pytest.raises(ValueError):
            ok(methods, mode)
