"""tests/f0cond_ref.py, the float64 restatement of the pitch controls (DESIGN.md "Pitch controls") that tests/test_gpu_f0cond.py holds the kernel
against: its parts on rows whose answer is known, and the quality of the inputs the GPU tests use.  No GPU."""
import numpy as np
import pytest

import f0cond_ref as F
import yin_ref as Y


def _hz(n):
    return 440.0 * 2.0 ** ((np.asarray(n, np.float64) - 69.0) / 12.0)


def _note(f):
    return 69.0 + 12.0 * np.log2(np.asarray(f, np.float64) / 440.0)


def _brute_median(f, r):
    out = np.empty(len(f))
    for i in range(len(f)):
        w = sorted(float(f[j]) if 0 <= j < len(f) else 0.0 for j in range(i - r, i + r + 1))
        out[i] = w[r]
    return out


def test_median_against_brute_force():
    rng = np.random.default_rng(0)
    for n in (15, 32, 101):
        f = np.where(rng.random(n) < 0.3, 0.0, 100.0 + 300.0 * rng.random(n))
        for r in range(8):
            got, margin = F.condition(f, r=r)
            assert np.array_equal(got, _brute_median(f, r)), (n, r)
            assert np.all(margin == 1.0)
    assert np.array_equal(F.condition([0.0, 200.0, 0.0, 210.0, 220.0, 230.0, 0.0], r=1)[0], [0.0, 0.0, 200.0, 210.0, 220.0, 220.0, 0.0])


def test_multiplier_is_a_float_product():
    assert F.multiplier(12) == 2.0 and F.multiplier(7) == 1.0 and F.multiplier(-13) == 0.5
    assert F.multiplier(0, 7.0) == np.float32(2.0 ** (7.0 / 12.0)) and F.multiplier(12, 7.0) == np.float32(2.0) * np.float32(2.0 ** (7.0 / 12.0))
    assert F.multiplier(0, 0.0, 3.0) == np.float32(2.0 ** (-0.25))
    assert F.multiplier(0, 2.0, 3.0) == np.float32(np.float32(2.0 ** (-0.25)) * np.float32(2.0 ** (2.0 / 12.0)))
    assert F.multiplier(0, 7.0).dtype == np.float32


def test_gate():
    f = np.array([0.0, 99.0, 100.0, 150.0, 200.0, 201.0])
    got, margin = F.condition(f, lo=100.0, hi=200.0)
    assert np.array_equal(got, [0.0, 0.0, 100.0, 150.0, 200.0, 0.0])
    assert margin[0] == 1.0 and margin[2] == 0.0 and margin[4] == 0.0 and abs(margin[1] - 0.01) < 1e-15 and abs(margin[3] - 0.25) < 1e-15
    assert np.array_equal(F.condition(f, lo=0.0, hi=np.inf)[0], f)
    # the gate refers to the multiplied value, and comes in front of the median
    assert np.array_equal(F.condition(f, up=2.0, lo=100.0, hi=250.0)[0], [0.0, 198.0, 200.0, 0.0, 0.0, 0.0])
    assert np.array_equal(F.condition([150.0, 99.0, 150.0], lo=100.0, hi=200.0, r=1)[0], [0.0, 150.0, 0.0])


def test_snap_lands_on_allowed_notes_and_is_idempotent():
    rng = np.random.default_rng(1)
    f = np.concatenate([[0.0], _hz(36.0 + 48.0 * rng.random(200))])
    for mask in (F.SCALE_CHROMATIC, F.SCALE_C_MAJOR, 1 << 9, 0b100000000001):
        got, margin = F.condition(f, mask=mask, s=1.0)
        assert got[0] == 0.0 and margin[0] == 1.0
        n = _note(got[1:])
        assert np.max(np.abs(n - np.round(n))) < 1e-12
        assert all((mask >> (int(k) % 12)) & 1 for k in np.round(n))
        assert np.all(np.abs(_note(f[1:]) - n) <= 6.0 + 1e-9)
        again, _ = F.condition(got, mask=mask, s=1.0)
        assert np.max(np.abs(again[1:] - got[1:]) / got[1:]) < 1e-12
        # the nearest allowed note, by exhaustion
        for v, k in zip(f[1:], np.round(n)):
            notes = F.allowed_notes(mask, 0, 127)
            assert abs(_note(v) - k) == np.min(np.abs(notes - _note(v)))


def test_snap_ties_go_to_the_lower_note():
    # n = 60.5 exactly: 440 * 2^(-8.5 / 12) is not exact in binary, so the tie is made in note space through a float64 whose note IS x.5
    for k in (48, 59, 60, 71):
        f = _hz(k + 0.5)
        n = float(_note(f))
        if n != k + 0.5:
            continue
        assert abs(_note(F.condition([f], mask=F.SCALE_CHROMATIC, s=1.0)[0][0]) - k) < 1e-12
    tied = [k for k in range(36, 84) if float(_note(_hz(k + 0.5))) == k + 0.5]
    assert len(tied) >= 4, tied
    # C major: between E (64) and F (65) a semitone, between C (60) and D (62) the midpoint is 61
    f = _hz(61.0)
    assert float(_note(f)) == 61.0
    got, margin = F.condition([f], mask=F.SCALE_C_MAJOR, s=1.0)
    assert abs(_note(got[0]) - 60.0) < 1e-12 and margin[0] == 0.0
    assert abs(_note(F.condition([_hz(61.01)], mask=F.SCALE_C_MAJOR, s=1.0)[0][0]) - 62.0) < 1e-12


def test_single_class_mask_jumps_octaves():
    only_a = 1 << 9
    for n, want in ((45.0, 45), (50.9, 45), (51.1, 57), (57.0, 57), (62.99, 57), (63.01, 69), (80.0, 81), (20.0, 21)):
        got, _ = F.condition([_hz(n)], mask=only_a, s=1.0)
        assert abs(_note(got[0]) - want) < 1e-12, (n, want)
    got, margin = F.condition([_hz(50.9)], mask=only_a, s=1.0)
    assert abs(margin[0] - 0.1) < 1e-9


def test_strength_scales_the_step_and_neutral_is_the_identity():
    f = np.array([0.0, 131.0, 207.3, 440.0, 987.0])
    full, _ = F.condition(f, mask=F.SCALE_C_MAJOR, s=1.0)
    half, _ = F.condition(f, mask=F.SCALE_C_MAJOR, s=0.5)
    v = f > 0
    assert np.max(np.abs((_note(half[v]) - _note(f[v])) - 0.5 * (_note(full[v]) - _note(f[v])))) < 1e-12
    for kw in (dict(mask=0, s=1.0), dict(mask=F.SCALE_C_MAJOR, s=0.0), dict(F.settings("median1"), r=0), {}):
        got, margin = F.condition(f, **kw)
        assert np.array_equal(got, f) and np.all(margin == 1.0)


def test_float32_recipe_stays_close():
    f0, _ = Y.yin(F.inputs()["glide"], 2560)
    for case in ("chromatic", "cmajor_half", "only_a", "stream1"):
        ref, margin = F.condition(f0, **F.settings(case))
        f32, _ = F.condition(f0.astype(np.float32), dtype=np.float32, **F.settings(case))
        assert f32.dtype == np.float32
        v = (ref > 0) & (margin >= F.SNAP_MARGIN)
        assert np.array_equal(f32[margin >= F.SNAP_MARGIN] > 0, ref[margin >= F.SNAP_MARGIN] > 0)
        assert np.max(np.abs(f32[v] - ref[v]) / ref[v]) < 2e-6


def _quality(f0, yin_margin, case, pitch_shift, formant=None):
    c = F.CASES[case]
    rows, margin, gm, sm = F.condition(f0, F.multiplier(pitch_shift, c["st"], formant), parts=True, **F.settings(case))
    assert np.sum(gm < F.GATE_MARGIN) == 0, (case, gm.min())
    assert np.sum(sm < F.SNAP_MARGIN) == 0, (case, sm.min())
    assert np.array_equal(margin, np.minimum(gm, sm))
    assert np.sum(F.window_min(yin_margin, c["r"]) < 1e-4) == 0, case          # the source's own voicing decisions (tests/yin_ref.py)
    return rows


def test_inputs_of_the_gpu_tests_sit_on_no_decision_boundary():
    # the GPU tests may leave up to 10 % of the rows out of a decision check; with these inputs and settings they need to leave out none
    yin = {name: Y.yin(x, 2560) for name, x in F.inputs().items()}
    assert np.sum(yin["composite"][0] > 0) >= 12 and np.sum(yin["composite"][0] == 0) >= 12          # voiced / unvoiced edges
    assert np.sum(yin["glide"][0] > 0) >= 24
    for name, case in F.PITCH_CASES:
        rows = _quality(*yin[name], case, 0)
        if case == "gate":
            cut = (yin[name][0] > 0) & (rows == 0)
            assert cut.any() and (rows > 0).any(), (name, "the gate must cut part of the voiced rows")
    lo, hi = F.CASES["gate"]["lo"], F.CASES["gate"]["hi"]
    g = yin["glide"][0]
    assert np.any((g > 0) & (g < lo)) and np.any(g > hi) and np.any((g > lo) & (g < hi))
    # the per-stream test: every chunk of every stream under its stream's settings (infer calls: formant factor (float)2^0 = 1)
    xs = F.stream_chunks()
    for k in range(2):
        for s, (case, shift) in enumerate(F.STREAM_CASES):
            if case != "neutral":
                f0, ym = Y.yin(xs[k][s], 2560)
                rows = _quality(f0, ym, case, shift, 0.0)
                assert np.sum(rows > 0) >= 6
                if case == "stream2":
                    assert np.any((f0 > 0) & (rows == 0)), "the gate must cut part of the voiced rows"
    # the settings changed between two chunks of one stream (stream 0's first chunk neutral, stream 1's second chunk conditioned)
    assert np.sum(_quality(*Y.yin(xs[1][1], 2560), "changed", 12, 0.0) > 0) >= 6
    assert np.sum(Y.yin(xs[0][0], 2560)[1] < 1e-4) == 0


def test_whole_window_input_of_the_gpu_test():
    # tests/test_gpu_f0cond.py test_pitch_over_the_default_converter_window: the k = 14 window (448 rows) under a width-7 median and a C major snap leaves at
    # most 10 % of its rows next to a decision boundary, keeps voiced rows at the window's end, and float32 changes no sure decision
    frame16k = 5120 * 13
    x = Y.whole_window_signal(frame16k)
    f0, ym = Y.yin(x, frame16k)
    kw = F.settings("stream1")
    assert kw["r"] == 3 and kw["mask"] == F.SCALE_C_MAJOR
    ref, margin, gm, _ = F.condition(f0, parts=True, **kw)
    sure = (F.window_min(ym, 3) >= 1e-4) & (margin >= F.SNAP_MARGIN) & (gm >= F.GATE_MARGIN)
    assert ref.shape == (448,) and np.sum(~sure) <= 0.10 * 448, np.sum(~sure)
    assert np.any((ref[-4:] > 0) & sure[-4:]) and np.sum((ref > 0) & sure) >= 224
    f32, _ = F.condition(Y.yin(x, frame16k, np.float32)[0], dtype=np.float32, **kw)
    assert np.array_equal(f32[sure] > 0, ref[sure] > 0)
    v = sure & (ref > 0)
    assert np.max(np.abs(f32[v].astype(np.float64) - ref[v]) / ref[v]) < 1e-5
