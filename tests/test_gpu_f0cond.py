"""The per-stream pitch controls (DESIGN.md "Pitch controls"; rvc_set_pitch_semitones / rvc_set_f0_range / rvc_set_f0_median / rvc_set_f0_snap, the
stage of f0cond.hip.h inside the pitch tail) against the float64 restatement of tests/f0cond_ref.py, with YIN (tests/yin_ref.py) as the f0 source
unless stated.  The smallest geometry: sample_frame_16k_size = 2560, an f0 window of 4960 samples, 32 rows, the tiny zoo.

Bounds are derived as in tests/test_gpu_yin.py: the same recipe (YIN, then the controls) in float32 numpy against float64, times 8, floor 1e-6,
measured and printed on every run.  A row takes part in a decision check (voicing, which note) when its float64 margins allow: 1e-4 at YIN's
threshold for every row of its median window, 1e-4 relative at the gate, 1e-3 semitone at a snap midpoint; at most 10 % of the rows may be left
out, and tests/test_f0cond_ref.py shows that the inputs used here leave out none.  Selection (median, gate survivors) and the power-of-two shift
are checked bit for bit; the semitone factor to one float rounding.
The kernel's own error has not been observed on a device yet; every case prints it before it asserts."""
from __future__ import annotations

import numpy as np
import pytest
from scipy.signal import medfilt

import f0cond_ref as F
import yin_ref as Y
from common import BASELINE_160MS as g, voice_signal, zoo
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc_common import SCALE_C_MAJOR, SCALE_CHROMATIC, RvcInferError, scale_mask

pytestmark = pytest.mark.gpu

FRAME16K = g.sample_frame_16k          # 2560
R = g.model_return_length
L = g.input_buffer_16k_size
SHIFT, CACHE_START = FRAME16K // 160, 1024 + 4 - 32          # rvc.rs:168,172 at 32 rows
YIN_MARGIN = 1e-4
assert FRAME16K == 2560 and Y.f0_frame(FRAME16K) == 4960 and SCALE_C_MAJOR == F.SCALE_C_MAJOR and SCALE_CHROMATIC == F.SCALE_CHROMATIC


def _engine(z, method="yin", streams=1, full=True):
    from obs_rvc_amd.rvc import RvcInfer
    e = RvcInfer(z["data"])
    if full:
        e.load_contentvec(2); e.load_model(z["model"])
    e.load_f0_method(method)
    if streams > 1:
        e.set_streams(streams)
    e.set_noise_seed(1234, 0)
    return e


def _apply(e, case, stream=None):
    c = F.CASES[case] if isinstance(case, str) else case
    e.set_pitch_semitones(c["st"], stream)
    e.set_f0_range(c["lo"], c["hi"], stream)
    e.set_f0_median(c["r"], stream)
    e.set_f0_snap(c["mask"], c["s"], stream)


def _sr(z):
    return int(W.read_blob(z["model"])[0]["sr"])


def _sure(yin_margin, cond_margin, gate_margin, r):
    """rows whose decisions the float64 reference is sure of"""
    sure = (F.window_min(yin_margin, r) >= YIN_MARGIN) & (cond_margin >= F.SNAP_MARGIN) & (gate_margin >= F.GATE_MARGIN)
    assert np.sum(~sure) <= 0.10 * len(sure), "more than 10 %% of the rows next to a decision boundary: %d" % np.sum(~sure)
    return sure


def _check(got, ref, sure, bound, what=""):
    """got (float32, device) against ref (float64): voicing on the sure rows, the relative error on the sure rows both call voiced"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(got[sure] > 0, ref[sure] > 0), np.where((got > 0) != (ref > 0))
    v = sure & (got > 0) & (ref > 0)
    err = float(np.max(np.abs(got[v] - ref[v]) / ref[v])) if v.any() else 0.0
    print("%s: voiced %d of %d, left out %d, largest relative error %.3e (bound %.3e)" % (what, v.sum(), len(ref), np.sum(~sure), err, bound))
    assert err <= bound, err
    return v


def _on_allowed_notes(rows, mask, bound, what=""):
    """every voiced row's 12 log2(f / 440) within the bound of an allowed integer: a relative error eps of f is 12 log2(1 + eps) semitones"""
    f = np.asarray(rows, np.float64)
    f = f[f > 0]
    m = 12.0 * np.log2(f / 440.0)
    k = np.round(m)
    off = float(np.max(np.abs(m - k))) if len(f) else 0.0
    print("%s: %d voiced rows, farthest from a note %.3e semitones (bound %.3e)" % (what, len(f), off, 12.0 * np.log2(1.0 + bound)))
    assert len(f) and off <= 12.0 * np.log2(1.0 + bound)
    assert all((mask >> ((int(n) + 69) % 12)) & 1 for n in k)


@pytest.fixture(scope="module")
def base():
    """per input: the float64 YIN rows and margins, the float32 run of the same recipe, and the device's neutral rvc_pitch rows; one f0-only engine"""
    e = _engine(zoo("tiny"), full=False)
    out = {"engine": e}
    for name, x in F.inputs().items():
        ref, margin = Y.yin(x, FRAME16K)
        f32, _ = Y.yin(x, FRAME16K, np.float32)
        out[name] = {"x": x, "ref": ref, "margin": margin, "f32": f32, "got0": e.pitch(x, 0, FRAME16K)}
    yield out
    e.close()


def _bound(b, case, up=1.0):
    """8 x (float32 numpy against float64 of YIN + the controls) on the sure voiced rows, floor 1e-6"""
    kw = F.settings(case)
    ref, margin, gm, _ = F.condition(b["ref"], up, parts=True, **kw)
    f32, _ = F.condition(b["f32"], up, dtype=np.float32, **kw)
    v = (ref > 0) & (f32 > 0) & (F.window_min(b["margin"], kw["r"]) >= YIN_MARGIN) & (margin >= F.SNAP_MARGIN) & (gm >= F.GATE_MARGIN)
    basev = float(np.max(np.abs(f32[v].astype(np.float64) - ref[v]) / ref[v])) if v.any() else 0.0
    bound = max(8.0 * basev, 1e-6)
    print("float32 numpy against float64 (%s): %.3e -> bound %.3e" % (case, basev, bound))
    return bound


# ---- 1. neutral = untouched ----
@pytest.mark.parametrize("method,streams", [("yin", 1), ("yin", 3), ("rmvpe", 1), ("rmvpe", 3)])
def test_neutral_settings_change_nothing(method, streams):
    z = zoo("tiny")
    xs = [np.stack([voice_signal(L, seed=10 * k + s + 1) for s in range(streams)]) for k in range(2)]
    xs[1][streams // 2, -4960:] = Y.composite_signal()[-4960:]
    res = []
    for touched in (True, False):
        e = _engine(z, method, streams)
        if touched:
            _apply(e, F.NEUTRAL)
            for s in range(streams):
                _apply(e, F.NEUTRAL, s)
        p = e.pitch(xs[1][0], 12, FRAME16K) if streams == 1 else None
        e.reset_state()
        ys = [e.infer_batch(xs[k], FRAME16K, [12, 0, -7][:streams], g.skip_head, R) for k in range(2)]
        res.append((p, ys, [e.pitch_cache(s) for s in range(streams)]))
        e.close()
    (pa, ya, ca), (pb, yb, cb) = res
    assert streams > 1 or (np.array_equal(pa, pb) and np.any(pa > 0))
    assert all(np.array_equal(a, b) and np.all(np.isfinite(a)) for a, b in zip(ya, yb))
    assert all(np.array_equal(a, b) for a, b in zip(ca, cb)) and np.any(ca[0] > 0)


# ---- 2. transpose ----
def test_transpose_in_semitones(base):
    e, b = base["engine"], base["composite"]
    x, got0 = b["x"], b["got0"]
    assert np.sum(got0 > 0) >= 12
    try:
        for st in (7.0, -5.0, 0.5):
            e.set_pitch_semitones(st)
            got = e.pitch(x, 0, FRAME16K)
            want = got0.astype(np.float64) * float(np.float32(2.0 ** (st / 12.0)))
            v = got0 > 0
            err = float(np.max(np.abs(got[v] - want[v]) / want[v]))
            print("st %+.1f: largest relative deviation from one exact product %.3e (bound 2^-24 = %.3e)" % (st, err, 2.0 ** -24))
            assert np.array_equal(got > 0, v) and err <= 2.0 ** -24
            # the integer shift of rvc.rs:121 on top: a power of two, exact
            assert np.array_equal(e.pitch(x, 12, FRAME16K), got * np.float32(2.0))
        e.set_pitch_semitones(7.0)
        seven = e.pitch(x, 7, FRAME16K)
        e.set_pitch_semitones(0.0)
        plain = e.pitch(x, 7, FRAME16K)
        assert np.array_equal(plain, got0)                      # pitch_shift = 7 alone: the reference's truncating division shifts nothing
        assert not np.array_equal(seven, plain) and np.all(seven[got0 > 0] > 1.49 * got0[got0 > 0])
        # bad arguments: RVC_SHAPE, and the value stays
        e.set_pitch_semitones(0.5)
        half = e.pitch(x, 0, FRAME16K)
        bad = [lambda: e.set_pitch_semitones(24.5), lambda: e.set_pitch_semitones(-25.0), lambda: e.set_pitch_semitones(float("nan")),
               lambda: e.set_pitch_semitones(1.0, stream=1), lambda: e.set_pitch_semitones(1.0, stream=-1),
               lambda: e.set_f0_range(-1.0, 100.0), lambda: e.set_f0_range(200.0, 100.0), lambda: e.set_f0_range(float("nan"), 100.0),
               lambda: e.set_f0_range(0.0, float("nan")), lambda: e.set_f0_range(0.0, 100.0, stream=1),
               lambda: e.set_f0_median(8), lambda: e.set_f0_median(-1), lambda: e.set_f0_median(1, stream=1),
               lambda: e.set_f0_snap(0x1000, 1.0), lambda: e.set_f0_snap(SCALE_C_MAJOR, 1.5), lambda: e.set_f0_snap(SCALE_C_MAJOR, -0.1),
               lambda: e.set_f0_snap(SCALE_C_MAJOR, float("nan")), lambda: e.set_f0_snap(SCALE_C_MAJOR, 1.0, stream=1)]
        for f in bad:
            with pytest.raises(RvcInferError) as ei:
                f()
            assert ei.value.kind == "NdarrayShapeError" and str(ei.value) != "NdarrayShapeError"          # (with a message)
        assert np.array_equal(e.pitch(x, 0, FRAME16K), half)
        e.set_pitch_semitones(24.0); e.set_pitch_semitones(-24.0); e.set_f0_range(0.0, float("inf")); e.set_f0_snap("A minor", 0.0)
        assert scale_mask("A", "minor") == SCALE_C_MAJOR and scale_mask(0, "chromatic") == SCALE_CHROMATIC
    finally:
        _apply(e, F.NEUTRAL)
    assert np.array_equal(e.pitch(x, 0, FRAME16K), got0)


# ---- 3. median, 4. range gate, 5. snap: rvc_pitch on both inputs ----
@pytest.mark.parametrize("name,case", F.PITCH_CASES)
def test_pitch_against_the_reference(base, name, case):
    e, b = base["engine"], base[name]
    c = F.CASES[case]
    bound = _bound(b, case)
    ref, margin, gm, _ = F.condition(b["ref"], parts=True, **F.settings(case))
    sure = _sure(b["margin"], margin, gm, c["r"])
    try:
        _apply(e, case)
        got = e.pitch(b["x"], 0, FRAME16K)
    finally:
        _apply(e, F.NEUTRAL)
    assert got.shape == (32,) and got.dtype == np.float32
    _check(got, ref, sure, bound, "%s / %s" % (name, case))
    got0 = b["got0"]
    if c["r"]:
        # structure: pure selection -- the filtered rows are medfilt of the same engine's unfiltered rows, bit for bit
        assert np.array_equal(got, medfilt(got0, 2 * c["r"] + 1)) and not np.array_equal(got, got0)
    if case == "gate":
        keep = got > 0
        assert np.array_equal(got[keep], got0[keep]) and np.any((got0 > 0) & ~keep) and keep.any()
        assert np.all((got[keep] >= c["lo"]) & (got[keep] <= c["hi"]))
    if c["mask"]:
        assert np.array_equal(got > 0, got0 > 0)
        if c["s"] == 1.0:
            _on_allowed_notes(got, c["mask"], bound, "%s / %s" % (name, case))
        else:
            assert not np.array_equal(got, got0)


def test_pitch_over_the_default_converter_window():
    """the file converter's default window (k = 14): 71 520 samples, n == the f0 frame, 448 rows in the LDS-resident window.  A median of width 7 and a
    C major snap of strength 0.7 (case `stream1`) filter it across its whole length; the same reference, margins and bound rule as above"""
    frame16k, case = 5120 * 13, "stream1"
    x = Y.whole_window_signal(frame16k)
    assert len(x) == Y.f0_frame(frame16k) == 71520
    c = F.CASES[case]
    ref0, ymargin = Y.yin(x, frame16k)
    b = {"ref": ref0, "margin": ymargin, "f32": Y.yin(x, frame16k, np.float32)[0]}
    bound = _bound(b, case)
    ref, margin, gm, _ = F.condition(ref0, parts=True, **F.settings(case))
    sure = _sure(ymargin, margin, gm, c["r"])
    e = _engine(zoo("tiny"), full=False)
    try:
        got0 = e.pitch(x, 0, frame16k)
        _apply(e, case)
        got = e.pitch(x, 0, frame16k)
    finally:
        e.close()
    assert got.shape == (448,) and got.dtype == np.float32
    v = _check(got, ref, sure, bound, "whole window / %s" % case)
    assert v[-4:].any() and v.sum() >= 224                              # voiced rows at the window's end, where the median's window leaves the buffer
    assert not np.array_equal(got, got0)
    # structure: with the snap off the filtered rows are medfilt of the same engine's unfiltered rows, bit for bit, over all 448
    e = _engine(zoo("tiny"), full=False)
    try:
        _apply(e, "median3")
        assert np.array_equal(e.pitch(x, 0, frame16k), medfilt(got0, 7))
    finally:
        e.close()


# ---- 6. per stream, two chunks, three streams ----
def _cache_ref(chunks, case, pitch_shift):
    """reference pitch cache of one stream after the chunks (infer calls: the formant factor (float)2^0 is part of the multiplier), and which entries are sure"""
    c = F.CASES[case] if case != "neutral" else F.NEUTRAL
    kw = {k: c[k] for k in ("lo", "hi", "r", "mask", "s")}
    cache, sure = np.zeros(1024), np.ones(1024)
    for x in chunks:
        f0, ym = Y.yin(x, FRAME16K)
        rows, margin, gm, _ = F.condition(f0, F.multiplier(pitch_shift, c["st"], 0.0), parts=True, **kw)
        ok = (F.window_min(ym, c["r"]) >= YIN_MARGIN) & (margin >= F.SNAP_MARGIN) & (gm >= F.GATE_MARGIN)
        cache, _ = Y.update_cache(cache, rows, SHIFT, CACHE_START, 0, 0)
        sure, _ = Y.update_cache(sure, ok.astype(np.float64), SHIFT, CACHE_START, 0, 0)
    return cache, sure > 0


def _stream_bound(chunks, case, pitch_shift):
    c = F.CASES[case] if case != "neutral" else F.NEUTRAL
    worst = 0.0
    for x in chunks:
        b = {"ref": Y.yin(x, FRAME16K)[0], "f32": Y.yin(x, FRAME16K, np.float32)[0], "margin": Y.yin(x, FRAME16K)[1]}
        kw = {k: c[k] for k in ("lo", "hi", "r", "mask", "s")}
        up = F.multiplier(pitch_shift, c["st"], 0.0)
        ref, margin, gm, _ = F.condition(b["ref"], up, parts=True, **kw)
        f32, _ = F.condition(b["f32"], up, dtype=np.float32, **kw)
        v = (ref > 0) & (f32 > 0) & (F.window_min(b["margin"], kw["r"]) >= YIN_MARGIN) & (margin >= F.SNAP_MARGIN) & (gm >= F.GATE_MARGIN)
        worst = max(worst, float(np.max(np.abs(f32[v].astype(np.float64) - ref[v]) / ref[v])) if v.any() else 0.0)
    bound = max(8.0 * worst, 1e-6)
    print("float32 numpy against float64 (%s): %.3e -> bound %.3e" % (case, worst, bound))
    return bound


def _check_cache(got, chunks, case, pitch_shift, what):
    ref, sure = _cache_ref(chunks, case, pitch_shift)
    lo = CACHE_START - SHIFT * (len(chunks) - 1)
    assert np.all(got[:lo] == 0.0)
    assert np.sum(~sure[lo:]) <= 0.10 * (1024 - lo)
    v = _check(got[lo:], ref[lo:], sure[lo:], _stream_bound(chunks, case, pitch_shift), what)
    assert v.sum() >= 6


def test_per_stream_settings_two_chunks():
    z = zoo("tiny")
    sr = _sr(z)
    xs = F.stream_chunks()
    shifts = [s for _, s in F.STREAM_CASES]
    e, plain = _engine(z, streams=3), _engine(z, streams=3)
    _apply(e, "stream1", 1)
    _apply(e, "stream2", 2)
    for k in range(2):
        y = e.infer_batch(xs[k], FRAME16K, shifts, g.skip_head, R)
        yp = plain.infer_batch(xs[k], FRAME16K, shifts, g.skip_head, R)
        assert y.shape == (3, R * sr // 100) and np.all(np.isfinite(y))
        assert np.array_equal(y[0], yp[0])                                        # the stream with nothing set: the settings-free engine's PCM
    assert np.array_equal(e.pitch_cache(0), plain.pitch_cache(0)) and np.any(e.pitch_cache(0) > 0)
    assert not np.array_equal(e.pitch_cache(1), plain.pitch_cache(1)) and not np.array_equal(e.pitch_cache(2), plain.pitch_cache(2))
    for s, (case, shift) in enumerate(F.STREAM_CASES):
        _check_cache(e.pitch_cache(s), [xs[0][s], xs[1][s]], case, shift, "stream %d (%s)" % (s, case))
    # rvc_reset_state leaves the settings alone; a stream added later gets the engine-wide default
    e.reset_state()
    e.infer_batch(xs[0], FRAME16K, shifts, g.skip_head, R)
    _check_cache(e.pitch_cache(1), [xs[0][1]], "stream1", 0, "stream 1 after reset_state")
    e.close(); plain.close()


# ---- 7. no plan rebuild; graph replay; chunk pipelining; geometry buckets ----
def test_settings_change_between_chunks_without_a_plan_build():
    import torch
    z = zoo("tiny")
    sr = _sr(z)
    xs = F.stream_chunks()
    x0, x1 = xs[0][0], xs[1][1]
    N = R * sr // 100

    def run(mode):
        e = _engine(z)
        if mode == "graph":
            e.set_use_graph(True)
        if mode == "pipeline":
            e.set_pipeline(True)
            d_in = torch.from_numpy(np.stack([x0, x1])).cuda()
            d_out = torch.zeros((2, N), device="cuda")
            torch.cuda.synchronize()
        builds = []
        for k, x in enumerate((x0, x1)):
            if k == 1:
                _apply(e, "changed")
            if mode == "pipeline":
                e.infer_device(d_in[k].data_ptr(), L, FRAME16K, 12, g.skip_head, R, d_out[k].data_ptr(), N, sync=False)
            else:
                assert np.all(np.isfinite(e.infer(x, FRAME16K, 12, g.skip_head, R)))
            builds.append(e.plan_cache_info()["builds"])
        e.synchronize()
        cache = e.pitch_cache()
        e.close()
        return cache, builds
    eager, builds = run("eager")
    assert builds[0] == builds[1], builds                                         # the settings are no part of a plan's identity
    c = F.CASES["changed"]
    ref, sure = np.zeros(1024), np.ones(1024)
    for k, x in enumerate((x0, x1)):
        cc = c if k == 1 else F.NEUTRAL
        f0, ym = Y.yin(x, FRAME16K)
        rows, margin, gm, _ = F.condition(f0, F.multiplier(12, cc["st"], 0.0), parts=True, **{q: cc[q] for q in ("lo", "hi", "r", "mask", "s")})
        ok = (F.window_min(ym, cc["r"]) >= YIN_MARGIN) & (margin >= F.SNAP_MARGIN)
        ref, _ = Y.update_cache(ref, rows, SHIFT, CACHE_START, 0, 0)
        sure, _ = Y.update_cache(sure, ok.astype(np.float64), SHIFT, CACHE_START, 0, 0)
    lo = CACHE_START - SHIFT
    assert np.sum(sure[lo:] <= 0) <= 0.10 * (1024 - lo)
    _check(eager[lo:], ref[lo:], sure[lo:] > 0, _stream_bound([x1], "changed", 12), "eager, settings changed before chunk 2")
    graph, gb = run("graph")
    assert np.array_equal(graph, eager) and gb[0] == gb[1], gb
    piped, pb = run("pipeline")
    assert np.array_equal(piped, eager)
    assert pb[1] <= pb[0] + 1, pb                # (the second chunk of a pipelined pair runs in the other plan slot: one build whatever the settings)

    # one rvc_infer_batch_g call, two geometries: every stream keeps its settings
    e = _engine(z, streams=3)
    _apply(e, "stream1", 1)
    _apply(e, "stream2", 2)
    shifts = [s for _, s in F.STREAM_CASES]
    ys = e.infer_batch_g(list(xs[0]), [FRAME16K] * 3, shifts, [g.skip_head, g.skip_head + 2, g.skip_head], [R, R - 2, R])
    assert [len(y) for y in ys] == [N, (R - 2) * sr // 100, N] and all(np.all(np.isfinite(y)) for y in ys)
    for s, (case, shift) in enumerate(F.STREAM_CASES):
        _check_cache(e.pitch_cache(s), [xs[0][s]], case, shift, "batch_g stream %d (%s)" % (s, case))
    e.close()


# ---- 8. RMVPE as the source ----
def test_rmvpe_source_median_and_transpose():
    """Structure only (selection plus one rounding); the unconditioned rows stay pinned to the oracle by the existing parity tests.  The seeded tiny
    network calls all 32 rows of the composite input voiced (the CPU oracle says so too), between 180 and 205 Hz."""
    z = zoo("tiny")
    x = voice_signal(L, seed=3)
    x[-4960:] = Y.composite_signal()[-4960:]
    e, twin = _engine(z, "rmvpe"), _engine(z, "rmvpe")
    rows = twin.pitch(x, 0, FRAME16K)
    assert rows.shape == (32,) and np.sum(rows > 0) >= 6
    e.set_f0_median(3); e.set_pitch_semitones(3.0)
    assert np.all(np.isfinite(e.infer(x, FRAME16K, 12, g.skip_head, R)))
    want = medfilt(rows * np.float32(np.float32(2.0) * np.float32(2.0 ** (3.0 / 12.0))), 7)          # pitch_shift 12: exact; then one float factor
    assert not np.array_equal(want, medfilt(rows, 7) * np.float32(2.0)) and not np.array_equal(medfilt(rows, 7), rows)
    ref, _ = Y.update_cache(np.zeros(1024), want.astype(np.float64), SHIFT, CACHE_START, 0, 0)
    assert np.array_equal(e.pitch_cache().astype(np.float64), ref)
    assert np.array_equal(e.pitch(x, 12, FRAME16K), want)                         # rvc_pitch: the same rows
    e.close(); twin.close()


# ---- 9. native session ----
def test_native_session_honours_the_engine_settings():
    from obs_rvc_amd.streaming import NativeStreamingSession
    z = zoo("tiny")
    sr = _sr(z)
    rng = np.random.default_rng(5)

    def run(conditioned):
        e = _engine(z, streams=2)
        if conditioned:
            _apply(e, "session", 0)
        s = NativeStreamingSession(e, 48000, 0.16, 0.07, 2.0, sr, 12, 0.6)
        assert s.sample_frame_16k == FRAME16K and s.sample_frame_size == 7680
        outs = []
        for k in range(2):
            outs.append(s.process_one_frame(audio[:, k * s.sample_frame_size:(k + 1) * s.sample_frame_size]))
        caches = [e.pitch_cache(0), e.pitch_cache(1)]
        del s
        e.close()
        return np.stack(outs), caches
    n = 2 * 7680
    t = np.arange(n) / 48000.0
    audio = np.stack([(0.2 * sum(np.sin(2 * np.pi * f * k * t) / k for k in range(1, 5)) + 1e-3 * rng.standard_normal(n)).astype(np.float32) for f in (150.0, 171.0)])
    out, caches = run(True)
    ref_out, ref_caches = run(False)
    assert out.shape == ref_out.shape and np.all(np.isfinite(out))
    # the stream left neutral: the neutral session, bit for bit
    assert np.array_equal(out[:, 1], ref_out[:, 1]) and np.array_equal(caches[1], ref_caches[1])
    assert np.any(ref_caches[0] > 0) and not np.array_equal(caches[0], ref_caches[0])
    assert np.array_equal(caches[0] > 0, ref_caches[0] > 0)
    # chromatic snap at strength 1: every voiced entry sits on an equal-tempered note (the bound of the chromatic case: its floor, 1e-6)
    _on_allowed_notes(caches[0], SCALE_CHROMATIC, 1e-6, "session cache")
    # and it is the neutral entry moved by st = +4 and snapped: within half a semitone of +4 (pitch_shift 12 is in both)
    v = caches[0] > 0
    d = 12.0 * np.log2(caches[0][v].astype(np.float64) / ref_caches[0][v])
    assert np.all(np.abs(d - 4.0) <= 0.5 + 1e-3), d
