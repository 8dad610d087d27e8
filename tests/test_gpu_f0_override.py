"""f0 from outside (obs_rvc_amd/csrc/f0_override.hip.h) on the tiny zoo, Tm = 32: the three kernels alone through rvc_debug_f0_override
against tests/f0_override_ref.py, rvc_pitch with an override under YIN, RMVPE and hybrid[pm+yin] against tests/f0cond_ref.py on the selected rows, an all-NaN
override as a different plan with the same bits, consumption / hold / reset, graph replay, pipelined calls, buckets and the session, a conversion under a
curve against the composition of public calls, a model without pitch guidance, and every refusal.

Bounds.  Selection, the NaN pattern, zeros and copied values: bit for bit.  Interpolated grid rows: the same recipe in float32 numpy against float64, times 8,
floor 1e-6 (the rule of sections 11 and 12), computed here from the test's own curves.  Conditioned rows: the bound of tests/test_gpu_f0cond.py."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

import f0_override_ref as O
import f0cond_ref as F
import pm_ref as P
from common import BASELINE_160MS as g, voice_signal, zoo
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError

pytestmark = pytest.mark.gpu

FRAME16K, R, L = g.sample_frame_16k, g.model_return_length, g.input_buffer_16k_size
FR, TM = 4960, 32
CACHE_START = 1024 + 4 - TM          # the rows f0[3 : 31] of the last chunk (rvc.rs:168-179)
_FP, _IP, _LP, _DP = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_double)
nan = np.float32(np.nan)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _engine(method="yin", streams=1, full=True, model=None):
    z = zoo("tiny")
    e = RvcInfer(z["data"])
    if full:
        e.load_contentvec(2); e.load_model(model or z["model"])
    if method:
        e.load_f0_method(method)
    if streams > 1:
        e.set_streams(streams)
    e.set_noise_seed(1234, 0)
    return e


def _sr():
    return int(W.read_blob(zoo("tiny")["model"])[0]["sr"])


def _inputs(S, chunk):
    """S buffers of the chunk's length with different audio; chunk 1's f0 windows are the PM test inputs"""
    xs = np.stack([voice_signal(L, seed=10 * chunk + s + 1) for s in range(S)])
    if chunk == 1:
        xs[:, -FR:] = P.stream_signals()[np.arange(S) % 3][:, -FR:]
    return xs


def _ov_rows(n, seed):
    """n override rows of every kind: NaN, 0 and voiced"""
    rng = np.random.default_rng(seed)
    ov = rng.uniform(60.0, 900.0, n).astype(np.float32)
    kind = rng.integers(0, 3, n)
    ov[kind == 0] = nan
    ov[kind == 1] = 0.0
    if n >= 3:
        ov[:3] = (nan, 0.0, 321.5)
    return ov


def _debug(e, op, rows=None, ov=None, ov_n=None, geo=None, t=None, out=None):
    rows = None if rows is None else np.ascontiguousarray(rows, np.float32)
    ov = np.ascontiguousarray(ov, np.float32)
    B, Tm = rows.shape if rows is not None else (0, 0)
    cnt = None if ov_n is None else np.ascontiguousarray(ov_n, np.int32)
    geo = None if geo is None else np.ascontiguousarray(geo, np.int64)
    t = None if t is None else np.ascontiguousarray(t, np.float64)
    rc = e._L.rvc_debug_f0_override(e._h, op, None if rows is None else rows.ctypes.data_as(_FP), B, Tm, ov.ctypes.data_as(_FP),
                                    None if cnt is None else cnt.ctypes.data_as(_IP), None if geo is None else geo.ctypes.data_as(_LP),
                                    None if t is None else t.ctypes.data_as(_DP), 0 if t is None else len(t), out.ctypes.data_as(_FP))
    assert rc == 0, e._L.rvc_last_error_message(e._h)
    return out


@pytest.fixture(scope="module")
def bare():
    e = _engine(full=False)
    yield e
    e.close()


# ---------------------------------------------------------------- 1. the kernels alone
def _tracker_rows(B, seed=5):
    rng = np.random.default_rng(seed)
    rows = rng.uniform(50.0, 1100.0, (B, TM)).astype(np.float32)
    rows[:, 1::5] = 0.0
    rows[:, 2::7] = nan
    return rows


@pytest.mark.parametrize("n", [1, 31, 32])
def test_select_one_stream(bare, n):
    rows, ov = _tracker_rows(1), _ov_rows(n, n)
    buf = np.full((1, 1024), 777.0, np.float32); buf[0, :n] = ov
    got = _debug(bare, 0, rows, buf, [n], out=np.zeros((1, TM), np.float32))
    assert same_bits(got[0], O.select(rows[0], O.align_end(ov, TM)))
    assert same_bits(got[0, : TM - n], rows[0, : TM - n])          # the rows in front of the first override row keep the tracker's value


def test_select_three_streams_and_the_gather(bare):
    rows = _tracker_rows(3, 6)
    ns = [32, 0, 7]          # stream 1 brings nothing: all NaN
    buf = np.full((3, 1024), 777.0, np.float32)
    ovs = [_ov_rows(n, 40 + n) for n in ns]
    for s, ov in enumerate(ovs):
        buf[s, : len(ov)] = ov
    got = _debug(bare, 0, rows, buf, ns, out=np.zeros((3, TM), np.float32))
    for s in range(3):
        assert same_bits(got[s], O.select(rows[s], O.align_end(ovs[s], TM))), s
    assert same_bits(got[1], rows[1])
    # the gather of a conversion: H = 20, C = 5, 47 grid frames = 3 windows; a batch of 3 from window 1 on has one padding window
    geo = {"H": 20, "C": 5, "Tm": TM, "Nf": 47, "W": 3}
    grid = _ov_rows(47, 9)
    for w0, nw in ((0, 3), (1, 2), (2, 1)):
        got = _debug(bare, 1, rows, grid, geo=[47, w0, nw, 20, 5], out=np.zeros((3, TM), np.float32))
        for s in range(3):
            want = O.select(rows[s], O.window_override(grid, geo, w0 + s) if s < nw else np.full(TM, nan))
            assert same_bits(got[s], want), (w0, s)


def _grid_check(got, t, hz, Nf, what):
    ref, r32 = O.curve_grid(t, hz, Nf), O.curve_grid(t, hz, Nf, np.float32)
    T, hz = 100.0 * np.asarray(t, np.float64), np.asarray(hz, np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    copied = ok & (np.isin(np.arange(Nf, dtype=np.float64), T) | (ref == 0) | np.isin(ref, hz.astype(np.float64)))
    assert np.array_equal(got[copied].astype(np.float64), ref[copied]), what          # zeros and copied values, bit for bit
    v = ok & (ref > 0)
    dev = float(np.max(np.abs(r32[v].astype(np.float64) - ref[v]) / ref[v])) if v.any() else 0.0
    err = float(np.max(np.abs(got[v].astype(np.float64) - ref[v]) / ref[v])) if v.any() else 0.0
    bound = max(8.0 * dev, 1e-6)
    print("%s: float32 numpy against float64 %.3e -> bound %.3e, device %.3e on %d rows" % (what, dev, bound, err, v.sum()))
    assert err <= bound, (what, err)
    return err


@pytest.mark.parametrize("Nf", [1, 2, 333])
def test_grid_kernel(bare, Nf):
    for k, (t, hz) in enumerate(O.gpu_curves()):
        got = _debug(bare, 2, None, hz, geo=[Nf], t=t, out=np.zeros(Nf, np.float32))
        _grid_check(got, t, hz, Nf, "curve %d, Nf %d" % (k, Nf))


@pytest.mark.parametrize("nW", [1, 2, 5])
def test_export_kernel(bare, nW):
    g0 = O.geometry(2, 3, 1, 1)
    geo = O.geometry(2, 3, 1, nW * g0["H"] - 7)
    assert geo["W"] == nW
    rows = np.random.default_rng(nW).uniform(0.0, 500.0, (nW, geo["Tm"])).astype(np.float32)
    want, hits = O.export(rows, geo)
    assert np.all(hits == 1)
    out = np.full(geo["Nf"], -1.0, np.float32)
    for w0 in range(0, nW, 2):          # batches of two windows, the last one short
        nw = min(2, nW - w0)
        batch = np.zeros((2, geo["Tm"]), np.float32); batch[:nw] = rows[w0: w0 + nw]
        out = _debug(bare, 3, batch, np.zeros(1, np.float32), geo=[geo["Nf"], w0, nw, geo["H"], geo["C"]], out=out)
    assert same_bits(out, want)


# ---------------------------------------------------------------- 2. rvc_pitch with an override
@pytest.mark.parametrize("method", ["yin", "rmvpe", "hybrid[pm+yin]"])
def test_pitch_with_an_override(method):
    e = _engine(method, full=False)
    x = P.stream_signals()[0]
    base = e.pitch(x, 0, FRAME16K)
    assert base.shape == (TM,)
    ov = _ov_rows(TM, 3)
    sel = O.select(base, ov)
    e.set_f0_override(0, ov)
    got = e.pitch(x, 0, FRAME16K)
    assert same_bits(got, sel)                                   # pitch_shift 0, no control: pure selection
    assert same_bits(e.pitch(x, 0, FRAME16K), base)              # ... consumed by that call
    e.set_f0_override(0, ov[-9:])
    assert same_bits(e.pitch(x, 12, FRAME16K), O.select(base, O.align_end(ov[-9:], TM)) * np.float32(2.0))
    # the controls act on overridden rows: a 3-semitone transpose and a median of radius 1, against tests/f0cond_ref.py on the selected rows
    sel0 = np.where(np.isnan(sel), 0.0, sel).astype(np.float32)          # (NaN rows of the tracker: none here)
    assert not np.any(np.isnan(sel))
    try:
        e.set_pitch_semitones(3.0); e.set_f0_median(1)
        e.set_f0_override(0, ov)
        cond = e.pitch(x, 0, FRAME16K)
    finally:
        e.set_pitch_semitones(0.0); e.set_f0_median(0)
    up = F.multiplier(0, 3.0)
    want, _ = F.condition(sel0.astype(np.float64), up, r=1)
    w32, _ = F.condition(sel0, up, r=1, dtype=np.float32)
    v = want > 0
    dev = float(np.max(np.abs(w32[v].astype(np.float64) - want[v]) / want[v]))
    bound = max(8.0 * dev, 1e-6)
    assert np.array_equal(cond > 0, v)
    err = float(np.max(np.abs(cond[v].astype(np.float64) - want[v]) / want[v]))
    print("%s, transpose + median on overridden rows: float32 numpy %.3e -> bound %.3e, device %.3e" % (method, dev, bound, err))
    assert err <= bound
    assert np.any(cond != base)
    e.close()


# ---------------------------------------------------------------- 3. a different plan, the same numbers
def _two_chunks(e, S, before=None):
    ys = []
    for c in range(2):
        if before:
            before(e, c)
        x = _inputs(S, c)
        ys.append(e.infer(x[0], FRAME16K, 12, g.skip_head, R) if S == 1 else e.infer_batch(x, FRAME16K, (12, 0, -12)[:S], g.skip_head, R))
    return np.stack(ys), np.stack([e.pitch_cache(s) for s in range(S)])


@pytest.mark.parametrize("method", ["yin", "rmvpe"])
@pytest.mark.parametrize("S", [1, 3])
def test_all_nan_override_is_neutral(method, S):
    e = _engine(method, S)
    plain, cache = _two_chunks(e, S)
    if S == 1:
        p0 = e.pitch(_inputs(1, 1)[0], 0, FRAME16K)
    e.close()
    e = _engine(method, S)
    builds = lambda: e.plan_cache_info()["builds"]
    b0 = builds()

    def all_nan(e, c):
        for s in range(S):
            e.set_f0_override(s, np.full(TM if s != 1 else 5, nan))
    ys, cache2 = _two_chunks(e, S, all_nan)
    assert builds() == b0 + 1                                    # one plan for the two chunks: the values are no part of its identity
    assert same_bits(ys, plain) and same_bits(cache2, cache)
    if S == 1:
        e.set_f0_override(0, np.full(TM, nan))
        b1 = builds()
        assert same_bits(e.pitch(_inputs(1, 1)[0], 0, FRAME16K), p0) and builds() == b1 + 1
    e.reset_state()
    b1 = builds()
    _two_chunks(e, S)                                            # no override: the plain plan, built now
    assert builds() == b1 + 1
    e.set_f0_override(0, _ov_rows(TM, 1)); _two_chunks(e, S)
    e.set_f0_override(S - 1, _ov_rows(7, 2)); _two_chunks(e, S)
    assert builds() == b1 + 1                                    # both kinds are cached: neither new values nor going back builds anything
    e.close()


# ---------------------------------------------------------------- 4. consumption, hold, reset
def test_consumption_hold_reset():
    ov = np.linspace(120.0, 240.0, TM).astype(np.float32)
    e = _engine("yin", full=False)
    tracker = e.pitch(_inputs(1, 1)[0], 0, FRAME16K)          # the tracker's rows, on an engine that never had an override
    e.close()
    assert not same_bits(tracker, ov)

    def run(kind):
        e = _engine("yin")
        e.set_f0_override_hold(kind != "oneshot")
        e.set_f0_override(0, ov)
        y0 = e.infer(_inputs(1, 0)[0], FRAME16K, 0, g.skip_head, R)
        if kind == "cleared":
            e.set_f0_override(0, None)
        y1 = e.infer(_inputs(1, 1)[0], FRAME16K, 0, g.skip_head, R)
        cache = e.pitch_cache()
        if kind == "held":
            held = e.pitch(_inputs(1, 1)[0], 0, FRAME16K)
            assert same_bits(held, ov)                                    # still pending, and rvc_pitch honours it
            e.reset_state()
            after = e.pitch(_inputs(1, 1)[0], 0, FRAME16K)                # hold is still on: only rvc_reset_state can have taken the override away
            assert same_bits(after, tracker) and not same_bits(after, ov)
        e.close()
        return y0, y1, cache
    a, b, c = run("oneshot"), run("cleared"), run("held")
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])          # chunk 2 after a one-shot = chunk 2 of a run that had none
    assert same_bits(a[0], c[0]) and not same_bits(a[1], c[1])
    assert same_bits(c[2][CACHE_START:], ov[3:31])               # held: the second chunk's rows are the override's (pitch_shift 0: exact)
    assert not same_bits(a[2][CACHE_START:], ov[3:31])
    shift = FRAME16K // 160
    assert same_bits(a[2][CACHE_START - shift: CACHE_START], ov[3: 3 + shift])          # ... and the first chunk's, moved down, in every run


# ---------------------------------------------------------------- 5. replay, pipelining, buckets, the session
def _ov_for(c, s):
    return np.linspace(100.0 + 50 * s + 20 * c, 300.0 + 10 * s, TM - 3 * s).astype(np.float32)


def test_replay_pipeline_buckets_session():
    import torch
    S, sr = 2, _sr()
    N = R * sr // 100

    def run(mode):
        e = _engine("rmvpe", S)
        if mode == "graph":
            e.set_use_graph(True)
        if mode == "pipeline":
            e.set_pipeline(True)
            d_in = torch.from_numpy(np.stack([_inputs(S, c) for c in range(2)])).cuda()
            d_out = torch.zeros((2, S, N), device="cuda")
            torch.cuda.synchronize()
        out = np.zeros((2, S, N), np.float32)
        for c in range(2):
            for s in range(S):
                e.set_f0_override(s, _ov_for(c, s))
            x = _inputs(S, c)
            if mode == "pipeline":
                e.infer_device(d_in[c].data_ptr(), L, FRAME16K, 0, g.skip_head, R, d_out[c].data_ptr(), N, sync=False)
            elif mode == "buckets":
                ys = e.infer_batch_g(list(x), [FRAME16K] * S, [0] * S, [g.skip_head, g.skip_head + 1], [R, R - 1])
                out[c, 0] = ys[0]; out[c, 1, : len(ys[1])] = ys[1]
            else:
                out[c] = e.infer_batch(x, FRAME16K, 0, g.skip_head, R)
        e.synchronize()
        if mode == "pipeline":
            out = d_out.cpu().numpy()
        caches = np.stack([e.pitch_cache(s) for s in range(S)])
        e.close()
        return out, caches
    eager, cache = run("eager")
    for s in range(S):          # every stream's cache ends in ITS override of the second chunk
        assert same_bits(cache[s][CACHE_START:], _ov_for(1, s)[3 - 3 * s: 31 - 3 * s]), s          # (its TM - 3 s rows end at the window's end)
    again, cache2 = run("eager")
    assert same_bits(eager, again) and same_bits(cache, cache2)
    for mode in ("graph", "pipeline"):
        out, c2 = run(mode)
        assert same_bits(c2, cache) and same_bits(out, eager), mode
    b1, cb1 = run("buckets")
    b2, cb2 = run("buckets")
    assert same_bits(b1, b2) and same_bits(cb1, cb2) and same_bits(cb1, cache)          # two geometries, two bucket plans: each stream got its own rows
    # the native session honours a held override
    from obs_rvc_amd.streaming import NativeStreamingSession
    e = _engine("yin")
    e.set_f0_override_hold(True)
    e.set_f0_override(0, np.full(TM, 200.0, np.float32))
    ses = NativeStreamingSession(e, 48000, 0.16, 0.07, 2.0, sr, 12, 0.6)
    assert ses.sample_frame_16k == FRAME16K
    audio = voice_signal(2 * ses.sample_frame_size, seed=4, sr=48000)
    for k in range(2):
        ses.process_one_frame(audio[k * ses.sample_frame_size:(k + 1) * ses.sample_frame_size])
    assert np.all(e.pitch_cache()[CACHE_START - 8:] == np.float32(400.0))          # 200 Hz, an octave up, in both chunks' rows
    del ses
    e.close()


# ---------------------------------------------------------------- 6. a conversion under a curve
K, CTX, XF, ZC = 2, 3, 1, 48
NREC = 20800          # 1.3 s: Nf = 130, H = 55, W = 3
CURVE_T = np.array([0.4537, 0.6021, 0.7013, 0.8479])
CURVE_HZ = np.array([150.0, 220.0, 0.0, 180.0], np.float32)


@pytest.mark.parametrize("S", [1, 2])
def test_conversion_under_a_curve(S):
    import convert_ref as CR
    x = voice_signal(NREC, seed=11)
    geo = RvcInfer.convert_geometry(len(x), 100 * ZC, K, CTX, XF)
    og = O.geometry(K, CTX, XF, 130)
    assert geo["windows"] == og["W"] == 3 and geo["hop"] == og["H"] and geo["n"] == 160 * og["F"]
    assert O.grid_margin(CURVE_T, 130) >= 1e-6
    e = _engine("rmvpe", S)
    conv = lambda: e.convert(x, k=K, context=CTX, crossfade=XF, pitch_shift=12, highpass=False)[0]
    with pytest.raises(RvcInferError):
        e.convert_f0()
    y0 = conv(); f0_0 = e.convert_f0(); off0 = e.convert_info()["offsets"]
    assert f0_0.shape == (130,) and np.any(f0_0 > 0)
    assert np.all(np.isnan(e.f0_curve_grid(130)))
    e.set_f0_curve(CURVE_T, CURVE_HZ)
    grid = e.f0_curve_grid(130)
    _grid_check(grid, CURVE_T, CURVE_HZ, 130, "the conversion's curve")
    y1 = conv(); f0_1 = e.convert_f0(); off1 = e.convert_info()["offsets"]
    cov = ~np.isnan(grid)
    assert cov.sum() == 39 and not cov[45] and cov[46] and cov[84] and not cov[85]
    assert same_bits(f0_1[cov], grid[cov] * np.float32(2.0))          # covered frames: the curve, conditioned (an octave up)
    assert same_bits(f0_1[~cov], f0_0[~cov])                           # uncovered frames: the tracker's, as without the curve
    assert not same_bits(y1, y0)
    # the composition: per-window infer_batch with the matching per-stream overrides, then the stitch
    win = CR.gather_windows(np.asarray(x, np.float32), geo)
    pad = np.concatenate([win, np.zeros(((-3) % S, geo["n"]), np.float32)])
    e.reset_state()
    ys = []
    for i in range(0, len(pad), S):
        for s in range(S):
            e.set_f0_override(s, O.window_override(grid, og, i + s) if i + s < 3 else None)
        ys.append(e.infer_batch(pad[i: i + S], geo["sample_frame_16k_size"], 12, geo["skip_head"], geo["return_length"]) if S > 1 else
                  e.infer(pad[i], geo["sample_frame_16k_size"], 12, geo["skip_head"], geo["return_length"])[None])
    audio, off = e.sola_stitch(np.concatenate(ys)[:3], XF * ZC, ZC, geo["hop"] * ZC)
    assert same_bits(audio[: geo["output_samples"]], y1) and np.array_equal(off, off1)
    # streaming calls never read the curve, and clearing it gives the first conversion back
    e.reset_state()
    p = e.infer_batch(_inputs(S, 1), FRAME16K, 0, g.skip_head, R) if S > 1 else e.infer(_inputs(1, 1)[0], FRAME16K, 0, g.skip_head, R)
    e.clear_f0_curve(); e.reset_state()
    q = e.infer_batch(_inputs(S, 1), FRAME16K, 0, g.skip_head, R) if S > 1 else e.infer(_inputs(1, 1)[0], FRAME16K, 0, g.skip_head, R)
    assert same_bits(p, q)
    y2 = conv()
    assert same_bits(y2, y0) and np.array_equal(e.convert_info()["offsets"], off0) and same_bits(e.convert_f0(), f0_0)
    # a conversion begins by clearing the streams' overrides: one started with a held override pending equals one started without
    e.set_f0_override_hold(True)
    for s in range(S):
        e.set_f0_override(s, np.full(TM, 300.0, np.float32))
    y3 = conv()
    assert same_bits(y3, y0) and same_bits(e.convert_f0(), f0_0)
    e.close()


# ---------------------------------------------------------------- 7. a model without pitch guidance, and every refusal
def test_a_model_without_pitch_guidance_ignores_both():
    z = zoo("tiny")
    path = os.path.join(os.path.dirname(z["model"]), "model-tiny-nof0-v2.rvcw")
    if not os.path.exists(path):
        W.write_blob(path, *W.make_synth("tiny", 48, f0=False))
    x, rec = _inputs(1, 1)[0], voice_signal(NREC, seed=11)
    e = _engine("yin", model=path)
    assert not e.model_has_f0()
    y0 = e.infer(x, FRAME16K, 0, g.skip_head, R)
    c0 = e.convert(rec, k=K, context=CTX, crossfade=XF, highpass=False)[0]
    e.reset_state()
    e.set_f0_override_hold(True)
    e.set_f0_override(0, np.full(TM, 300.0, np.float32))
    e.set_f0_curve(CURVE_T, CURVE_HZ)
    assert same_bits(e.infer(x, FRAME16K, 0, g.skip_head, R), y0)
    assert same_bits(e.convert(rec, k=K, context=CTX, crossfade=XF, highpass=False)[0], c0)
    with pytest.raises(RvcInferError):
        e.convert_f0()
    e.close()


def test_refusals_leave_the_state():
    e = _engine("yin", full=False)
    x = P.stream_signals()[0]
    ov = _ov_rows(TM, 8)
    e.set_f0_override_hold(True)
    e.set_f0_override(0, ov)
    want = e.pitch(x, 0, FRAME16K)
    bad = [(1, ov), (-1, ov), (0, np.zeros(1025, np.float32)), (0, np.float32([100.0, -1.0])), (0, np.float32([np.inf])), (0, np.float32([-np.inf])),
           (0, np.float32([20000.5]))]
    for stream, rows in bad:
        with pytest.raises(RvcInferError) as ei:
            e.set_f0_override(stream, rows)
        assert ei.value.kind == "NdarrayShapeError" and "f0 override" in str(ei.value)
        assert same_bits(e.pitch(x, 0, FRAME16K), want)
    with pytest.raises(RvcInferError):
        e._chk(e._L.rvc_set_f0_override_hold(e._h, 2))
    e.set_f0_override(0, np.float32([0.0, 20000.0, np.nan]))          # the edges are legal
    e.set_f0_override(0, np.full(TM + 1, 100.0, np.float32))          # more rows than this call's window: refused by the call, and it stays
    for _ in range(2):
        with pytest.raises(RvcInferError) as ei:
            e.pitch(x, 0, FRAME16K)
        assert "f0 window" in str(ei.value)
    e.set_f0_override(0, ov)
    assert same_bits(e.pitch(x, 0, FRAME16K), want)
    # the curve
    e.set_f0_curve(CURVE_T, CURVE_HZ)
    g0 = e.f0_curve_grid(100)
    for t, hz in (([0.1, 0.1], [1.0, 2.0]), ([0.2, 0.1], [1.0, 2.0]), ([0.1, np.inf], [1.0, 2.0]), ([0.1], [-1.0]), ([0.1], [np.nan]), ([0.1], [20001.0])):
        with pytest.raises(RvcInferError) as ei:
            e.set_f0_curve(t, hz)
        assert ei.value.kind == "NdarrayShapeError" and same_bits(e.f0_curve_grid(100), g0)
    out = np.zeros(4, np.float32)
    assert e._L.rvc_f0_curve_grid(e._h, 5, out.ctypes.data_as(_FP), 4) == 5
    n = C.c_size_t(77)
    assert e._L.rvc_convert_f0(e._h, out.ctypes.data_as(_FP), 4, C.byref(n)) == 5          # no conversion has completed
    e.close()
