"""The PM f0 method (rvc_load_f0_method(9), pm_peak_kernel + pm_cand_kernel + pm_path_kernel + the pitch tail) against the float64
restatement of tests/pm_ref.py: loading and plan identity, the candidates and the path alone through rvc_debug_pm, rvc_pitch and the pitch cache at 1 and 3
streams, two chunks eager / graph / pipelined, the pitch controls on top, the native session, formant shift, and PM as a hybrid member.
The smallest geometry: sample_frame_16k_size = 2560, an f0 window of 4960 samples, Tm = 32 frames.

Bounds (the rule of DESIGN.md sections 11 and 12): the same recipe in float32 numpy deviates from float64 by 1.77e-7 (f, relative), 3.31e-7 (s) and 3.40e-7
(delta, both absolute) on the three inputs; the kernels, whose summation order is not numpy's, are allowed 8 times the value measured on each run, floor 1e-6.
Candidates are compared on the frames whose float64 decision margin is at least 1e-5 (tests/test_pm_ref.py: all but frame 25 of stream 0); the path on
the frames whose path margin is at least 4 Tm 2^-24 times the sum of the absolute terms along the best path (all of them on these inputs)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import f0_hybrid_ref as H
import f0cond_ref as F
import pm_ref as P
import yin_ref as Y
from common import BASELINE_160MS as g, voice_signal, zoo
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc_common import F0_RMVPE, F0_YIN, RvcInferError

pytestmark = pytest.mark.gpu

FRAME16K = g.sample_frame_16k          # 2560
R = g.model_return_length
L = g.input_buffer_16k_size
FR, TM = 4960, 32
CAND_MARGIN = 1e-5
SHIFT, CACHE_START = FRAME16K // 160, 1024 + 4 - 32          # rvc.rs:168,172 at 32 frames
_FP = C.POINTER(C.c_float)
assert FRAME16K == 2560 and P.f0_frame(FRAME16K) == FR


def _engine(z, method="pm", streams=1, full=True):
    from obs_rvc_amd.rvc import RvcInfer
    e = RvcInfer(z["data"])
    if full:
        e.load_contentvec(2); e.load_model(z["model"])
    e.load_f0_method(method)
    if streams > 1:
        e.set_streams(streams)
    e.set_noise_seed(1234, 0)
    return e


def _debug_cand(e, X, with_path=False):
    """rvc_debug_pm (a) on X [B][n]: peak + candidates (and the path over them)"""
    X = np.ascontiguousarray(X, np.float32)
    B, n = X.shape
    cn = np.full((B, TM), -1, np.int32)
    cf, cs, cd = (np.full((B, TM, 15), np.nan, np.float32) for _ in range(3))
    path, f0 = np.full((B, TM), -1, np.int32), np.full((B, TM), np.nan, np.float32)
    rc = e._L.rvc_debug_pm(e._h, X.ctypes.data_as(_FP), B, n, FR, TM, cn.ctypes.data, cf.ctypes.data_as(_FP), cs.ctypes.data_as(_FP), cd.ctypes.data_as(_FP),
                           path.ctypes.data if with_path else None, f0.ctypes.data_as(_FP) if with_path else None)
    assert rc == 0, e._L.rvc_last_error_message(e._h)
    return {"n": cn, "f": cf, "s": cs, "delta": cd, "path": path, "f0": f0}


def _debug_path(e, n, f, delta):
    """rvc_debug_pm (b) on candidate arrays [B][Tm], [B][Tm][15]"""
    n, f, delta = np.ascontiguousarray(n, np.int32), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(delta, np.float32)
    B, Tm = n.shape
    path, f0 = np.full((B, Tm), -1, np.int32), np.full((B, Tm), np.nan, np.float32)
    rc = e._L.rvc_debug_pm(e._h, None, B, 0, 0, Tm, n.ctypes.data, f.ctypes.data_as(_FP), None, delta.ctypes.data_as(_FP), path.ctypes.data, f0.ctypes.data_as(_FP))
    assert rc == 0, e._L.rvc_last_error_message(e._h)
    return path, f0


@pytest.fixture(scope="module")
def pm_case():
    """the three inputs, their float64 references, the bounds from the float32 run of the same recipe, and one f0-only engine"""
    X = P.stream_signals()
    refs, dev = [], {"f": 0.0, "s": 0.0, "delta": 0.0}
    for s in range(3):
        f0, c, idx, pmargin, terms = P.pm(X[s], FRAME16K)
        c32 = P.candidates(X[s], FRAME16K, np.float32)
        keep = c["margin"] >= CAND_MARGIN
        pkeep = pmargin >= 4 * TM * 2.0 ** -24 * terms
        assert np.sum(~keep) <= 2 and np.sum(pkeep) >= 30          # (conditions on the input: tests/test_pm_ref.py)
        a, b = c["f"][keep], c32["f"][keep].astype(np.float64)
        dev["f"] = max(dev["f"], float(np.max(np.abs(a - b)[a > 0] / a[a > 0])))
        for k in ("s", "delta"):
            dev[k] = max(dev[k], float(np.max(np.abs(c[k][keep] - c32[k][keep].astype(np.float64)))))
        refs.append({"f0": f0, "c": c, "idx": idx, "keep": keep, "pkeep": pkeep})
    bound = {k: max(8.0 * v, 1e-6) for k, v in dev.items()}
    print("float32 numpy against float64 %s -> bounds %s" % (dev, bound))
    e = _engine(zoo("tiny"), full=False)
    yield {"X": X, "refs": refs, "bound": bound, "engine": e}
    e.close()


def _check_rows(got, ref, sure, bound, what=""):
    """f0 rows of the device against the reference: voicing on the sure rows, the relative error where both are voiced"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(got[sure] > 0, ref[sure] > 0), (what, np.where((got > 0) != (ref > 0))[0])
    v = (got > 0) & (ref > 0) & sure
    err = float(np.max(np.abs(got[v] - ref[v]) / ref[v])) if v.any() else 0.0
    print("%s: voiced %d of %d, left out %d, largest relative error %.3e (bound %.3e)" % (what, v.sum(), len(ref), np.sum(~sure), err, bound))
    assert err <= bound, (what, err)


def test_method_loading(tmp_path):
    from obs_rvc_amd.rvc import RvcInfer
    from obs_rvc_amd.rvc_common import F0_PM
    x = P.composite_signal()
    e = RvcInfer(str(tmp_path))                      # a data directory with nothing under f0/
    assert e.f0_method == 0
    e.load_f0_method("pm")
    assert e.f0_method == 9 == F0_PM
    e.load_f0_method(F0_YIN)
    e.load_f0_method(9)
    assert e.f0_method == 9
    for bad in (3, 6, 8, -1):
        with pytest.raises(RvcInferError) as ei:
            e.load_f0_method(bad)
        assert ei.value.kind == "NdarrayShapeError" and "RVC_F0_PM" in str(ei.value) and e.f0_method == 9
    with pytest.raises(ValueError):
        e.load_f0_method("harvest")
    f0 = e.pitch(x, 0, FRAME16K)
    assert f0.shape == (TM,) and np.all(np.isfinite(f0)) and np.any(f0 > 0) and f0[0] == 0.0
    e.close()


def test_plan_identity_between_the_methods(pm_case):
    x = pm_case["X"][0]
    e = _engine(zoo("tiny"), "rmvpe", full=False)
    builds = lambda: e.plan_cache_info()["builds"]
    b0 = builds()
    r1 = e.pitch(x, 0, FRAME16K); b1 = builds()
    e.load_f0_method("pm")
    p1 = e.pitch(x, 0, FRAME16K); b2 = builds()
    e.load_f0_method("yin")
    y1 = e.pitch(x, 0, FRAME16K); b3 = builds()
    assert b1 == b0 + 1 and b2 == b1 + 1 and b3 == b2 + 1          # a plan built under one method is not served under another
    e.load_f0_method("pm")
    p2 = e.pitch(x, 0, FRAME16K)
    e.load_f0_method("yin")
    y2 = e.pitch(x, 0, FRAME16K)
    assert builds() == b3                                           # switching back finds the old plans
    assert np.array_equal(p1, p2) and np.array_equal(y1, y2) and not np.array_equal(p1, y1) and not np.array_equal(p1, r1)
    assert e.f0_method == F0_YIN
    e.load_f0_method("rmvpe")
    assert e.f0_method == F0_RMVPE
    e.close()


@pytest.mark.parametrize("streams", [1, 3])
def test_candidates_against_the_reference(pm_case, streams):
    e, bound = pm_case["engine"], pm_case["bound"]
    got = _debug_cand(e, pm_case["X"][:streams])
    worst = {"f": 0.0, "s": 0.0, "delta": 0.0}
    for s in range(streams):
        c, keep = pm_case["refs"][s]["c"], pm_case["refs"][s]["keep"]
        # the unvoiced candidate's score is compared on every frame: no decision stands before it
        d0 = float(np.max(np.abs(got["delta"][s][:, 0] - c["delta"][:, 0])))
        assert np.all(got["f"][s][:, 0] == 0) and np.all(got["s"][s][:, 0] == 0) and d0 <= bound["delta"], d0
        for t in np.where(keep)[0]:
            n = int(c["n"][t])
            assert got["n"][s, t] == n, (s, t, got["n"][s, t], n)
            gf, gs, gd = (got[k][s, t].astype(np.float64) for k in ("f", "s", "delta"))
            assert np.all(gf[n + 1:] == 0) and np.all(gs[n + 1:] == 0) and np.all(gd[n + 1:] == 0)
            if n:
                assert np.all(gf[1:n + 1] > 0) and np.max(np.abs(16000.0 / gf[1:n + 1] - 16000.0 / c["f"][t, 1:n + 1])) < 0.01, (s, t)          # the same lags
                worst["f"] = max(worst["f"], float(np.max(np.abs(gf[1:n + 1] - c["f"][t, 1:n + 1]) / c["f"][t, 1:n + 1])))
                worst["s"] = max(worst["s"], float(np.max(np.abs(gs[1:n + 1] - c["s"][t, 1:n + 1]))))
                worst["delta"] = max(worst["delta"], float(np.max(np.abs(gd[1:n + 1] - c["delta"][t, 1:n + 1]))))
    print("%d stream(s): largest deviation %s (bounds %s)" % (streams, worst, bound))
    for k in worst:
        assert worst[k] <= bound[k], (k, worst[k], bound[k])


def test_path_against_the_reference(pm_case):
    e = pm_case["engine"]
    refs = pm_case["refs"]
    n = np.stack([r["c"]["n"] for r in refs])
    f = np.stack([r["c"]["f"] for r in refs]).astype(np.float32)
    d = np.stack([r["c"]["delta"] for r in refs]).astype(np.float32)
    for B in (1, 3):
        path, f0 = _debug_path(e, n[:B], f[:B], d[:B])
        for s in range(B):
            pk = refs[s]["pkeep"]
            print("streams %d, stream %d: %d of %d frames over the path margin, %d differ" % (B, s, pk.sum(), TM, np.sum(path[s] != refs[s]["idx"])))
            assert np.array_equal(path[s][pk], refs[s]["idx"][pk]), (B, s, path[s], refs[s]["idx"])
            assert np.array_equal(f0[s], f[s][np.arange(TM), path[s]])


def test_path_at_the_longest_window():
    """Tm = 1024, synthetic candidates: the back-pointer storage at its largest, 16 staged chunks.  A slow random walk in log-frequency with a decoy an
    octave up and up to 12 weaker candidates per frame, unvoiced stretches, and frames with 14 candidates"""
    Tm = 1024
    n, f, d = P.synthetic_candidates(Tm)
    f32, d32 = f.astype(np.float32), d.astype(np.float32)
    idx, f0, margin, terms = P.path(n, f32, d32)
    thr = 4 * Tm * 2.0 ** -24 * terms
    sure = margin >= thr
    print("Tm 1024: %d frames over the path margin %.3e, voiced %d" % (sure.sum(), thr, np.sum(f0 > 0)))
    assert sure.sum() >= 0.9 * Tm and np.sum(f0 > 0) > 500 and np.sum(f0 == 0) > 200
    e = _engine(zoo("tiny"), full=False)
    path, got = _debug_path(e, n[None], f32[None], d32[None])
    e.close()
    assert np.array_equal(path[0][sure], idx[sure]), np.where(path[0] != idx)[0]
    assert np.array_equal(got[0], f32[np.arange(Tm), path[0]])


def test_pitch_against_the_reference(pm_case):
    e = pm_case["engine"]
    x, r = pm_case["X"][0], pm_case["refs"][0]
    got = e.pitch(x, 0, FRAME16K)
    assert got.shape == (TM,)
    _check_rows(got, r["f0"], r["keep"] & r["pkeep"], pm_case["bound"]["f"], "rvc_pitch")
    both = _debug_cand(e, x[None], with_path=True)
    assert np.array_equal(both["f0"][0], got)          # the plan's three launches are the debug entry's
    for shift in (12, -12):
        assert np.array_equal(e.pitch(x, shift, FRAME16K), got * np.float32(Y.uppower(shift)))
    # a semitone transpose and a median of radius 1 on top: the reference's rows through tests/f0cond_ref.py
    try:
        e.set_pitch_semitones(3.0); e.set_f0_median(1)
        cond = e.pitch(x, 0, FRAME16K)
    finally:
        e.set_pitch_semitones(0.0); e.set_f0_median(0)
    want, _ = F.condition(r["f0"], F.multiplier(0, 3.0), r=1)
    sure = F.window_min((r["keep"] & r["pkeep"]).astype(np.float64), 1) > 0
    _check_rows(cond, want, sure, pm_case["bound"]["f"] + 2.0 ** -23, "transpose + median")
    assert np.array_equal(e.pitch(x, 0, FRAME16K), got)


def _inputs3():
    """three 16 kHz buffers of the chunk's length whose f0 windows are the three test inputs"""
    X = P.stream_signals()
    xs = np.stack([voice_signal(L, seed=s + 1) for s in range(3)])
    xs[:, -FR:] = X[:, -FR:]
    return xs


def test_streams_two_chunks(pm_case):
    z = zoo("tiny")
    sr = int(W.read_blob(z["model"])[0]["sr"])
    shifts = (12, 0, -12)
    second = _inputs3()
    first = np.stack([voice_signal(L, seed=10 + s) for s in range(3)])

    def run():
        e = _engine(z, streams=3)
        ys = [e.infer_batch(x, FRAME16K, shifts, g.skip_head, R) for x in (first, second)]
        caches = np.stack([e.pitch_cache(s) for s in range(3)])
        e.close()
        return ys, caches
    ys, caches = run()
    assert ys[0].shape == (3, R * sr // 100) and all(np.all(np.isfinite(y)) for y in ys)
    ys2, caches2 = run()
    assert all(np.array_equal(a, b) for a, b in zip(ys, ys2)) and np.array_equal(caches, caches2)          # bitwise repeatable
    for s in range(3):
        r = pm_case["refs"][s]
        lo = CACHE_START          # the rows the second chunk wrote, f0[3 : 31] (rvc.rs:168-179): its f0 window is test input s
        _check_rows(caches[s][lo:], (r["f0"] * Y.uppower(shifts[s]))[3:31], (r["keep"] & r["pkeep"])[3:31], pm_case["bound"]["f"], "stream %d of 3" % s)
        assert np.any(caches[s][lo - SHIFT:lo] > 0)          # (the first chunk's rows, moved down)


def test_two_chunks_eager_graph_pipeline():
    import torch
    z = zoo("tiny")
    sr = int(W.read_blob(z["model"])[0]["sr"])
    N = R * sr // 100
    x0, x1 = voice_signal(L, seed=3), _inputs3()[0]

    def run(mode):
        e = _engine(z)
        out = np.zeros((2, N), np.float32)
        if mode == "graph":
            e.set_use_graph(True)
        if mode == "pipeline":
            e.set_pipeline(True)
            d_in = torch.from_numpy(np.stack([x0, x1])).cuda()
            d_out = torch.zeros((2, N), device="cuda")
            torch.cuda.synchronize()
        for k, x in enumerate((x0, x1)):
            if mode == "pipeline":
                e.infer_device(d_in[k].data_ptr(), L, FRAME16K, 12, g.skip_head, R, d_out[k].data_ptr(), N, sync=False)
            else:
                out[k] = e.infer(x, FRAME16K, 12, g.skip_head, R)
        e.synchronize()
        if mode == "pipeline":
            out = d_out.cpu().numpy()
        cache = e.pitch_cache()
        e.close()
        return out, cache
    eager, cache = run("eager")
    again, cache2 = run("eager")
    assert np.all(np.isfinite(eager)) and np.any(cache > 0)
    assert np.array_equal(eager, again) and np.array_equal(cache, cache2)
    graph, gcache = run("graph")
    assert np.array_equal(graph, eager) and np.array_equal(gcache, cache)
    piped, pcache = run("pipeline")
    assert np.array_equal(pcache, cache) and np.array_equal(piped, eager)


def test_formant_shift_and_native_session(pm_case):
    from obs_rvc_amd.streaming import NativeStreamingSession
    z = zoo("tiny")
    sr = int(W.read_blob(z["model"])[0]["sr"])
    x = _inputs3()[0]
    r = pm_case["refs"][0]
    e = _engine(z)
    e.set_formant_shift(3.0)
    y = e.infer(x, FRAME16K, 12, g.skip_head, R)
    assert y.shape == (R * sr // 100,) and np.all(np.isfinite(y))
    # the cached f0 is the reference times uppower (exact) times (float)2^(-3/12): one more rounding of the product, 2^-24 relative
    want = r["f0"] * Y.uppower(12) * float(np.float32(2.0 ** (-3.0 / 12.0)))
    _check_rows(e.pitch_cache()[CACHE_START:], want[3:31], (r["keep"] & r["pkeep"])[3:31], pm_case["bound"]["f"] + 2.0 ** -24, "formant shift")
    e.close()
    e = _engine(z)
    s = NativeStreamingSession(e, 48000, 0.16, 0.07, 2.0, sr, 12, 0.6)
    assert s.sample_frame_16k == FRAME16K
    rng = np.random.default_rng(5)
    t = np.arange(2 * s.sample_frame_size) / 48000.0
    audio = (0.2 * sum(np.sin(2 * np.pi * 150.0 * k * t) / k for k in range(1, 5)) + 1e-3 * rng.standard_normal(len(t))).astype(np.float32)
    for k in range(2):
        out = s.process_one_frame(audio[k * s.sample_frame_size:(k + 1) * s.sample_frame_size])          # (raises unless RVC_OK)
        assert out.shape == (s.sample_frame_size,) and np.all(np.isfinite(out))
    assert np.any(e.pitch_cache() > 0)
    del s
    e.close()


def test_hybrid_member(pm_case):
    x = pm_case["X"][0]
    e = pm_case["engine"]
    pm = e.pitch(x, 0, FRAME16K)
    h = _engine(zoo("tiny"), "yin", full=False)
    yin = h.pitch(x, 0, FRAME16K)
    h.load_f0_hybrid(["pm"])
    assert h.f0_method == 8 and np.array_equal(h.pitch(x, 0, FRAME16K), pm)          # a hybrid of one member is that method, bit for bit
    for mode, mid in (("vote", H.VOTE), ("median", H.MEDIAN)):
        for members, rows in ((["pm", "yin"], [pm, yin]), (["yin", "pm"], [yin, pm])):
            h.load_f0_hybrid(members, mode)
            got = h.pitch(x, 0, FRAME16K)
            assert np.array_equal(got, H.combine(np.stack(rows), mid)), (mode, members)
    h.load_f0_method("hybrid[pm+yin]")
    assert h.f0_method == 8
    with pytest.raises(ValueError):
        h.load_f0_hybrid([9, 9])
    assert h._L.rvc_load_f0_hybrid(h._h, (C.c_int * 2)(9, 9), 2, 0) == 5 and h._L.rvc_load_f0_hybrid(h._h, (C.c_int * 2)(9, 6), 2, 0) == 5          # RVC_SHAPE
    assert h.f0_method == 8 and h._L.rvc_load_f0_hybrid(h._h, (C.c_int * 4)(9, 2, 1, 4), 1, 1) == 0
    h.load_f0_method("pm")
    assert np.array_equal(h.pitch(x, 0, FRAME16K), pm)
    h.close()
