"""Consonant protection (rvc_set_protect[_stream], csrc/protect.hip.h protect_mix_kernel) against the float64 restatement of
tests/protect_ref.py: the kernel alone through rvc_debug_protect, the stage inside a plan, neutrality, per-stream values, arguments.

Bound per element: 2^-21 (|p blend| + |(1 - p) raw|).  The recipe has two products, one sum and the float 1 - p, each rounded once at 2^-24 relative: at
most 4 * 2^-24 of the term magnitudes; the factor 2 on top covers the fma / no-fma difference.  A derivation, not a measurement.  Elements the definition
leaves alone (voiced rows, streams at 0.5, padding) are compared bit for bit; p = 0 gives the raw value.
The smallest geometry: 160 ms chunks, 21 rows per call, the tiny zoo, YIN unless stated.
Every comparison prints its figure before it asserts; DESIGN.md section 13 records what an MI355X run of this file gave (at most 0.33 of the bound)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import protect_ref as P
from common import BASELINE_160MS as g, rel_rms, rms, voice_signal, zoo
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc_common import RvcInferError

pytestmark = pytest.mark.gpu

FRAME16K, R, L, SKIP = g.sample_frame_16k, g.model_return_length, g.input_buffer_16k_size, g.skip_head
SEED = 1234
PCM_TOL = 1e-3       # one-stream against batched plans: the tolerance of tests/test_gpu_multi.py test_every_stream_has_its_own_pitch_shift (RMS of the PCM)
TAP_TOL = 1e-4       # and of a feature tap across plans: tests/test_gpu_parity.py, rel_rms of "cv.out" (relative RMS)
VALUES = (0.5, 0.0, 0.33)


class _Spec(C.Structure):
    """rvc_debug_protect_spec (include/rvc_mi355x_debug.h)"""
    _fields_ = [(n, C.c_int) for n in ("streams", "C", "R", "T", "skip_head", "ph_ld", "cv_ld", "graph")]


def _debug_protect(e, phone, cv, pitchf, values, R_, T, skip_head, graph=False):
    """phone [B][C][ph_ld], cv [B][C][cv_ld], pitchf [B][R] -> the mixed copy of phone"""
    fp = C.POINTER(C.c_float)
    fn = e._L.rvc_debug_protect
    fn.argtypes = [C.c_void_p, C.POINTER(_Spec), fp, fp, fp, C.POINTER(C.c_double)]
    fn.restype = C.c_int
    B, Cc, ph_ld = phone.shape
    out = np.ascontiguousarray(phone, np.float32).copy()
    cv, pitchf = np.ascontiguousarray(cv, np.float32), np.ascontiguousarray(pitchf, np.float32)
    assert cv.shape[:2] == (B, Cc) and pitchf.shape == (B, R_)
    s = _Spec(B, Cc, R_, T, skip_head, ph_ld, cv.shape[2], 1 if graph else 0)
    vals = (C.c_double * B)(*values)
    e._chk(fn(e._h, C.byref(s), out.ctypes.data_as(fp), cv.ctypes.data_as(fp), pitchf.ctypes.data_as(fp), vals))
    return out


def _check_mix(got, blend, cv, pitchf, p, skip_head, what):
    """got / blend [C][R] of one stream against protect_ref; -> the unvoiced mask"""
    ref, bound, uv = P.protect_mix(blend, cv, pitchf, p, skip_head)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(np.max(err[:, uv] / bound[:, uv])) if uv.any() and np.all(bound[:, uv] > 0) else 0.0
    print("%s: p %.2f, %d of %d rows unvoiced, largest error %.3e, largest error / bound %.3f" % (what, p, uv.sum(), len(uv), float(err.max()), worst))
    assert np.all(err <= bound), (what, float(np.max(err - bound)))
    assert np.array_equal(got[:, ~uv], blend[:, ~uv])                  # rows the definition leaves alone: their bits
    if float(np.float32(p)) == 0.0 and uv.any():
        assert np.array_equal(got[:, uv], P.raw_rows(cv, skip_head, blend.shape[1])[:, uv])
    return uv


@pytest.fixture(scope="module")
def bare():
    from obs_rvc_amd.rvc import RvcInfer
    e = RvcInfer(zoo("tiny")["data"])
    yield e
    e.close()


# ---- 1. the kernel alone ----
@pytest.mark.parametrize("Cc", [48, 256])
@pytest.mark.parametrize("R_", [1, 21, 200])
@pytest.mark.parametrize("B", [1, 3])
def test_kernel_alone(bare, Cc, R_, B):
    rng = np.random.default_rng(1000 * Cc + 10 * R_ + B)
    T = R_ // 2 + 10
    ph_ld, cv_ld = R_ + 3, T + 5                                        # leading dimensions larger than R and T
    reach = 2 * T + 1 - R_                                              # skip_head + R = 2 T + 1: the call's last row is row 2 T, the repeated last column
    patterns = {"voiced": np.full(R_, 220.0), "unvoiced": np.zeros(R_), "alternating": np.array([0.0, 1.0, 0.5, 220.0])[np.arange(R_) % 4]}
    value_sets = [VALUES] if B == 3 else [(0.33,), (0.0,), (0.5,)]
    seen_parity = set()
    for skip_head in (reach, reach - 1):
        seen_parity.add(skip_head % 2)
        for values in value_sets:
            for name in patterns:
                phone = rng.standard_normal((B, Cc, ph_ld)).astype(np.float32)
                cv = rng.standard_normal((B, Cc, cv_ld)).astype(np.float32)
                pitchf = np.stack([np.roll(patterns[name], b) for b in range(B)]).astype(np.float32)
                got = _debug_protect(bare, phone, cv, pitchf, values, R_, T, skip_head, graph=(name == "alternating" and skip_head == reach))
                assert np.array_equal(got[:, :, R_:], phone[:, :, R_:])   # the padding behind the rows
                for b in range(B):
                    uv = _check_mix(got[b, :, :R_], phone[b, :, :R_], cv[b, :, :T], pitchf[b], values[b], skip_head,
                                    "C %d R %d B %d skip %d %s stream %d" % (Cc, R_, B, skip_head, name, b))
                    on = float(np.float32(values[b])) < 0.5
                    assert uv.sum() == (int(np.sum(pitchf[b] < 1)) if on else 0)
                    if not on:
                        assert np.array_equal(got[b], phone[b])
                    elif uv.any() and values[b] > 0:
                        assert not np.array_equal(got[b, :, :R_][:, uv], phone[b, :, :R_][:, uv])
    assert seen_parity == {0, 1}


@pytest.mark.parametrize("ph_ld,cv_ld", [(352, 224), (353, 224)], ids=["plan_ld", "odd_ld"])
def test_kernel_at_the_default_converter_window(bare, ph_ld, cv_ld):
    """the file converter's default window (k = 14): 3 streams, 768 channels, T = 223 ContentVec frames, skip_head 48, 351 rows -- the last one is row
    48 + 350 = 398, ContentVec frame 199.  Leading dimensions padded to 4 floats as the plan pads them, and an odd one.  Every stream has an unvoiced
    run that starts at row 0 and one that ends at row 350; values 0 (the raw rows, bit for bit), 0.33 and 0.5 (off)"""
    B, Cc, T, skip_head, R_ = 3, 768, 223, 48, 351
    values = (0.0, 0.33, 0.5)
    rng = np.random.default_rng(351 + ph_ld)
    phone = rng.standard_normal((B, Cc, ph_ld)).astype(np.float32)
    cv = rng.standard_normal((B, Cc, cv_ld)).astype(np.float32)
    pitchf = np.full((B, R_), 220.0, np.float32)
    for b in range(B):
        pitchf[b, :7 + b] = 0.0                                          # from row 0
        pitchf[b, R_ - 5 - 64 * b:] = 0.0                                # to row 350 (stream 2: across the 256th row)
        pitchf[b, 100 + b:300:37] = 0.5                                  # single unvoiced rows in between
    for graph in (False, True):
        got = _debug_protect(bare, phone, cv, pitchf, values, R_, T, skip_head, graph=graph)
        assert np.array_equal(got[:, :, R_:], phone[:, :, R_:])
        for b in range(B):
            uv = _check_mix(got[b, :, :R_], phone[b, :, :R_], cv[b, :, :T], pitchf[b], values[b], skip_head, "k = 14 window, ph_ld %d stream %d" % (ph_ld, b))
            on = float(np.float32(values[b])) < 0.5
            assert uv.sum() == (int(np.sum(pitchf[b] < 1)) if on else 0) and (not on or (uv[0] and uv[R_ - 1]))
            if not on:
                assert np.array_equal(got[b], phone[b])
    assert np.array_equal(P.raw_rows(cv[0, :, :T], skip_head, R_)[:, R_ - 1], cv[0, :, (skip_head + R_ - 1) // 2])     # row 350 reads frame 199
    assert (skip_head + R_ - 1) // 2 == 199


def test_debug_hook_rejects_bad_shapes(bare):
    ph, cv, pf = np.zeros((1, 4, 8), np.float32), np.zeros((1, 4, 4), np.float32), np.zeros((1, 8), np.float32)
    for kw in (dict(R_=8, T=4, skip_head=2), dict(R_=8, T=5, skip_head=0)):       # skip_head + R > 2 T + 1; cv_ld < T
        with pytest.raises(RvcInferError):
            _debug_protect(bare, ph, cv, pf, (0.2,), **kw)
    with pytest.raises(RvcInferError):
        _debug_protect(bare, ph, cv, pf, (0.6,), R_=8, T=4, skip_head=0)


# ---- engines ----
def _index(seed=5):
    return W.make_index(3000, 48, seed=seed)


def _engine(method="yin", streams=1, index=True, stream_id=0, taps=False):
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("tiny")
    e = RvcInfer(z["data"])
    e.load_contentvec(2); e.load_model(z["model"]); e.load_f0_method(method)
    if streams > 1:
        e.set_streams(streams)
    e.set_noise_seed(SEED, stream_id)
    if index:
        e.load_index(_index()); e.set_index_rate(0.75)
    if taps:
        e.enable_taps(True)
    return e


def _half_voiced(stream=0, chunk=0):
    """a sine in front, zeros behind: the call's 21 pitchf rows are the f0 rows 8 .. 28 of the last 4960 samples, so the cut sits in their middle"""
    t = np.arange(L) / 16000.0
    x = (0.3 * np.sin(2 * np.pi * (220.0 + 15.0 * stream + 7.0 * chunk) * t)).astype(np.float32)
    x[L - 2200 - 160 * (stream % 2):] = 0.0
    return x


def _both_kinds(pitchf):
    v = int(np.sum(~P.unvoiced(pitchf)))
    print("pitchf rows: %d voiced, %d unvoiced" % (v, len(pitchf) - v))
    assert len(pitchf) == R and 4 * v >= R and 4 * (R - v) >= R, pitchf


# ---- 2. in the plan ----
def test_in_the_plan():
    x = _half_voiced()
    a = _engine(taps=True)
    ya = a.infer(x, FRAME16K, 12, SKIP, R)
    pitchf = a.tap("pitchf")
    _both_kinds(pitchf)
    Cc = a.tap("phone_ct").size // R
    blend, cv = a.tap("phone_ct").reshape(Cc, R), a.tap("cv.out").reshape(Cc, -1)
    hits_a = a.knn()
    with pytest.raises(RvcInferError):
        a.tap("phone_prot")                                             # no protection, no stage
    a.close()
    b = _engine(taps=True)
    b.set_protect(0.33)
    yb = b.infer(x, FRAME16K, 12, SKIP, R)
    assert np.array_equal(b.tap("phone_ct"), blend.reshape(-1)) and np.array_equal(b.tap("pitchf"), pitchf) and np.array_equal(b.tap("cv.out"), cv.reshape(-1))
    uv = _check_mix(b.tap("phone_prot").reshape(Cc, R), blend, cv, pitchf, 0.33, SKIP, "plan")
    assert not np.array_equal(b.tap("phone_prot").reshape(Cc, R)[:, uv], blend[:, uv])
    hits_b = b.knn()
    assert len(hits_a[0]) == R and np.array_equal(hits_a[0], hits_b[0]) and np.array_equal(hits_a[1], hits_b[1])
    assert ya.shape == yb.shape and np.all(np.isfinite(yb)) and not np.array_equal(ya, yb)
    b.close()


# ---- 3. neutrality ----
def _two_chunks(e, streams, method):
    ys = []
    for k in range(2):
        # (RMVPE's seeded tiny network gets the suite's usual voice signal: what it calls voiced is not the point here)
        xs = np.stack([_half_voiced(s, k) if method == "yin" else voice_signal(L, seed=10 * k + s + 1) for s in range(streams)])
        ys.append(e.infer_batch(xs, FRAME16K, [12, 0, -12][:streams], SKIP, R) if streams > 1 else e.infer(xs[0], FRAME16K, 12, SKIP, R))
    return ys, [e.pitch_cache(s) for s in range(streams)], e.knn(), e.plan_cache_info()["builds"]


@pytest.mark.parametrize("method", ["yin", "rmvpe"])
@pytest.mark.parametrize("streams", [1, 3])
def test_off_and_no_index_change_nothing(method, streams):
    for index, value in ((True, 0.5), (False, 0.33)):
        res = []
        for touched in (False, True):
            e = _engine(method, streams, index=index)
            if touched:
                e.set_protect(value)
                e.set_protect(value, stream=streams - 1)
            res.append(_two_chunks(e, streams, method))
            e.close()
        (ya, ca, ha, ba), (yb, cb, hb, bb) = res
        assert all(np.array_equal(p, q) and np.all(np.isfinite(p)) for p, q in zip(ya, yb))
        assert all(np.array_equal(p, q) for p, q in zip(ca, cb)) and (method != "yin" or np.any(ca[0] > 0))
        assert np.array_equal(ha[0], hb[0]) and np.array_equal(ha[1], hb[1]) and len(ha[0]) == (R * streams if index else 0)
        assert ba == bb, (index, value, ba, bb)                         # 0.5, and any value without an index: no additional plan


def test_changing_the_value_builds_no_plan():
    e, ref = _engine(), _engine()
    e.set_protect(0.33); ref.set_protect(0.2)
    x0, x1 = _half_voiced(0, 0), _half_voiced(0, 1)
    e.infer(x0, FRAME16K, 12, SKIP, R); ref.infer(x0, FRAME16K, 12, SKIP, R)
    builds = e.plan_cache_info()["builds"]
    y33 = e.infer(x1, FRAME16K, 12, SKIP, R)
    e.reset_state(); e.set_noise_seed(SEED, 0)
    e.infer(x0, FRAME16K, 12, SKIP, R)
    e.set_protect(0.2)
    y20 = e.infer(x1, FRAME16K, 12, SKIP, R)
    assert e.plan_cache_info()["builds"] == builds
    # the value did arrive: chunk 2 at 0.2 differs from chunk 2 at 0.33 and is what an engine at 0.2 from the start gives (chunk 1 does not reach chunk 2
    # through the features, only through the pitch cache, which protection never writes)
    assert not np.array_equal(y20, y33) and np.array_equal(y20, ref.infer(x1, FRAME16K, 12, SKIP, R))
    e.close(); ref.close()


# ---- 4. per stream ----
def _close(a, b, tol, what, rel=False):
    d = rel_rms(a, b) if rel else rms(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    print("%s: %s %.3e (tolerance %.1e), bit-identical: %s" % (what, "relative rms" if rel else "rms", d, tol, np.array_equal(a, b)))
    assert d < tol, (what, d)


def test_per_stream_values():
    xs = np.stack([_half_voiced(s) for s in range(3)])
    shifts = [12, 12, 12]

    def batch(values, taps=True, graph=False):
        e = _engine(streams=3, taps=taps)
        for s, v in enumerate(values):
            if v is not None:
                e.set_protect(v, stream=s)
        if graph:
            e.set_use_graph(True)
        return e
    e = batch(VALUES)
    y = e.infer_batch(xs, FRAME16K, shifts, SKIP, R)
    prot, pitchf = e.tap("phone_prot"), e.tap("pitchf").reshape(3, R)
    Cc = prot.size // (3 * R)
    prot = prot.reshape(3, Cc, R)
    # the batch against the definition on its OWN tensors, every stream, at the element-wise bound: phone_blend / cv.out_all are what the stage read,
    # for every stream of the plan (phone_ct and cv.out are stream 0's only)
    blend_all, cv_all = e.tap("phone_blend").reshape(3, Cc, R), e.tap("cv.out_all").reshape(3, Cc, -1)
    assert np.array_equal(blend_all[0], e.tap("phone_ct").reshape(Cc, R)) and np.array_equal(cv_all[0], e.tap("cv.out").reshape(Cc, -1))
    for s, v in enumerate(VALUES):
        _both_kinds(pitchf[s])
        uv = _check_mix(prot[s], blend_all[s], cv_all[s], pitchf[s], v, SKIP, "batch of 3, stream %d" % s)
        assert uv.sum() == (int(np.sum(P.unvoiced(pitchf[s]))) if v < 0.5 else 0)
        if v == 0.5:
            assert np.array_equal(prot[s], blend_all[s])
    hits = e.knn()
    e.close()
    # (the same tap level: a tapped plan keeps the explicit layers, the untapped one folds them, and the two agree only to rounding)
    plain = batch((None, None, None))
    yp = plain.infer_batch(xs, FRAME16K, shifts, SKIP, R)
    plain.close()
    assert np.array_equal(y[0], yp[0]) and not np.array_equal(y[1], yp[1]) and not np.array_equal(y[2], yp[2])      # the stream at 0.5: the unprotected batch's PCM
    # three one-stream engines with the same seed and stream id.  A one-stream plan and a three-stream plan run different kernels (tile choices, the one-stream
    # synthesizer), so they agree to the tolerances of the existing parity tests (PCM_TOL, TAP_TOL above), not bit for bit; what IS exact is checked exactly:
    # the voicing, the hits, and the definition applied to the one-stream engine's own tensors
    for s, v in enumerate(VALUES):
        o = _engine(stream_id=s, taps=True)
        if v < 0.5:
            o.set_protect(v)
        yo = o.infer(xs[s], FRAME16K, 12, SKIP, R)
        pf, blend, cv = o.tap("pitchf"), o.tap("phone_ct").reshape(Cc, R), o.tap("cv.out").reshape(Cc, -1)
        _both_kinds(pf)
        assert np.array_equal(P.unvoiced(pf), P.unvoiced(pitchf[s]))
        ho = o.knn()
        assert np.array_equal(ho[0], hits[0][s * R:(s + 1) * R])
        one = o.tap("phone_prot").reshape(Cc, R) if v < 0.5 else blend
        if v < 0.5:
            _check_mix(one, blend, cv, pf, v, SKIP, "one-stream engine %d" % s)
        _close(prot[s], one, TAP_TOL, "stream %d phone_prot, batch of 3 against one stream" % s, rel=True)
        _close(y[s], yo, PCM_TOL, "stream %d PCM, batch of 3 against one stream" % s)
        if s == 0:
            assert np.array_equal(y[0], yo)                                 # the stream at 0.5: the unprotected one-stream engine's PCM, bit for bit
        uv = P.unvoiced(pf)
        if v == 0.0:
            # p = 0 in the batch: the unvoiced rows are the batch's raw rows; against the one-stream engine's raw rows to the tap tolerance
            _close(prot[s][:, uv], P.raw_rows(cv, SKIP, R)[:, uv], TAP_TOL, "stream %d unvoiced rows against raw" % s, rel=True)
        o.close()
    # from here on the production plan (no taps): the eager run, and the same stream-0 check against the unprotected batch
    e1 = batch(VALUES, taps=False)
    y1 = e1.infer_batch(xs, FRAME16K, shifts, SKIP, R)
    e1.close()
    p1 = batch((None, None, None), taps=False)
    yp1 = p1.infer_batch(xs, FRAME16K, shifts, SKIP, R)
    p1.close()
    assert np.array_equal(y1[0], yp1[0]) and not np.array_equal(y1[1], yp1[1]) and not np.array_equal(y1[2], yp1[2])
    _close(y1, y, PCM_TOL, "production plan against the tapped plan")
    # graph replay: the same plan, the same bits
    eg = batch(VALUES, taps=False, graph=True)
    yg = [eg.infer_batch(xs, FRAME16K, shifts, SKIP, R) for _ in range(2)][0]
    eg.close()
    assert np.array_equal(yg, y1)
    y = y1
    # rvc_infer_batch_g, two geometries: streams 0 and 2 keep the geometry above, stream 1 (p = 0) runs two rows later and shorter.  Buckets are plans of 2 and
    # of 1 stream: against the eager single-geometry runs to PCM_TOL, and against what the same call gives without protection
    geo_sh, geo_R = [SKIP, SKIP + 2, SKIP], [R, R - 2, R]
    eb = batch(VALUES, taps=False)
    yb = eb.infer_batch_g(list(xs), [FRAME16K] * 3, shifts, geo_sh, geo_R)
    eb.close()
    pb = batch((None, None, None), taps=False)
    ypb = pb.infer_batch_g(list(xs), [FRAME16K] * 3, shifts, geo_sh, geo_R)
    pb.close()
    e2 = batch(VALUES, taps=False)
    y2 = e2.infer_batch(xs, FRAME16K, shifts, SKIP + 2, R - 2)
    e2.close()
    assert np.array_equal(yb[0], ypb[0]) and not np.array_equal(yb[1], ypb[1]) and not np.array_equal(yb[2], ypb[2])
    _close(yb[0], y[0], PCM_TOL, "batch_g stream 0 against the eager run")
    _close(yb[2], y[2], PCM_TOL, "batch_g stream 2 against the eager run")
    _close(yb[1], y2[1], PCM_TOL, "batch_g stream 1 against the eager run of its geometry")
    # the protected streams are nearer to their protected eager runs than to the unprotected call: the bucket did get the stream's own value
    assert rms(yb[2] - y[2]) < rms(yb[2] - ypb[2]) and rms(yb[1] - y2[1]) < rms(yb[1] - ypb[1])


# ---- 5. arguments ----
def test_arguments():
    e = _engine(streams=2)
    for f in (lambda: e.set_protect(float("nan")), lambda: e.set_protect(-0.1), lambda: e.set_protect(0.6), lambda: e.set_protect(0.2, stream=2),
              lambda: e.set_protect(0.2, stream=-1), lambda: e.set_protect(float("nan"), stream=0), lambda: e.set_protect(0.6, stream=1)):
        with pytest.raises(RvcInferError) as ei:
            f()
        assert ei.value.kind == "NdarrayShapeError" and str(ei.value) != "NdarrayShapeError"        # RVC_SHAPE, with a message
    e.set_protect(0.5); e.set_protect(0.0)
    # a stream added after the engine-wide call inherits the value; rvc_reset_state leaves it alone
    e.set_protect(0.25)
    e.set_streams(3)
    e.set_noise_seed(SEED, 0)
    e.load_index(_index()); e.set_index_rate(0.75)
    e.reset_state()
    e.enable_taps(True)
    xs = np.stack([_half_voiced(s) for s in range(3)])
    e.infer_batch(xs, FRAME16K, 12, SKIP, R)
    prot = e.tap("phone_prot")
    Cc = prot.size // (3 * R)
    prot, pitchf = prot.reshape(3, Cc, R), e.tap("pitchf").reshape(3, R)
    e.close()
    o = _engine(stream_id=2, taps=True)
    o.set_protect(0.25)
    o.infer(xs[2], FRAME16K, 12, SKIP, R)
    one, pf = o.tap("phone_prot").reshape(Cc, R), o.tap("pitchf")
    blend = o.tap("phone_ct").reshape(Cc, R)
    o.close()
    uv = P.unvoiced(pf)
    assert np.array_equal(uv, P.unvoiced(pitchf[2])) and uv.any()
    _close(prot[2], one, TAP_TOL, "the added stream against a one-stream engine at 0.25", rel=True)
    # and it is protected: its unvoiced rows are nearer to the protected one-stream rows than to the blended ones
    assert rms(prot[2][:, uv] - one[:, uv]) < 0.1 * rms(prot[2][:, uv] - blend[:, uv])
