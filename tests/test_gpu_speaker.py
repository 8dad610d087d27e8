"""Run-time speaker selection on the GPU: seeded `tiny` models with a speaker table (make_synth n_spk = 3 / 9).

  1. the fold against float64 (tests/speaker_ref.py) through the read-only aid rvc_debug_speaker_biases: one speaker, a 2-way and an 8-way mix; per element
     |gpu - ref| <= (gin + 8) 2^-24 (|base_b| + |cond_b| + sum_q |cond_w g|), from the length of the sums; the plain and the composed copy identical bits
  2. end to end: engine A selects on the table, engine B loads a blob baked for that speaker (sy.g = the row, or the float64 mix rounded to f32); both against
     the CPU oracle on B's blob and against each other at the tiny end-to-end tolerance of tests/test_gpu_parity.py (PCM_TOL), at 1, 3 and 9 streams (9: the
     plain WaveNets) and on a model without pitch guidance (there the reference is the float64 chain of tests/nof0_ref.py, as in tests/test_gpu_nof0.py)
  3. a change between chunks: eager, graph replay, pipelined unsynchronised calls; bitwise repeatable, no plan built
  4. a compose_flows that comes after the set call does not reinstate the baked speaker
  5. errors leave the state alone; a blob without a table; reload

None of it runs on the parent commit: the symbols do not exist."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import debug_abi as D
import nof0_ref as NR
import speaker_ref as SP
import synth_ref as SR
import test_gpu_stream_taps as T
from common import BASELINE_160MS as g, rms, set_opt, voice_signal, zoo
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc_common import RvcInferError
from test_gpu_parity import PCM_TOL

pytestmark = pytest.mark.gpu
FRAME, SKIP, R = g.sample_frame_16k, g.skip_head, g.model_return_length
SEED = 1234
MIX3 = {0: 0.3, 2: 0.7}


@functools.lru_cache(maxsize=None)
def _table_model(n_spk, f0=True):
    """(zoo, model path, cfg, tensors) of the seeded tiny model with an n_spk-row table"""
    z = W.build_model_zoo(W.default_zoo_root("tiny"), "tiny", 2, None, n_spk=n_spk)
    if f0:
        return (z, z["model"]) + W.read_blob(z["model"])
    path = os.path.join(os.path.dirname(z["model"]), "model-tiny-nof0-v2-spk%d.rvcw" % n_spk)
    cfg, tens = W.make_synth("tiny", 48, f0=False, n_spk=n_spk)
    if not os.path.exists(path):
        W.write_blob(path, cfg, tens)
    return z, path, cfg, tens


def _g_of(tens, mix):
    ids, w = SP.normalise_mix(mix, tens["sy.emb_g"].shape[0])
    return SP.mix_g(tens["sy.emb_g"], ids, w)


def _baked(tmp_path, cfg, tens, mix, tag):
    """the blob written for that speaker: sy.g = the row itself (one id) or the float64 mix rounded to f32; no table"""
    ids, w = SP.normalise_mix(mix, tens["sy.emb_g"].shape[0])
    gq = tens["sy.emb_g"][ids[0]] if len(ids) == 1 else SP.mix_g(tens["sy.emb_g"], ids, w)
    cb, tb = SP.baked(cfg, tens, gq)
    p = str(tmp_path / ("baked-%s.rvcw" % tag))
    W.write_blob(p, cb, tb)
    return p, cb, tb


def _engine(z, model, S=1, f0=True, seed=SEED, id0=0):
    from obs_rvc_amd.rvc import RvcInfer
    e = RvcInfer(z["data"]); e.load_contentvec(2)
    if f0:
        e.load_f0()
    e.load_model(model)
    if S > 1:
        e.set_streams(S)
    e.set_noise_seed(seed, id0)
    return e


def _biases(e, composed):
    L = D.lib()
    n = C.c_size_t()
    out = np.empty(1 << 16, np.float32)
    rc = L.rvc_debug_speaker_biases(e._h, int(composed), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(n))
    assert rc == 0, (rc, composed)
    return out[: n.value].copy()


def _check_fold(e, cfg, tens, mix, what, composed=True):
    ref, mag = SP.fold(cfg, tens, _g_of(tens, mix))
    bound = SP.fold_bound(cfg, mag)
    plain = _biases(e, 0)
    err = np.abs(plain.astype(np.float64) - ref)
    print("speaker fold %s: %d rows, max |gpu - ref64| / bound %.3f (max err %.2e, max bound %.2e)" % (what, ref.size, float(np.max(err / bound)), err.max(), bound.max()))
    assert plain.shape == ref.shape and np.all(err <= bound), (what, int(np.argmax(err / bound)), float(np.max(err / bound)))
    if composed:
        assert D.same_bits(_biases(e, 1), plain), what


# ---- 1. the fold against float64 ---------------------------------------------------------------------------------------------------------------------
def test_fold_against_float64_and_both_copies_identical():
    z, model, cfg, tens = _table_model(9)
    e = _engine(z, model)
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    assert e.speakers() == 9 and e.speaker_mix() == {0: 1.0}
    _check_fold(e, cfg, tens, {0: 1.0}, "as loaded (the host fold)")
    L = D.lib()
    assert L.rvc_debug_speaker_fold_ms(e._h) == -1.0
    e.set_profile(True)
    for what, mix in (("one speaker", {4: 1.0}), ("2-way mix", {1: 0.25, 7: 0.75}), ("8-way mix", {i: float(i) for i in range(1, 9)}),
                      ("speaker 0 by a set call", {0: 1.0})):
        if len(mix) == 1:
            e.set_speaker(next(iter(mix)))
        else:
            e.set_speaker_mix(mix)
        ids, w = SP.normalise_mix(mix, 9)
        got = e.speaker_mix()
        assert list(got) == ids and list(got.values()) == w.tolist(), what
        assert np.all(np.isfinite(e.infer(x, FRAME, 12, SKIP, R)))           # (the chunk queues the fold)
        _check_fold(e, cfg, tens, mix, what)
    ms = L.rvc_debug_speaker_fold_ms(e._h)
    print("speaker fold launch on tiny (%d rows x %d): %.4f ms" % (SP.fold(cfg, tens, tens["sy.g"])[0].size, int(cfg["gin"]), ms))
    assert 0.0 < ms < 50.0
    e.close()


# ---- 2. end to end against a baked blob --------------------------------------------------------------------------------------------------------------
def _oracle_pcm(z, model, xin, S):
    from oracle import oracle as O
    out = []
    for s in range(S):
        o = O.OracleRvcInfer(z["data"]); o.load_contentvec(2); o.load_f0(1); o.load_model(model); o.set_noise_seed(SEED, s)
        out.append(o.infer(xin[s], FRAME, 12, SKIP, R))
        o.close()
    return np.stack(out)


@pytest.mark.parametrize("S", [1, 3, 9])
def test_end_to_end_against_a_baked_blob(S, tmp_path):
    z, model, cfg, tens = _table_model(3)
    xin = np.stack([voice_signal(g.input_buffer_16k_size, seed=30 + s) for s in range(S)])
    a = _engine(z, model, S)
    assert a.speakers() == 3
    y_loaded = a.infer_batch(xin, FRAME, 12, SKIP, R)
    for tag, mix in (("row2", {2: 1.0}), ("mix", MIX3)):
        if len(mix) == 1:
            a.set_speaker(2)
        else:
            a.set_speaker_mix(mix)
        a.reset_state()
        ya = a.infer_batch(xin, FRAME, 12, SKIP, R)
        pb, cb, tb = _baked(tmp_path, cfg, tens, mix, tag)
        b = _engine(z, pb, S)
        assert b.speakers() == 1
        yb = b.infer_batch(xin, FRAME, 12, SKIP, R)
        b.close()
        yo = _oracle_pcm(z, pb, xin, S)
        for s in range(S):
            ea, eb, eab = rms(ya[s] - yo[s]), rms(yb[s] - yo[s]), rms(ya[s] - yb[s])
            print("speaker %s S=%d stream %d: A-oracle %.2e, B-oracle %.2e, A-B %.2e (bound %.0e); loaded-A %.2e" % (tag, S, s, ea, eb, eab, PCM_TOL, rms(ya[s] - y_loaded[s])))
            assert ya[s].shape == yo[s].shape and ea < PCM_TOL and eb < PCM_TOL and eab < PCM_TOL, (tag, s, ea, eb, eab)
            assert rms(ya[s] - y_loaded[s]) > PCM_TOL, (tag, s)            # the speaker is audible: the check above is no tautology
        _check_fold(a, cfg, tens, mix, "%s S=%d" % (tag, S))
    a.close()


def test_end_to_end_without_pitch_guidance(tmp_path):
    from oracle import oracle as O
    z, model, cfg, tens = _table_model(3, f0=False)
    xs = T._inputs(1)
    o = O.OracleRvcInfer(z["data"]); o.load_contentvec(2)
    cv = np.asarray(o.hubert(xs[1][0]), np.float32)
    o.close()
    cv = cv.reshape(cv.shape[-2], cv.shape[-1])
    I = int(cfg["inter"])
    eps = O.philox_normal(T.SEED, T.ID0, 1, 0, I * R).reshape(I, R)              # the second chunk's normals

    def two_chunks(e):
        e.reset_state()
        for c in range(2):
            y = e.infer(xs[c][0], FRAME, None, SKIP, R)
        return y
    a = _engine(z, model, f0=False, seed=T.SEED, id0=T.ID0)
    assert a.speakers() == 3 and a.model_has_f0() is False
    for tag, mix in (("row2", {2: 1.0}), ("mix", MIX3)):
        if len(mix) == 1:
            a.set_speaker(2)
        else:
            a.set_speaker_mix(mix)
        ya = two_chunks(a)
        pb, cb, tb = _baked(tmp_path, cfg, tens, mix, "nof0-" + tag)
        b = _engine(z, pb, f0=False, seed=T.SEED, id0=T.ID0)
        yb = two_chunks(b)
        b.close()
        ref = NR.synth(cb, tb, SR.phone_gather(cv, SKIP, R), eps)["pcm"]
        ea, eb, eab = rms(ya - ref), rms(yb - ref), rms(ya - yb)
        print("speaker %s no-f0: A-ref64 %.2e, B-ref64 %.2e, A-B %.2e (bound %.0e)" % (tag, ea, eb, eab, PCM_TOL))
        assert ya.shape == ref.shape and ea < PCM_TOL and eb < PCM_TOL and eab < PCM_TOL, (tag, ea, eb, eab)
    a.close()


# ---- 3. a change between chunks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph", "pipeline"])
def test_change_between_chunks(mode):
    import torch
    z, model, cfg, tens = _table_model(3)
    L_, N = g.input_buffer_16k_size, R * int(cfg["sr"]) // 100
    x = voice_signal(L_, seed=3)
    e = _engine(z, model)
    if mode == "graph":
        e.set_use_graph(True)
    if mode == "pipeline":
        e.set_pipeline(True)
        d_in = torch.from_numpy(x).cuda()
        d_out = torch.zeros((N,), device="cuda")
        torch.cuda.synchronize()

    def chunk():
        e.reset_state()                      # the same chunk counter (the prior's and the source's noise) and pitch cache every time
        if mode == "pipeline":
            assert e.infer_device(d_in.data_ptr(), L_, FRAME, 12, SKIP, R, d_out.data_ptr(), N, sync=False) == N
            e.synchronize()
            return d_out.cpu().numpy().copy()
        return e.infer(x, FRAME, 12, SKIP, R)
    chunk(); chunk()                         # (pipelined calls alternate between two plan slots: both are built here)
    builds = e.plan_cache_info()["builds"]
    y0 = chunk()
    e.set_speaker(1)
    y1 = chunk()
    e.set_speaker(0); e.set_speaker(1)
    y2 = chunk()
    e.set_speaker(0)
    y3 = chunk()
    assert y0.shape == (N,) and np.all(np.isfinite(y1))
    assert D.same_bits(y1, y2), mode
    assert not np.array_equal(y0, y1) and rms(y0 - y1) > PCM_TOL, mode
    assert rms(y3 - y0) < PCM_TOL            # speaker 0 folded on the device against the loader's host fold of it: the same speaker, another summation order
    assert e.plan_cache_info()["builds"] == builds, mode
    _check_fold(e, cfg, tens, {0: 1.0}, mode)
    e.close()


def test_unsynchronised_pipelined_calls_see_the_set_calls_in_order():
    import torch
    z, model, cfg, tens = _table_model(3)
    L_, N = g.input_buffer_16k_size, R * int(cfg["sr"]) // 100
    xs = np.stack([voice_signal(L_, seed=40 + i) for i in range(4)])
    steps = [None, {1: 1.0}, {2: 1.0}, {0: 0.5, 1: 0.5}]

    def run(pipelined):
        e = _engine(z, model)
        e.set_pipeline(pipelined)
        d_in = torch.from_numpy(xs).cuda()
        d_out = torch.zeros((4, N), device="cuda")
        torch.cuda.synchronize()
        for i, mix in enumerate(steps):
            if mix is not None:
                e.set_speaker_mix(mix)
            e.infer_device(d_in[i].data_ptr(), L_, FRAME, 12, SKIP, R, d_out[i].data_ptr(), N, sync=not pipelined)
        e.synchronize()
        y = d_out.cpu().numpy().copy()
        e.close()
        return y
    ys, yp = run(False), run(True)
    assert np.all(np.isfinite(ys)) and D.same_bits(ys, yp)


# ---- 4. a late compose -------------------------------------------------------------------------------------------------------------------------------
def test_a_late_compose_does_not_reinstate_the_baked_speaker(tmp_path):
    z, model, cfg, tens = _table_model(3)
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    pb, cb, tb = _baked(tmp_path, cfg, tens, {2: 1.0}, "late")
    b = _engine(z, pb)
    yb = b.infer(x, FRAME, 12, SKIP, R)
    b.close()
    set_opt("RVC_NO_WN_COMPOSE", "1")
    try:
        a = _engine(z, model)                # loaded with the hook on: the flows are not composed
        L = D.lib()
        n = C.c_size_t()
        assert L.rvc_debug_speaker_biases(a._h, 1, None, 0, C.byref(n)) == D.RVC_SHAPE
        a.set_speaker(2)
        y_plain = a.infer(x, FRAME, 12, SKIP, R)      # a plain plan first: the fold has run, on the plain copies alone
        ops_plain = a.plan_ops()
    finally:
        set_opt("RVC_NO_WN_COMPOSE", None)
    a.reset_state()
    ya = a.infer(x, FRAME, 12, SKIP, R)               # one stream: build_synth composes now, from the host copies of speaker 0
    assert a.plan_ops() < ops_plain                    # (the composed plan has fewer launches)
    print("late compose: A-B %.2e, plain-composed %.2e (bound %.0e)" % (rms(ya - yb), rms(ya - y_plain), PCM_TOL))
    assert rms(ya - yb) < PCM_TOL and rms(y_plain - yb) < PCM_TOL
    _check_fold(a, cfg, tens, {2: 1.0}, "late compose")
    a.close()


# ---- 5. errors and defaults --------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_mix_and_defaults():
    from obs_rvc_amd.rvc import RvcInfer
    L = D.lib()
    z, model, cfg, tens = _table_model(3)
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    e = RvcInfer(z["data"]); e.load_contentvec(2); e.load_f0()
    assert e.speakers() == 0 and L.rvc_model_speakers(None) == 0
    with pytest.raises(RvcInferError) as err:
        e.set_speaker(0)
    assert err.value.code == 1                         # RVC_MODEL_NOT_LOADED
    with pytest.raises(RvcInferError):
        e.speaker_mix()
    e.load_model(model); e.set_noise_seed(SEED, 0)
    e.set_speaker_mix({2: 3.0, 1: 1.0})
    want = {2: 0.75, 1: 0.25}
    assert e.speaker_mix() == want
    i32, f64 = C.c_int32, C.c_double

    def raw(ids, ws, n=None):
        a, w = (i32 * max(len(ids), 1))(*ids), (f64 * max(len(ws), 1))(*ws)
        return L.rvc_set_speaker_mix(e._h, a, w, len(ids) if n is None else n)
    for ids, ws in (([3], [1.0]), ([-1], [1.0]), ([], []), (list(range(9)), [1.0] * 9), ([0, 0], [0.5, 0.5]), ([0, 1], [1.0, -0.1]), ([0], [float("nan")]),
                    ([0], [float("inf")]), ([0, 1], [0.0, 0.0])):
        assert raw(ids, ws) == D.RVC_SHAPE and e.speaker_mix() == want, (ids, ws)
        assert len(L.rvc_last_error_message(e._h)) > 0
    assert L.rvc_set_speaker(e._h, 3) == D.RVC_SHAPE and L.rvc_set_speaker(e._h, -1) == D.RVC_SHAPE and e.speaker_mix() == want
    assert L.rvc_set_speaker_mix(e._h, None, None, 1) == D.RVC_SHAPE and e.speaker_mix() == want
    n = C.c_size_t()
    assert L.rvc_speaker_mix(e._h, (i32 * 1)(), (f64 * 1)(), 1, C.byref(n)) == D.RVC_SHAPE and n.value == 2
    # reload / unload put the mix back to the blob's baked speaker; the baked speaker may be any row
    e.load_model(model)
    assert e.speaker_mix() == {0: 1.0}
    e.set_speaker(1); e.unload_model()
    assert e.speakers() == 0
    t1 = dict(tens); t1["sy.g"] = tens["sy.emb_g"][1]
    p1 = os.path.join(os.path.dirname(model), "model-tiny-v2-spk3-sid1.rvcw")
    W.write_blob(p1, cfg, t1)
    e.load_model(p1)
    assert e.speakers() == 3 and e.speaker_mix() == {1: 1.0}
    # a blob without a table: one speaker, id 0; set_speaker(0) launches nothing and changes no bit
    plain = zoo("tiny")["model"]
    e.load_model(plain); e.set_noise_seed(SEED, 0)
    assert e.speakers() == 1 and e.speaker_mix() == {0: 1.0}
    y0 = e.infer(x, FRAME, 12, SKIP, R)
    b0 = _biases(e, 0)
    e.set_profile(True)
    e.set_speaker(0); e.set_speaker_mix({0: 2.0})
    e.reset_state()
    y1 = e.infer(x, FRAME, 12, SKIP, R)
    assert D.same_bits(y0, y1) and D.same_bits(b0, _biases(e, 0)) and L.rvc_debug_speaker_fold_ms(e._h) == -1.0 and e.speaker_mix() == {0: 1.0}
    assert L.rvc_set_speaker(e._h, 1) == D.RVC_SHAPE and raw([0, 1], [0.5, 0.5]) == D.RVC_SHAPE
    e.close()
    # a table that does not hold sy.g is refused at load
    tbad = dict(tens); tbad["sy.g"] = tens["sy.g"] + np.float32(1.0)
    pbad = os.path.join(os.path.dirname(model), "model-tiny-v2-spk3-bad.rvcw")
    W.write_blob(pbad, cfg, tbad)
    e2 = RvcInfer(z["data"])
    with pytest.raises(RvcInferError):
        e2.load_model(pbad)
    e2.close()
