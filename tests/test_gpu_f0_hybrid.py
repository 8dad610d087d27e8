"""Hybrid f0 (rvc_load_f0_hybrid, f0_hybrid.hip.h) on the device, tiny zoo with the micro FCPE and the micro CREPE as crepe-tiny.

1. the combine kernel alone through rvc_debug_f0_hybrid, bit for bit against tests/f0_hybrid_ref.py, and its stand-alone RMVPE decode on a built salience;
2. members in a plan: the hybrid's row equals the reference applied to the rows the same engine returns under each member alone.  RMVPE as a member is held
   to the same bits too: the stand-alone decode restates pitch_post_kernel's expressions and the compiler contracts both alike (RMVPE_DECODE_BITWISE; the
   derived bound 64 * 2^-24 with identical voicing is what would apply otherwise, and is what the decode is held to against float64 in 1.);
3. a hybrid of one member is that method: the PCM of three consecutive chunks, bit for bit;
4. graph replay, pipelined calls, a member setting changed between chunks, protect, pitch controls on one stream, no plan build on a repeated call;
5. the surface: refusals leave everything as it was, read-back, back to a single method, a model without pitch guidance, the convert CLI.

rvc_pitch is a single-stream call, so the three-stream cases of 2. and 4. read each stream's row from the "f0" tap of an infer_batch call at pitch_shift 0 with
neutral controls: the same row of the same tail."""
from __future__ import annotations

import ctypes as C
import os
import wave

import numpy as np
import pytest
from scipy.signal import medfilt

import f0_hybrid_ref as H
import yin_ref as Y
from common import BASELINE_160MS as g, voice_signal, zoo
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc_common import F0_CREPE_TINY, F0_FCPE, F0_HYBRID, F0_RMVPE, F0_YIN, HYBRID_MEDIAN, HYBRID_VOTE, RvcInferError

pytestmark = pytest.mark.gpu

FRAME16K = g.sample_frame_16k          # 2560
RL = g.model_return_length
L = g.input_buffer_16k_size
_FP = C.POINTER(C.c_float)
RMVPE_DECODE_BITWISE = True
DECODE_REL = 64.0 * 2.0 ** -24          # 9-term sums, one division and powf on at most 7200 cents
assert FRAME16K == 2560 and Y.f0_frame(FRAME16K) == 4960


@pytest.fixture(scope="module")
def z():
    zz = zoo("tiny")
    W.write_fcpe(zz["data"], "micro")
    W.write_crepe(zz["data"], "micro", as_preset="tiny")
    return zz


def _engine(z, streams=1, model=True):
    from obs_rvc_amd.rvc import RvcInfer
    e = RvcInfer(z["data"])
    if model:
        e.load_contentvec(2); e.load_model(z["model"])
    if streams > 1:
        e.set_streams(streams)
    e.set_noise_seed(1234, 0)
    return e


def _inputs(S, chunk=0):
    """per stream a different voice buffer whose f0 window holds silence, a noise burst, a glide, tones (yin_ref.composite_signal), rotated per stream"""
    xs = np.stack([voice_signal(L, seed=10 * chunk + s + 1) for s in range(S)])
    for s in range(S):
        xs[s, -4960:] = np.roll(Y.composite_signal(seed=s + chunk)[-4960:], 900 * s + 300 * chunk)
    return xs


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def _combine(e, rows, mode, sal=None, rm_at=-1):
    rows = np.ascontiguousarray(rows, np.float32)
    n, B, Tm = rows.shape
    out, rm = np.full((B, Tm), -1.0, np.float32), np.full((B, Tm), -1.0, np.float32)
    salp = None if sal is None else np.ascontiguousarray(sal, np.float32).ctypes.data_as(_FP)
    rc = e._L.rvc_debug_f0_hybrid(e._h, rows.ctypes.data_as(_FP), n, B, Tm, mode, salp, rm_at, out.ctypes.data_as(_FP), rm.ctypes.data_as(_FP), None)
    assert rc == 0, (rc, e._L.rvc_last_error_message(e._h))
    return out, rm


# frames that between them reach every class, as member values in member order (padded / cut to n below); 220 twice: equal values among members
_PATTERNS = {
    1: [[220.0], [0.0], [float("nan")], [-40.0], [1e-3]],
    2: [[220.0, 110.0], [220.0, 220.0], [220.0, 0.0], [0.0, 220.0], [0.0, 0.0], [float("nan"), 330.0], [-40.0, 330.0], [330.0, float("nan")], [440.0, 441.0]],
    3: [[220.0, 110.0, 330.0], [220.0, 220.0, 100.0], [0.0, 110.0, 330.0], [220.0, 0.0, 0.0], [0.0, 0.0, 0.0], [float("nan"), 110.0, 330.0], [-1.0, -2.0, 330.0],
        [330.0, 0.0, 110.0], [100.0, 300.0, 200.0]],
    4: [[220.0, 110.0, 330.0, 440.0], [220.0, 220.0, 220.0, 100.0], [0.0, 110.0, 330.0, 440.0], [220.0, 0.0, 0.0, 0.0], [220.0, 110.0, 0.0, 0.0],
        [0.0, 0.0, 330.0, 440.0], [0.0, 110.0, 0.0, 440.0], [0.0, 0.0, 0.0, 0.0], [float("nan"), 110.0, 330.0, -5.0], [400.0, 100.0, 300.0, 200.0],
        [float("nan"), float("nan"), 7.0, 9.0]],
}
_WANT = {1: {"all_voiced_odd", "all_unvoiced"}, 2: {"all_voiced_even", "all_unvoiced", "tie_lead_voiced", "tie_lead_unvoiced"},
         3: {"all_voiced_odd", "all_unvoiced", "majority_voiced", "majority_unvoiced"},
         4: {"all_voiced_even", "all_unvoiced", "majority_voiced", "majority_unvoiced", "tie_lead_voiced", "tie_lead_unvoiced"}}


def _hand_rows(n, B, Tm, seed):
    """(n, B, Tm): the patterns first (as far as Tm reaches, rotated per stream so that Tm = 1 sees a different one per stream), random voiced / unvoiced after"""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(60.0, 900.0, size=(n, B, Tm)).astype(np.float32)
    rows[rng.random(rows.shape) < 0.4] = 0.0
    pats = np.array(_PATTERNS[n], np.float32).T          # (n, P)
    P = pats.shape[1]
    for b in range(B):
        k = min(P, Tm)
        rows[:, b, :k] = np.roll(pats, -b * 2 - seed, axis=1)[:, :k]
    return rows


@pytest.fixture(scope="module")
def bare(z):
    e = _engine(z, streams=3, model=False)
    yield e
    e.close()


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", [HYBRID_VOTE, HYBRID_MEDIAN])
def test_combine_kernel_bitwise(bare, n, mode):
    classes, nan_seen, neg_seen, eq_seen = set(), False, False, False
    for B in (1, 3):
        for Tm in (1, 5, 33, 1024):
            for seed in range(len(_PATTERNS[n]) if Tm == 1 else 1):          # Tm = 1: every pattern gets its turn in frame 0
                rows = _hand_rows(n, B, Tm, seed)
                got, _ = _combine(bare, rows, mode)
                want = H.combine(rows, mode)
                assert np.array_equal(_bits(got), _bits(want)), (n, mode, B, Tm, np.argwhere(_bits(got) != _bits(want))[:4])
                flat = np.nan_to_num(rows.reshape(n, -1), nan=-1.0)          # (a NaN is unvoiced, as a negative value is)
                classes |= {H.frame_class(flat[:, i]) for i in range(flat.shape[1])}
                nan_seen |= bool(np.isnan(rows).any()); neg_seen |= bool((flat < 0).any() and (rows < 0).any())
                eq_seen |= any(len(set(c[c > 0].tolist())) < int((c > 0).sum()) for c in flat.T[:64])
    assert classes == _WANT[n], classes ^ _WANT[n]
    assert nan_seen and neg_seen and (eq_seen or n == 1)


@pytest.mark.parametrize("mode", [HYBRID_VOTE, HYBRID_MEDIAN])
def test_swapping_the_lead_changes_exactly_the_tie_frames(bare, mode):
    for n in (2, 3, 4):
        rows = _hand_rows(n, 3, 33, 1)
        swapped = rows.copy(); swapped[[0, n - 1]] = rows[[n - 1, 0]]
        a, _ = _combine(bare, rows, mode)
        b, _ = _combine(bare, swapped, mode)
        with np.errstate(invalid="ignore"):
            on = rows > 0
        tie = (2 * on.sum(axis=0) == n) & (on[0] != on[n - 1])          # an exact tie in which the two leads disagree
        changed = _bits(a) != _bits(b)
        if mode == HYBRID_VOTE:
            assert np.array_equal(changed, tie) and (tie.any() or n == 3)
        else:
            assert not changed.any()          # the plain median has no lead


def _decode64(sal, thr=0.03):
    """RMVPE's salience decode as pitch_post_kernel has it (rmvpe.rs:118-133, 243-248: the arg-max is taken on the row padded by 4, "first strictly greater
    wins" from a best of 0, and the nine values are gathered from the UNPADDED row at that index) in float64 on sal [360][Tm] -> (hz [Tm], the largest
    salience per frame)"""
    sal = np.asarray(sal, np.float64)
    hz = np.zeros(sal.shape[1])
    for t in range(sal.shape[1]):
        i = int(np.argmax(sal[:, t]))
        s = i + 4 if sal[i, t] > 0 else 0
        assert s + 8 < 360
        w = sal[s:s + 9, t]
        c = np.sum(w * ((np.arange(s, s + 9) - 4.0) * 20.0 + 1997.3794084376191)) / np.sum(w)
        if not sal[:, t].max() > thr:
            c = 0.0
        f = 10.0 * 2.0 ** (c / 1200.0)
        hz[t] = 0.0 if f == 10.0 else f
    return hz, sal.max(axis=0)


@pytest.mark.parametrize("Tm", [1, 5, 33, 1024])
def test_standalone_decode_and_combine(bare, Tm):
    """a built salience (one bump per frame wandering over the bins, decoys below it, every fifth frame under the threshold, peaks at both ends of the scan
    range) decoded in place of member 1 of three: the decoded row against float64 within DECODE_REL with identical voicing, the combination bit for bit on it"""
    B = 3
    rng = np.random.default_rng(Tm)
    sal = (0.02 * rng.random((B, 360, Tm))).astype(np.float32)
    k = np.arange(360)[None, :, None]
    centre = rng.integers(0, 345, size=(B, 1, Tm)); centre[:, 0, ::7] = 0; centre[:, 0, 3::11] = 344
    height = np.where(np.arange(Tm) % 5 == 4, 0.025, 0.6).astype(np.float32)[None, None, :]
    sal = np.maximum(sal, (height * np.exp(-0.5 * ((k - centre) / 1.5) ** 2)).astype(np.float32))
    rows = _hand_rows(3, B, Tm, 2)
    got, rm = _combine(bare, rows, HYBRID_VOTE, sal=sal, rm_at=1)
    for b in range(B):
        ref, top = _decode64(sal[b])
        sure = np.abs(top - 0.03) > 1e-6
        assert np.array_equal(rm[b][sure] > 0, ref[sure] > 0)
        v = sure & (ref > 0)
        err = float(np.max(np.abs(rm[b][v] - ref[v]) / ref[v])) if v.any() else 0.0
        print("Tm %d stream %d: voiced %d of %d, decode against float64 %.3e (bound %.3e)" % (Tm, b, v.sum(), Tm, err, DECODE_REL))
        assert err <= DECODE_REL and (v.any() or Tm == 1)
    full = rows.copy(); full[1] = rm
    assert np.array_equal(_bits(got), _bits(H.combine(full, HYBRID_VOTE)))
    got2, rm2 = _combine(bare, rows, HYBRID_MEDIAN, sal=sal, rm_at=1)
    assert _same(rm2, rm) and np.array_equal(_bits(got2), _bits(H.combine(full, HYBRID_MEDIAN)))


def test_debug_aid_refuses_bad_shapes(bare):
    rows = np.zeros((2, 1, 8), np.float32)
    out = np.zeros((1, 8), np.float32)
    call = lambda n, B, Tm, mode, rm_at: bare._L.rvc_debug_f0_hybrid(bare._h, rows.ctypes.data_as(_FP), n, B, Tm, mode, None, rm_at, out.ctypes.data_as(_FP), None, None)
    assert call(2, 1, 8, 0, -1) == 0
    for bad in ((0, 1, 8, 0, -1), (5, 1, 8, 0, -1), (2, 0, 8, 0, -1), (2, 4, 8, 0, -1), (2, 1, 0, 0, -1), (2, 1, 1025, 0, -1), (2, 1, 8, 2, -1), (2, 1, 8, 0, 0)):
        assert call(*bad) == 5, bad


# ------------------------------------------------------------------------------------------------ 2. members in a plan
def _rows(e, xs, shift=0):
    """the tail's f0 row of every stream: rvc_pitch at one stream, the "f0" tap of an infer_batch call otherwise"""
    if e.n_streams == 1:
        return e.pitch(xs[0], shift, FRAME16K)[None]
    e.infer_batch(xs, FRAME16K, shift, g.skip_head, RL)
    return np.stack([e.tap("f0", s) for s in range(e.n_streams)])


@pytest.fixture(scope="module")
def member_rows(z):
    """{S: (engine, inputs, {member: rows (S, 32)})}: each single method's rows on the engine the hybrids then run on, computed once"""
    out = {}
    for S in (1, 3):
        e = _engine(z, S)
        xs = _inputs(S)
        rows = {}
        for m in ("rmvpe", "yin", "crepe-tiny", "fcpe"):
            e.load_f0_method(m)
            rows[m] = _rows(e, xs)
            assert rows[m].shape == (S, 32) and np.all(np.isfinite(rows[m])) and np.all(rows[m] >= 0)
        out[S] = (e, xs, rows)
    yield out
    for e, _, _ in out.values():
        e.close()


def _check_against_members(got, members, rows, mode, what):
    stack = np.stack([rows[m] for m in members])
    want = H.combine(stack, mode)
    v = (stack > 0).sum(axis=0)
    print("%s: voiced members per frame %s, combined voiced %d of %d" % (what, np.bincount(v.ravel(), minlength=len(members) + 1).tolist(), (want > 0).sum(), want.size))
    if RMVPE_DECODE_BITWISE or "rmvpe" not in members:
        assert np.array_equal(_bits(got), _bits(want)), (what, np.argwhere(_bits(got) != _bits(want))[:4])
    else:
        assert np.array_equal(got > 0, want > 0)
        on = want > 0
        assert not on.any() or np.max(np.abs(got[on].astype(np.float64) - want[on]) / want[on]) <= DECODE_REL


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("members", [("rmvpe", "fcpe"), ("yin", "fcpe"), ("fcpe", "yin"), ("rmvpe", "yin", "crepe-tiny"), ("crepe-tiny", "rmvpe", "fcpe", "yin")])
@pytest.mark.parametrize("mode", ["vote", "median"])
def test_members_in_a_plan(member_rows, S, members, mode):
    e, xs, rows = member_rows[S]
    e.load_f0_hybrid(list(members), mode=mode)
    assert e.f0_method == F0_HYBRID
    got = _rows(e, xs)
    _check_against_members(got, members, rows, H.VOTE if mode == "vote" else H.MEDIAN, "hybrid[%s] %s S=%d" % ("+".join(members), mode, S))
    assert len(members) < 2 or any(not _same(rows[members[0]], rows[m]) for m in members[1:])          # the members do disagree
    # pitch_shift 12 is a factor of exactly 2 on the combined row
    assert np.array_equal(_bits(_rows(e, xs, 12)), _bits(got * np.float32(2.0)))


# ------------------------------------------------------------------------------------------------ 3. a hybrid of one is the method
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("member", ["yin", "fcpe", "crepe-tiny", "rmvpe"])
def test_hybrid_of_one_is_the_method(z, S, member):
    e = _engine(z, S)
    chunks = [_inputs(S, k) for k in range(3)]
    runs = []
    for hybrid in (False, True):
        if hybrid:
            e.load_f0_hybrid([member])
        else:
            e.load_f0_method(member)
        e.reset_state(); e.set_noise_seed(1234, 0)
        pcm = [e.infer_batch(x, FRAME16K, [12, 0, -12][:S], g.skip_head, RL) for x in chunks]          # the pitch cache carries over from chunk to chunk
        runs.append((pcm, [e.pitch_cache(s) for s in range(S)]))
    (pa, ca), (pb, cb) = runs
    assert e.f0_method == F0_HYBRID and e.f0_hybrid() == ([e._F0_NAMES[member]], HYBRID_VOTE)
    assert all(np.all(np.isfinite(a)) for a in pa) and any(np.any(c > 0) for c in ca)
    assert all(_same(a, b) for a, b in zip(ca, cb)), "pitch cache"
    assert all(_same(a, b) for a, b in zip(pa, pb)), "PCM"
    e.close()


# ------------------------------------------------------------------------------------------------ 4. integration with hybrid[rmvpe+fcpe]
def test_graph_replay_and_pipelined_calls(z):
    import torch
    e = _engine(z, 3)
    e.load_f0_hybrid(["rmvpe", "fcpe"])
    chunks = [_inputs(3, k) for k in range(3)]

    def run():
        e.reset_state(); e.set_noise_seed(1234, 0)
        return [e.infer_batch(x, FRAME16K, 0, g.skip_head, RL) for x in chunks], [e.pitch_cache(s) for s in range(3)]
    eager, cache = run()
    builds = e.plan_cache_info()["builds"]
    again, _ = run()
    assert e.plan_cache_info()["builds"] == builds and all(_same(a, b) for a, b in zip(eager, again))          # a repeated call builds nothing
    e.set_use_graph(True)
    graph, gcache = run()
    e.set_use_graph(False)
    assert all(_same(a, b) for a, b in zip(eager, graph)) and all(_same(a, b) for a, b in zip(cache, gcache)) and any(np.any(c > 0) for c in cache)
    # unsynchronised pipelined calls on device buffers: the same sequence twice, bit for bit
    n_out = eager[0].shape[1]
    d_in = [torch.from_numpy(x).cuda() for x in chunks]
    outs = []
    e.set_pipeline(True)
    for _ in range(2):
        e.reset_state(); e.set_noise_seed(1234, 0)
        d_out = [torch.zeros((3, n_out), dtype=torch.float32, device="cuda") for _ in chunks]
        torch.cuda.synchronize()
        for di, do in zip(d_in, d_out):
            assert e.infer_device(di.data_ptr(), L, FRAME16K, 0, g.skip_head, RL, do.data_ptr(), n_out, sync=False) == n_out
        e.synchronize()
        outs.append([o.cpu().numpy() for o in d_out])
    e.set_pipeline(False)
    assert all(_same(a, b) for a, b in zip(outs[0], outs[1])) and all(np.all(np.isfinite(a)) for a in outs[0])
    e.close()


def test_member_setting_changes_the_plan_between_chunks(member_rows):
    e, xs, rows = member_rows[1]
    builds = lambda: e.plan_cache_info()["builds"]
    try:
        e.load_f0_method("fcpe"); e.set_fcpe_threshold(0.9)          # FCPE alone under the raised threshold: it calls nothing voiced any more
        alone = e.pitch(xs[0], 0, FRAME16K)
        e.set_fcpe_threshold(0.006)
        e.load_f0_hybrid(["rmvpe", "fcpe"])          # (loading RMVPE drops every plan, as rvc_load_f0 does: no load between the calls below)
        base = e.pitch(xs[0], 0, FRAME16K)
        n = builds()
        assert _same(e.pitch(xs[0], 0, FRAME16K), base) and builds() == n
        e.set_fcpe_threshold(0.9)          # a plan of its own, from the next call on
        hi = e.pitch(xs[0], 0, FRAME16K)
        assert builds() == n + 1
        want = H.combine(np.stack([rows["rmvpe"][0], alone]), H.VOTE)
        assert np.array_equal(_bits(hi), _bits(want)) and not np.any(alone > 0) and np.any(rows["fcpe"][0] > 0)
        assert np.array_equal(hi > 0, rows["rmvpe"][0] > 0) and not _same(hi, base)          # with FCPE silent every frame is a tie, and RMVPE leads
    finally:
        e.set_fcpe_threshold(0.006)
    assert _same(e.pitch(xs[0], 0, FRAME16K), base) and builds() == n + 1          # the old value finds its plan again


def test_protect_and_pitch_controls(z, member_rows):
    _, xs, rows = member_rows[3]
    e = _engine(z, 3)
    e.load_f0_hybrid(["rmvpe", "fcpe"])
    rng = np.random.default_rng(3)
    e.load_index(rng.standard_normal((64, 48)).astype(np.float32)); e.set_index_rate(0.5)
    off = e.infer_batch(xs, FRAME16K, 0, g.skip_head, RL)
    e.reset_state(); e.set_noise_seed(1234, 0)
    e.set_protect(0.2)
    on = e.infer_batch(xs, FRAME16K, 0, g.skip_head, RL)
    assert np.all(np.isfinite(on)) and np.all(np.isfinite(off)) and on.shape == off.shape
    e.set_protect(0.5); e.set_index_rate(0.0)
    # controls on stream 1 only: a gate and a median of radius 3 -- selection, so the float32 restatement is exact: gate, then medfilt, of the combined row
    e.set_f0_range(80.0, 600.0, 1); e.set_f0_median(3, 1)
    got = _rows(e, xs)
    comb = H.combine(np.stack([rows["rmvpe"], rows["fcpe"]]), H.VOTE)
    gated = comb[1].copy(); gated[(gated > 0) & ((gated < 80.0) | (gated > 600.0))] = 0
    want1 = medfilt(gated, 7).astype(np.float32)
    assert np.array_equal(_bits(got[0]), _bits(comb[0])) and np.array_equal(_bits(got[2]), _bits(comb[2]))
    assert np.array_equal(_bits(got[1]), _bits(want1))
    print("controls on stream 1: %d of 32 rows changed by them" % int(np.sum(_bits(want1) != _bits(comb[1]))))
    e.close()


# ------------------------------------------------------------------------------------------------ 5. the surface
def test_refusals_leave_everything_as_it_was(z, tmp_path):
    from obs_rvc_amd.rvc import RvcInfer
    e = _engine(z, 1, model=False)
    x = _inputs(1)[0]
    L_ = e._L
    raw = lambda ms, mode, n=None: L_.rvc_load_f0_hybrid(e._h, (C.c_int * max(len(ms), 1))(*ms), len(ms) if n is None else n, mode)
    for state in ("yin", ["fcpe", "yin"]):
        if isinstance(state, str):
            e.load_f0_method(state)
        else:
            e.load_f0_hybrid(state, "median")
        method, hyb, base = e.f0_method, e.f0_hybrid(), e.pitch(x, 0, FRAME16K)
        for ms, mode, n in (([], 0, 0), ([1, 2, 4, 5, 7], 0, None), ([1, 1], 0, None), ([2, 7, 2], 0, None), ([0], 0, None), ([3], 0, None), ([6], 0, None),
                            ([8], 0, None), ([2, 8], 0, None), ([-1], 0, None), ([99], 0, None), ([2], 2, None), ([2], -1, None), ([2], 0, -1)):
            assert raw(ms, mode, n) == 5 and L_.rvc_last_error_message(e._h), (ms, mode, n)
            assert e.f0_method == method and e.f0_hybrid() == hyb
        assert L_.rvc_load_f0_hybrid(e._h, None, 2, 0) == 5
        with pytest.raises(RvcInferError) as ei:
            e.load_f0_method(8)
        assert ei.value.kind == "NdarrayShapeError" and e.f0_method == method and e.f0_hybrid() == hyb
        assert _same(e.pitch(x, 0, FRAME16K), base)
    e.close()
    # a member's missing file: RVC_BACKEND, whichever member it is, and nothing of the earlier members stays behind
    W.write_fcpe(str(tmp_path), "micro")
    e = RvcInfer(str(tmp_path))
    e.load_f0_method("fcpe")
    base = e.pitch(x, 0, FRAME16K)
    for ms in (["fcpe", "rmvpe"], ["yin", "crepe-tiny", "fcpe"], ["crepe", "fcpe"]):
        with pytest.raises(RvcInferError) as ei:
            e.load_f0_hybrid(ms)
        assert ei.value.kind == "Backend" and e.f0_method == F0_FCPE and e.f0_hybrid() is None
    assert _same(e.pitch(x, 0, FRAME16K), base)
    e.close()


def test_read_back_and_return_to_a_single_method(member_rows):
    e, xs, rows = member_rows[1]
    m = np.zeros(4, np.int32); mode = C.c_int(-1)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    e.load_f0_method("yin")
    assert e.f0_hybrid() is None and e._L.rvc_f0_hybrid(e._h, ip(m), 4, C.byref(mode)) == 0 and mode.value == -1 and not m.any()
    e.load_f0_hybrid(["fcpe", "rmvpe", "yin"], "median")
    assert e.f0_method == F0_HYBRID and e.f0_hybrid() == ([F0_FCPE, F0_RMVPE, F0_YIN], HYBRID_MEDIAN)
    assert e._L.rvc_f0_hybrid(e._h, ip(m), 2, None) == 3 and m.tolist() == [F0_FCPE, F0_RMVPE, 0, 0]          # cap is honoured, n is the whole count
    assert e._L.rvc_f0_hybrid(e._h, None, 0, C.byref(mode)) == 3 and mode.value == HYBRID_MEDIAN
    e.load_f0_hybrid(["yin", F0_CREPE_TINY])
    assert e.f0_hybrid() == ([F0_YIN, F0_CREPE_TINY], HYBRID_VOTE)
    e.load_f0_method("hybrid[rmvpe+fcpe]")          # the string form, under the default mode
    assert e.f0_hybrid() == ([F0_RMVPE, F0_FCPE], HYBRID_VOTE)
    for single in ("yin", "fcpe", "rmvpe"):
        e.load_f0_method(single)
        assert e.f0_hybrid() is None and e.f0_method == e._F0_NAMES[single]
        assert _same(e.pitch(xs[0], 0, FRAME16K)[None], rows[single])
    e.load_f0_hybrid(["yin"]); e.load_f0()
    assert e.f0_method == F0_RMVPE and e.f0_hybrid() is None


def test_model_without_pitch_guidance_accepts_and_ignores_it(z):
    from obs_rvc_amd.rvc import RvcInfer
    path = os.path.join(os.path.dirname(z["model"]), "model-tiny-nof0-v2.rvcw")
    if not os.path.exists(path):
        W.write_blob(path, *W.make_synth("tiny", 48, f0=False))
    x = _inputs(1)[0]
    outs = []
    for hybrid in (False, True):
        e = RvcInfer(z["data"]); e.load_contentvec(2); e.load_model(path); e.set_noise_seed(1234, 0)
        assert e.model_has_f0() is False
        if hybrid:
            e.load_f0_hybrid(["rmvpe", "fcpe"])
            assert e.f0_method == F0_HYBRID
        outs.append(e.infer(x, FRAME16K, None, g.skip_head, RL))
        assert not np.any(e.pitch_cache() != 0)
        if hybrid:
            assert e.pitch(x, 0, FRAME16K).shape == (32,)          # rvc_pitch is the tracker's
        e.close()
    assert _same(outs[0], outs[1]) and np.all(np.isfinite(outs[0]))


def test_convert_cli_runs_a_hybrid(z, tmp_path):
    from obs_rvc_amd.build_index import read_wav
    from obs_rvc_amd.convert import main
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    x = voice_signal(16000, seed=4)
    with wave.open(src, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.clip(np.rint(x * 32767.0), -32768, 32767).astype("<i2").tobytes())
    assert main([src, "-o", dst, "--model", z["model"], "--data", z["data"], "--f0", "hybrid[yin+fcpe]", "--f0-hybrid-mode", "median", "--streams", "2", "--window", "2",
                 "--context", "8", "--crossfade", "2"]) == 0
    y, rate = read_wav(dst)
    assert len(y) > 0 and rate > 0 and np.all(np.isfinite(y)) and np.any(y != 0)
