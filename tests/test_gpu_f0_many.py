"""A pitch per recording for rvc_convert_many (f0_analyze_many.hip.h, f0_select_many.hip.h, convert_many.hip.h) on the tiny zoo with YIN
at k = 2, C = 3, X = 2 (H = 54): four files of 1, 320 H + 1, 160 H and 160 H + 1 samples (W = 1, 3, 1, 2), each with its own tone (110 / 165 / 247 / 370 Hz)
and its own DC level, at S = 3 and S = 1.

No tolerance anywhere.  rvc_f0_stats_many is compared with rvc_f0_stats per file and the numpy definition, rvc_analyze_f0_many with rvc_analyze_f0 per file,
rvc_convert_many under a per-file pitch with the composition of public calls (gather per file, reset_state, rvc_set_pitch_semitones_stream per stream and batch,
infer_batch in the packed order, sola_stitch per file), all bit for bit: both sides of every equality run kernels the existing suites hold to float64.
A HIP error ends the session: nothing more is started on the device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import convert_many_ref as M
import f0_many_ref as FM
import f0_stats_ref as S
import silence_ref as SR
from common import BASELINE_160MS as g160, voice_signal, zoo
from obs_rvc_amd import _native
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError

pytestmark = pytest.mark.gpu

ZC, RATE = 48, 4800
K, CTX, XF, H, RL = 2, 3, 2, 54, 57
LENGTHS = (1, 320 * H + 1, 160 * H, 160 * H + 1)      # W = 1, 3, 1, 2: seven windows
WINDOWS = [1, 3, 1, 2]
ROWS = [1, 109, 54, 55]
TONES = (110.0, 165.0, 247.0, 370.0)
LIST = [0.0, 3.0, -5.0, 12.0]
DB, HANG = -40.0, 2
_FP = C.POINTER(C.c_float)
_SZ = C.POINTER(C.c_size_t)


def guard(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except RvcInferError as x:
        if "hip" in str(x).lower():
            pytest.exit("a HIP call failed (%s): nothing more is started on this device" % x, returncode=3)
        raise


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def engine(streams=3, f0="yin", model=True):
    z = zoo("tiny", 2)
    e = RvcInfer(z["data"])
    if model:
        e.load_contentvec(2); e.load_model(z["model"])
    e.load_f0_method(f0)
    e.set_streams(streams); e.set_noise_seed(1234, 0)
    return e


def harmonic(n, f0, dc=0.0):
    t = np.arange(n) / 16000.0
    return (dc + 0.3 * sum(np.sin(2 * np.pi * f0 * h * t) / h for h in range(1, 6))).astype(np.float32)


def recordings():
    """four files, each with its own pitch and its own DC level: a row or a sample taken from a neighbour moves the result"""
    return [harmonic(n, hz, dc) for n, hz, dc in zip(LENGTHS, TONES, (0.45, -0.4, 0.35, -0.5))]


GATED_ACTIVE = [True, True, False, True, False, True, True]


def gated_recordings():
    """the gate's files, W = 1, 3, 1, 2 again: file 1 has three whole windows and voice in windows 0 and 2 only -- its middle window is silent --, file 2 is
    room tone throughout; active windows GATED_ACTIVE (checked against tests/silence_ref.py where they are used)"""
    xs = recordings()
    room = lambda n, seed: (1e-4 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)
    x1 = room(160 * 3 * H, 1)
    for a, b in ((5, 45), (2 * H + 12, 2 * H + 45)):
        x1[160 * a: 160 * b] = harmonic(160 * (b - a), TONES[1])
    xs = [xs[0], x1, room(LENGTHS[2], 2), xs[3]]
    act = np.concatenate([SR.analyze(x, DB, HANG, K, CTX, XF)["active"] for x in xs])
    assert act.tolist() == GATED_ACTIVE and all(SR.margin(x, DB) > 1e-9 for x in xs)
    return xs


@pytest.fixture(scope="module")
def plain_engine():
    e = RvcInfer(zoo("tiny", 2)["data"])
    yield e
    e.close()


@pytest.fixture(scope="module")
def analysis():
    """rvc_analyze_f0 of every file alone at S = 3, and its median: the reference of the analysis and of the auto-transpose tests -> (rows, medians, voiced)"""
    e = engine(3, model=False)
    rows = [guard(e.analyze_f0, x, K, CTX, XF, highpass=False) for x in recordings()]
    stats = [guard(e.f0_stats, r) for r in rows]
    e.close()
    med, voiced = np.float32([s[0][0] for s in stats]), [s[1] for s in stats]
    assert [len(r) for r in rows] == ROWS and voiced[0] == 0 and min(voiced[1:]) > 20
    for m, hz in zip(med[1:], TONES[1:]):
        assert abs(float(m) - hz) < 0.03 * hz, (m, hz)          # (the files really differ in pitch; nothing below depends on how well YIN tracks)
    return rows, med, voiced


# ---------------------------------------------------------------- 1. the segmented select
def segments():
    """segments of 1, 2, 255, 256, 257, 8192, 8193 and 70 001 rows -- around the workgroup's 256 threads and the one-launch limit of the single select --, laid
    end to end so that every one but the first starts at an odd, unaligned row; all-unvoiced and single-voiced segments lie between voiced neighbours"""
    kinds = {1: "one voiced row", 2: "two values one ulp apart", 255: "NaN, +inf and negative rows", 256: "all unvoiced", 257: "a positive denormal among normal values",
             8192: "one voiced row", 8193: "log-uniform 50-1100 Hz, 40 % zeros", 70001: "NaN, +inf and negative rows"}
    segs = [S.select_inputs(n)[kinds[n]] for n in (1, 2, 255, 256, 257, 8192, 8193, 70001)]
    segs.insert(5, S.select_inputs(333, seed=1)["two values one ulp apart"])
    segs.append(S.select_inputs(1000, seed=2)["all rows equal"])
    offs = np.cumsum([0] + [len(s) for s in segs])[:-1]
    assert sum(int(o) % 4 != 0 for o in offs) >= 7
    return segs


@pytest.mark.parametrize("quantiles", [(0.5,), (0.0, 0.05, 0.25, 0.5, 0.5, 0.75, 0.95, 1.0)])
def test_stats_many_is_stats_per_file(plain_engine, quantiles):
    e, segs = plain_engine, segments()
    out, v = guard(e.f0_stats_many, segs, quantiles)
    assert out.shape == (len(segs), len(quantiles)) and out.dtype == np.float32
    for f, x in enumerate(segs):
        q1, v1 = guard(e.f0_stats, x, quantiles)
        q0, v0 = S.select(x, quantiles)
        assert v[f] == v1 == v0, f
        assert same_bits(out[f], q1) and same_bits(out[f], q0), f
    assert v[3] == 0 and not np.any(out[3]) and v[0] == 1 and v[6] == 1
    # one file is rvc_f0_stats itself
    for x in (segs[8], segs[0]):
        o1, v1 = guard(e.f0_stats_many, [x], quantiles)
        q1, vv = guard(e.f0_stats, x, quantiles)
        assert same_bits(o1[0], q1) and v1 == [vv]


def test_stats_many_refusals(plain_engine):
    e = plain_engine
    x = np.ones(4, np.float32)
    for rows, q in (([], (0.5,)), ([x, x[:0]], (0.5,)), ([x], ()), ([x], (0.5,) * 9), ([x], (1.5,)), ([x], (float("nan"),))):
        with pytest.raises(RvcInferError) as err:
            e.f0_stats_many(rows, q)
        assert err.value.code == 5, (len(rows), q)
    L = _native.lib()
    rows, q, out = (C.c_size_t * 1)(4), (C.c_double * 1)(0.5), (C.c_float * 1)()
    assert L.rvc_f0_stats_many(e._h, None, rows, 1, q, 1, out, None) == 5 and L.rvc_f0_stats_many(e._h, x.ctypes.data_as(_FP), None, 1, q, 1, out, None) == 5
    assert L.rvc_f0_stats_many(e._h, x.ctypes.data_as(_FP), rows, 65537, q, 1, out, None) == 5
    assert L.rvc_f0_stats_many(e._h, x.ctypes.data_as(_FP), rows, 1, q, 1, out, None) == 0 and out[0] == 1.0


# ---------------------------------------------------------------- 2. the packed analysis
@pytest.mark.parametrize("streams,highpass", [(3, False), (1, False), (3, True)])
def test_analyze_many_is_analyze_per_file(analysis, streams, highpass):
    e = engine(streams, model=False)
    xs = recordings()
    got = guard(e.analyze_f0_many, xs, K, CTX, XF, highpass=highpass)
    assert [len(r) for r in got] == ROWS
    for f, x in enumerate(xs):
        want = guard(e.analyze_f0, x, K, CTX, XF, highpass=highpass)
        assert same_bits(got[f], want), f
        if not highpass:
            assert same_bits(got[f], analysis[0][f]), f          # YIN is one kernel at every batch size: S = 1 gives S = 3's rows
    assert not same_bits(got[2], got[1][:54]) and np.any(got[3] > 0)
    # the segmented select of the rows is the select per file
    med, v = guard(e.f0_stats_many, got)
    for f in range(4):
        m1, v1 = guard(e.f0_stats, got[f])
        assert same_bits(med[f], m1) and v[f] == v1
    e.close()


def test_analyze_many_under_the_silence_gate():
    e = engine(3, model=False)
    xs = gated_recordings()
    ungated = guard(e.analyze_f0_many, xs, K, CTX, XF, highpass=False)
    e.set_convert_silence(DB, HANG)
    got = guard(e.analyze_f0_many, xs, K, CTX, XF, highpass=False)
    s = e.convert_silence_info()
    assert s["windows_run"] == 5 and s["windows_skipped"] == 2 and [len(r) for r in got] == [1, 3 * H, H, H + 1]
    for f, x in enumerate(xs):
        assert same_bits(got[f], guard(e.analyze_f0, x, K, CTX, XF, highpass=False)), f
    # the skipped middle window's rows are 0, its neighbours' rows are what they are without the gate
    assert not np.any(got[1][H: 2 * H]) and same_bits(got[1][:H], ungated[1][:H]) and same_bits(got[1][2 * H:], ungated[1][2 * H:]) and np.any(got[1][:H] > 0)
    assert same_bits(got[0], ungated[0]) and not np.any(got[2]) and same_bits(got[3], ungated[3])
    e.close()


def test_analyze_many_statuses():
    L, z = _native.lib(), zoo("tiny", 2)
    xs = recordings()
    outs = [np.empty(n, np.float32) for n in ROWS]
    rows = (C.c_size_t * 4)()

    def call(e, F=4, short=None, null_in=None, null_out=None, empty=None, k=K):
        for i in range(4):
            rows[i] = 0
        pin = (_FP * 4)(*[None if i == null_in else x.ctypes.data_as(_FP) for i, x in enumerate(xs)])
        pout = (_FP * 4)(*[None if i == null_out else o.ctypes.data_as(_FP) for i, o in enumerate(outs)])
        n = (C.c_size_t * 4)(*[0 if i == empty else len(x) for i, x in enumerate(xs)])
        cap = (C.c_size_t * 4)(*[len(o) - (1 if i == short else 0) for i, o in enumerate(outs)])
        return L.rvc_analyze_f0_many(e._h, pin, n, F, k, CTX, XF, 0, pout, cap, rows)
    e = RvcInfer(z["data"])
    assert call(e) == 3 and call(e, F=0) == 3                    # RVC_F0_NOT_LOADED, before any argument is looked at
    e.load_f0_method("yin"); e.set_streams(3)
    builds = e.plan_cache_info()["builds"]
    assert call(e, short=1) == 5 and list(rows) == ROWS          # cap[1] one short: RVC_SHAPE, every n_frames written
    msg = L.rvc_last_error_message(e._h).decode()
    assert "1" in msg and "small" in msg
    assert call(e, F=0) == 5 and call(e, empty=2) == 5 and call(e, k=1) == 5
    assert call(e, null_in=2) == 5 and call(e, null_out=0) == 5
    assert e.plan_cache_info()["builds"] == builds              # nothing was built, nothing launched, on a refused call
    assert guard(call, e) == 0 and list(rows) == ROWS           # ... and neither a voice model nor ContentVec is needed
    e.close()


# ---------------------------------------------------------------- 3. convert_many with a pitch per file
def composition(e, xs, t, active=None, shift=0):
    """what rvc_convert_many computes under a per-file pitch, from public calls: a numpy gather per file, reset_state, in front of every batch
    set_pitch_semitones(t_f(s), stream s) for its streams (0 for the padded ones), infer_batch in the packed order (under the gate: the active windows,
    compacted, and zero windows put back at the skipped places), sola_stitch per file -> (list of audio, offsets in global window order)"""
    wins = M.gather_windows_many(xs, RATE, K, CTX, XF)
    wpf = [len(w) for w in wins]
    geo = M.geometry([len(x) for x in xs], RATE, K, CTX, XF)
    act = np.ones(sum(wpf), bool) if active is None else np.asarray(active, bool)
    run = np.concatenate(wins)[act]
    A, S_, n = len(run), e.n_streams, run.shape[1]
    pad = np.concatenate([run, np.zeros(((-A) % S_, n), np.float32)])
    sts = FM.stream_semitones(wpf, S_, t, None if active is None else act)
    e.reset_state()
    ys = []
    try:
        for b, i in enumerate(range(0, len(pad), S_)):
            for s in range(S_):
                e.set_pitch_semitones(sts[b][s], stream=s)
            ys.append(guard(e.infer_batch, pad[i: i + S_], 5120 * (K - 1), shift, CTX, RL))
    finally:
        for s in range(S_):
            e.set_pitch_semitones(0.0, stream=s)
    y = SR.insert_zero_windows(np.concatenate(ys)[:A], SR.places(act), RL * ZC)
    audio, offs, g = [], [], 0
    for f, Wf in enumerate(wpf):
        a, o = guard(e.sola_stitch, y[g: g + Wf], XF * ZC, ZC, H * ZC)
        audio.append(a[: geo["output_samples"][f]]); offs += o.tolist()
        g += Wf
    return audio, offs


def many(e, xs, shift=0):
    got = guard(e.convert_many, xs, k=K, context=CTX, crossfade=XF, pitch_shift=shift, highpass=False)
    return got, e.convert_many_info()["offsets"].tolist()


def check(got, ref):
    assert got[1] == ref[1]
    assert len(got[0]) == len(ref[0])
    for f in range(len(ref[0])):
        assert same_bits(got[0][f], ref[0][f]), f
        assert np.all(np.isfinite(got[0][f]))


@pytest.fixture(scope="module")
def cleared():
    """rvc_convert_many of a fresh engine with nothing set -> (audio, offsets, plans built)"""
    e = engine(3)
    got = many(e, recordings())
    builds = e.plan_cache_info()["builds"]
    e.close()
    return got[0], got[1], builds


@pytest.mark.parametrize("streams", [3, 1])
def test_a_semitone_list_is_the_composition(cleared, analysis, streams):
    e = engine(streams)
    xs = recordings()
    with pytest.raises(RvcInferError):
        e.convert_many_pitch_info()                              # before any run
    e.set_convert_many_pitch(LIST)
    got = many(e, xs)
    info = e.convert_many_pitch_info()
    assert info["semitones"].tolist() == LIST and not np.any(info["auto_semitones"]) and info["ms_analysis"] > 0 and info["ms_select"] > 0
    assert same_bits(info["median_hz"], analysis[1]) and info["voiced"] == analysis[2]
    check(got, composition(e, xs, LIST))
    if streams == 3:      # file 0 (t = 0, alone with files of t = 3 in its batch) is the cleared call's; the others are not
        assert same_bits(got[0][0], cleared[0][0])
        assert all(not same_bits(got[0][f], cleared[0][f]) for f in (1, 2, 3))
        # composes with pitch_shift, and the list is read again by the next call
        check(many(e, xs, shift=12), composition(e, xs, LIST, shift=12))
    e.close()


def test_auto_transpose_per_file(cleared, analysis):
    rows, med, voiced = analysis
    e = engine(3)
    xs = recordings()
    e.set_convert_many_auto_transpose(220.0, 0, 24.0)
    assert e.convert_many_auto_transpose() == {"target_hz": 220.0, "step": 0, "limit": 24.0} and e.auto_transpose()["target_hz"] == 0.0
    got = many(e, xs)
    info = e.convert_many_pitch_info()
    assert same_bits(info["median_hz"], med) and info["voiced"] == voiced
    a, t = FM.file_semitones(None, 220.0, med, voiced, 0, 24.0)
    assert info["auto_semitones"].tolist() == a.tolist() and info["semitones"].tolist() == t.tolist()
    assert a[0] == 0.0 and 4.5 < a[1] < 5.5 and -2.5 < a[2] < -1.5 and -9.5 < a[3] < -8.5          # the one-sample file has no voiced row: 0
    check(got, composition(e, xs, t))
    assert same_bits(got[0][0], cleared[0][0]) and not same_bits(got[0][3], cleared[0][3])
    total = e.convert_many_info()
    assert total["ms_total"] >= total["ms_model"] + info["ms_analysis"]          # the total includes the pass
    # the list and the target compose; whole octaves
    e.set_convert_many_pitch(LIST)
    e.set_convert_many_auto_transpose(220.0, 12, 24.0)
    got = many(e, xs)
    a, t = FM.file_semitones(LIST, 220.0, med, voiced, 12, 24.0)
    info = e.convert_many_pitch_info()
    assert a.tolist() == [0.0, 0.0, 0.0, -12.0] and t.tolist() == [0.0, 3.0, -5.0, 0.0]
    assert info["auto_semitones"].tolist() == a.tolist() and info["semitones"].tolist() == t.tolist()
    check(got, composition(e, xs, t))
    # limit 2 clamps files 1 and 3
    e.set_convert_many_pitch(None)
    e.set_convert_many_auto_transpose(220.0, 0, 2.0)
    got = many(e, xs)
    a, t = FM.file_semitones(None, 220.0, med, voiced, 0, 2.0)
    assert a[1] == 2.0 and a[3] == -2.0 and -2.0 <= a[2] < 0.0 and e.convert_many_pitch_info()["semitones"].tolist() == t.tolist()
    check(got, composition(e, xs, t))
    e.close()


def test_auto_transpose_under_the_silence_gate():
    e = engine(3)
    xs = gated_recordings()
    act = np.array(GATED_ACTIVE)
    e.set_convert_silence(DB, HANG)
    rows = guard(e.analyze_f0_many, xs, K, CTX, XF, highpass=False)
    med, voiced = guard(e.f0_stats_many, rows)
    e.set_convert_many_pitch([1.0, 0.0, 7.0, 0.0])
    e.set_convert_many_auto_transpose(220.0, 0, 24.0)
    got = many(e, xs)
    info = e.convert_many_pitch_info()
    a, t = FM.file_semitones([1.0, 0.0, 7.0, 0.0], 220.0, med[:, 0], voiced, 0, 24.0)
    assert same_bits(info["median_hz"], med[:, 0]) and info["voiced"] == voiced and info["semitones"].tolist() == t.tolist()
    assert voiced[0] == 0 and voiced[2] == 0 and t[0] == 1.0 and t[2] == 7.0 and t[1] > 4 and t[3] < -8
    # compacted: batch 0 holds windows (0, 0), (1, 0), (1, 2), batch 1 holds (3, 0), (3, 1) and one padded stream
    assert FM.stream_semitones(WINDOWS, 3, t, act) == [[t[0], t[1], t[1]], [t[3], t[3], 0.0]]
    assert e.convert_many_info()["batches"] == 2
    check(got, composition(e, xs, t, active=act))
    assert not np.any(got[0][2])
    e.close()


def test_auto_transpose_with_an_index():
    e = engine(3)
    e.load_index(np.random.default_rng(5).standard_normal((64, 48)).astype(np.float32))
    e.set_index_rate(0.5)
    xs = recordings()
    e.set_convert_many_auto_transpose(220.0, 1, 12.0)
    got = many(e, xs)
    t = e.convert_many_pitch_info()["semitones"]
    assert t.tolist() == [0.0, 5.0, -2.0, -9.0]
    check(got, composition(e, xs, t))
    e.close()


# ---------------------------------------------------------------- 4. neutrality
def test_cleared_settings_are_the_parent_call(cleared):
    e = engine(3)
    e.set_convert_many_pitch(LIST); e.set_convert_many_auto_transpose(220.0, 12, 24.0)
    e.set_convert_many_pitch(None); e.set_convert_many_auto_transpose(0.0, 12, 24.0)
    got = many(e, recordings())
    assert all(same_bits(a, b) for a, b in zip(got[0], cleared[0])) and got[1] == cleared[1]
    assert e.plan_cache_info()["builds"] == cleared[2]          # no pitch-only plan, no other plan: nothing was queued for the pass
    with pytest.raises(RvcInferError):
        e.convert_many_pitch_info()
    e.close()


def test_the_factor_is_gone_behind_the_call():
    L, R = g160.input_buffer_16k_size, g160.model_return_length
    chunk = np.stack([voice_signal(L, seed=s + 1) for s in range(3)])
    x = recordings()[3]
    fresh = engine(3)
    c_fresh = guard(fresh.infer_batch, chunk, g160.sample_frame_16k, 0, g160.skip_head, R)
    y_fresh, _ = guard(fresh.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=0, highpass=False)
    fresh.close()
    e = engine(3)
    e.set_convert_many_pitch(LIST); e.set_convert_many_auto_transpose(220.0, 0, 24.0)
    many(e, recordings())
    assert np.any(e.convert_many_pitch_info()["semitones"] != 0)
    # streaming calls and the single-file converter never read the settings, on or off: the per-stream factor left with the call
    e.reset_state()
    assert same_bits(guard(e.infer_batch, chunk, g160.sample_frame_16k, 0, g160.skip_head, R), c_fresh)
    y, _ = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=0, highpass=False)
    assert same_bits(y, y_fresh)
    e.close()


# ---------------------------------------------------------------- 5. statuses
def test_per_file_pitch_statuses(cleared):
    L = _native.lib()
    e = engine(3)
    xs = recordings()
    message = lambda: L.rvc_last_error_message(e._h).decode()
    with pytest.raises(RvcInferError) as err:
        e.convert_many_pitch_info()
    assert err.value.code == 5
    for bad in ([0.0, 24.5, 0.0, 0.0], [0.0, 0.0, -25.0, 0.0], [float("nan"), 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, float("inf")]):
        assert not FM.check_pitch_list(bad)
        with pytest.raises(RvcInferError) as err:
            e.set_convert_many_pitch(bad)
        assert err.value.code == 5, bad
    for bad in ((-1.0, 1, 12.0), (20000.5, 1, 12.0), (float("nan"), 1, 12.0), (155.0, 2, 12.0), (155.0, 1, 24.5), (155.0, 1, float("nan"))):
        assert not S.check_auto_transpose_args(*bad)
        with pytest.raises(RvcInferError) as err:
            e.set_convert_many_auto_transpose(*bad)
        assert err.value.code == 5 and "auto transpose" in str(err.value), bad
    assert e.convert_many_auto_transpose() == {"target_hz": 0.0, "step": 1, "limit": 12.0}          # refused calls changed nothing:
    assert all(same_bits(a, b) for a, b in zip(many(e, xs)[0], cleared[0]))                        # ... the list is still cleared
    # a list whose length is not the call's F: RVC_SHAPE with a message, nothing launched
    e.set_convert_many_pitch([1.0, 2.0, 3.0])
    builds = e.plan_cache_info()["builds"]
    with pytest.raises(RvcInferError) as err:
        e.convert_many(xs, k=K, context=CTX, crossfade=XF, highpass=False)
    assert err.value.code == 5 and "3 entries" in message() and "4 recordings" in message() and e.plan_cache_info()["builds"] == builds
    # a curve set stays refused, and rvc_set_auto_transpose in force too, whatever the per-file settings say
    e.set_convert_many_pitch(LIST)
    e.set_f0_curve([0.0, 1.0], [200.0, 220.0])
    with pytest.raises(RvcInferError):
        e.convert_many(xs, k=K, context=CTX, crossfade=XF, highpass=False)
    assert "curve" in message()
    e.clear_f0_curve()
    e.set_auto_transpose(220.0)
    with pytest.raises(RvcInferError):
        e.convert_many(xs, k=K, context=CTX, crossfade=XF, highpass=False)
    assert "auto-transpose" in message()
    e.set_auto_transpose(0.0)
    with pytest.raises(RvcInferError):
        e.convert_many_pitch_info()                              # still none: no refused call ran the pass
    many(e, xs)
    m = (C.c_float * 2)()
    assert L.rvc_convert_many_pitch_info(e._h, m, None, None, None, 2, None) == 0 and m[0] == 0.0 and abs(m[1] - 165.0) < 5.0
    e.close()
