"""The file converter's silence gate (obs_rvc_amd/csrc/silence.hip.h) on the tiny zoo (sr = 4800, zc = 48) at k = 2, C = 3, X = 2
(H = 54, return_length = 57), S = 3: rvc_silence_map against the float64 definition of tests/silence_ref.py, masks and places exactly equal; the gated
rvc_convert / rvc_convert_many / rvc_convert_file / rvc_analyze_f0 against the composition of public calls bit for bit (gather of the active windows,
reset_state, infer_batch per compacted batch, zero windows inserted, sola_stitch); off is off; graph replay.  No tolerance anywhere.
A HIP error ends the session: nothing more is started on the device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import convert_many_ref as M
import convert_ref as R
import f0_override_ref as OV
import silence_ref as SR
from common import voice_signal, zoo
from obs_rvc_amd import _native
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError

pytestmark = pytest.mark.gpu

ZC, RATE = 48, 4800
K, CTX, XF, H, RL = 2, 3, 2, 54, 57
SHIFT = 12
DB, HANG = -40.0, 2
_FP = C.POINTER(C.c_float)
_U8 = C.POINTER(C.c_uint8)


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


def engine(streams=3, f0="rmvpe"):
    z = zoo("tiny", 2)
    e = RvcInfer(z["data"])
    e.load_contentvec(2); e.load_model(z["model"]); e.load_f0_method(f0)
    e.set_streams(streams); e.set_noise_seed(1234, 0)
    return e


@pytest.fixture(scope="module")
def plain_engine():
    e = RvcInfer(zoo("tiny", 2)["data"])
    yield e
    e.close()


def masked(n, speech, seed=11, tone=1e-4):
    """a voice in the frames `speech` (pairs [a, b) of 10 ms frames), room tone (white noise, about -80 dB) everywhere else"""
    x = voice_signal(n, seed=seed)
    m = np.zeros(n, bool)
    for a, b in speech:
        m[160 * a: 160 * b] = True
    room = (tone * np.random.default_rng(seed + 100).standard_normal(n)).astype(np.float32)
    return np.where(m, x, room).astype(np.float32)


# the recording of the composition tests: Nf = 9 * 54 + 7 = 493, ten windows.  Window w returns frames [54 w, 54 w + 57); with hang = 2 the four stretches of
# voice below make windows 1, 2, 5 and 7 active: a leading silent window, a run of two skipped ones, one skipped between two active ones, trailing silence, and
# A = 4 is no multiple of S = 3
N10 = 160 * 492 + 77
SPEECH = ((64, 100), (120, 151), (285, 311), (395, 421))
ACTIVE10 = [False, True, True, False, False, True, False, True, False, False]


def recording10():
    return masked(N10, SPEECH)


# ---------------------------------------------------------------- 1. the map against the float64 definition
def level_signal(n, db):
    """a sine whose RMS is `db` dB"""
    t = np.arange(n) / 16000.0
    return (np.sqrt(2.0) * 10.0 ** (db / 20.0) * np.sin(2 * np.pi * 250.0 * t)).astype(np.float32)


def map_cases():
    r = np.random.default_rng(7)
    out = []
    for nf in (1, 3, 4, 53, 54, 55, 9 * 54 + 7):
        n = 160 * nf - int(r.integers(0, 159))
        speech = [(a, min(a + 3, nf)) for a in range(int(r.integers(0, 5)), nf, 17)]
        out.append(("nf%d" % nf, masked(n, speech, seed=nf), DB))
    last = np.zeros(160 * 20 + 31, np.float32)
    last[160 * 20:] = 0.5                                      # the only loud samples lie in the last, partial frame
    out.append(("last_partial", last, DB))
    out.append(("all_silent", masked(160 * 120, ()), DB))
    out.append(("all_zero", np.zeros(160 * 60 + 1, np.float32), DB))
    out.append(("all_loud", voice_signal(160 * 120, seed=5), DB))
    out.append(("above", level_signal(160 * 70, DB + 0.1), DB))
    out.append(("below", level_signal(160 * 70, DB - 0.1), DB))
    return out


MAP_CASES = map_cases()


def check_map(e, x, db, hang):
    assert SR.margin(x, db) > 1e-9                             # a condition on the inputs: no frame sits on the threshold
    ref = SR.analyze(x, db, hang, K, CTX, XF)
    got = guard(e.silence_map, x, db, hang, k=K, context=CTX, crossfade=XF, sample_rate=RATE)
    for key in ("loud", "kept", "active"):
        assert got[key].shape == ref[key].shape and np.array_equal(got[key], ref[key]), key
    assert got["place"].tolist() == ref["place"].tolist()
    info = e.convert_silence_info()
    assert info["windows_run"] == int(ref["active"].sum()) and info["windows_skipped"] == int((~ref["active"]).sum())
    assert info["frames_loud"] == int(ref["loud"].sum()) and info["frames_kept"] == int(ref["kept"].sum())
    return ref


@pytest.mark.parametrize("name,x,db", MAP_CASES, ids=[c[0] for c in MAP_CASES])
def test_silence_map_is_the_definition(plain_engine, name, x, db):
    for hang in (0, 1, 5, 60, 1000):
        ref = check_map(plain_engine, x, db, hang)
    if name in ("all_silent", "all_zero", "below"):
        assert not ref["loud"].any() and not ref["active"].any()
    if name in ("all_loud", "above"):
        assert ref["loud"][:-3].all() and ref["active"].all()
    if name == "last_partial":
        assert ref["loud"].tolist() == [False] * 17 + [True] * 4


def test_silence_map_scans_long_recordings(plain_engine):
    nf = 70001                                                 # 69 rounds of the one-workgroup scan, 1297 windows: two rounds of the compaction
    x = np.zeros(160 * nf, np.float32)
    for i in range(5, nf, 300):
        x[160 * i + 40: 160 * i + 120] = 0.5                   # one isolated stretch of 5 ms every 300 frames: loud frames i - 3 .. i
    for hang in (0, 60, 1000):
        ref = check_map(plain_engine, x, DB, hang)
    assert ref["loud"].sum() == 4 * len(range(5, nf, 300)) and ref["active"].all()
    ref0 = SR.analyze(x, DB, 0, K, CTX, XF)
    assert 0 < ref0["active"].sum() < len(ref0["active"])


def test_silence_refusals(plain_engine):
    e, L = plain_engine, _native.lib()
    e.set_convert_silence(-45.0, 7)
    assert e.convert_silence() == {"threshold_db": -45.0, "hang_frames": 7, "on": True}
    for bad in ((float("nan"), 5), (-40.0, -1), (-40.0, 1001)):
        with pytest.raises(RvcInferError) as err:
            e.set_convert_silence(*bad)
        assert err.value.code == 5
        assert e.convert_silence() == {"threshold_db": -45.0, "hang_frames": 7, "on": True}
    e.set_convert_silence(-60.0)
    assert e.convert_silence() == {"threshold_db": -60.0, "hang_frames": 30, "on": False}
    x = recording10()
    nf, w = 493, 10
    fl, fk, wa, wp = np.zeros(nf, np.uint8), np.zeros(nf, np.uint8), np.zeros(w, np.uint8), np.zeros(w, np.int32)

    def call(db=DB, hang=HANG, cap_f=nf, cap_w=w, n=len(x), k=K):
        return L.rvc_silence_map(e._h, x.ctypes.data_as(_FP), n, db, hang, k, CTX, XF, RATE, fl.ctypes.data_as(_U8), fk.ctypes.data_as(_U8), cap_f, wa.ctypes.data_as(_U8),
                                 wp.ctypes.data_as(C.POINTER(C.c_int32)), cap_w)
    assert guard(call) == 0 and wa.tolist() == [int(v) for v in ACTIVE10]
    for kw in (dict(db=float("nan")), dict(hang=-1), dict(hang=1001), dict(cap_f=nf - 1), dict(cap_w=w - 1), dict(n=0), dict(k=1)):
        assert call(**kw) == 5, kw
    # every output pointer may be NULL
    assert L.rvc_silence_map(e._h, x.ctypes.data_as(_FP), len(x), DB, HANG, K, CTX, XF, RATE, None, None, 0, None, None, 0) == 0
    assert e.convert_silence() == {"threshold_db": -60.0, "hang_frames": 30, "on": False}


# ---------------------------------------------------------------- 2. gated convert = the composition of public calls
def composition(e, x, db=DB, hang=HANG):
    """gather of the active windows in order, reset_state, infer_batch per compacted batch (the last one padded with all-zero windows whose outputs are dropped),
    zero windows inserted at the skipped positions, sola_stitch, cut to Nf zc samples -> (audio, offsets, place, batches).  The engine's gate plays no part"""
    geo = RvcInfer.convert_geometry(len(x), RATE, K, CTX, XF)
    x = np.asarray(x, np.float32)
    assert SR.margin(x, db) > 1e-9
    a = SR.analyze(x, db, hang, K, CTX, XF)
    win = R.gather_windows(x, geo)[a["active"]]
    A, S = len(win), e.n_streams
    pad = np.concatenate([win, np.zeros(((-A) % S, geo["n"]), np.float32)])
    e.reset_state()
    ys = [guard(e.infer_batch, pad[i: i + S], geo["sample_frame_16k_size"], SHIFT, geo["skip_head"], geo["return_length"]) for i in range(0, len(pad), S)]
    y = np.concatenate(ys)[:A] if A else np.zeros((0, RL * ZC), np.float32)
    full = SR.insert_zero_windows(y, a["place"], RL * ZC)
    audio, off = guard(e.sola_stitch, full, XF * ZC, ZC, H * ZC)
    return audio[: geo["output_samples"]], off.tolist(), a, len(pad) // S


def f0_rows_of_skipped(a, nf):
    """the frames whose f0 row belongs to a skipped window: frame g is exported by window g // H"""
    return ~np.repeat(a["active"], H)[:nf]


def configure(e, case):
    if case == "index":
        e.load_index(np.random.default_rng(5).standard_normal((64, 48)).astype(np.float32))
        e.set_index_rate(0.5); e.set_protect(0.33)


@pytest.mark.parametrize("case", ["plain", "index", "yin", "highpass", "one_stream"])
def test_gated_convert_is_the_composition(case):
    e = engine(1 if case == "one_stream" else 3, "yin" if case == "yin" else "rmvpe")
    configure(e, case)
    x = recording10()
    hp = case == "highpass"
    seen = guard(e.highpass, x) if hp else x                   # the mask comes from the signal the model sees
    ref, ref_off, a, batches = composition(e, seen)
    if not hp:
        assert a["active"].tolist() == ACTIVE10
    A = int(a["active"].sum())
    assert 0 < A < 10 and A % 3 != 0 and not a["active"][0] and not a["active"][-1]
    # the conditioned f0 rows (pitch_shift 12) of the ungated conversion: a window's rows depend on the window alone, not on the place it runs in
    guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=hp)
    f0_ungated = e.convert_f0()
    e.set_convert_silence(DB, HANG)
    got, rate = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=hp)
    info, s = e.convert_info(), e.convert_silence_info()
    assert rate == RATE and got.shape == (493 * ZC,) and info["windows"] == 10 and info["batches"] == batches == -(-A // e.n_streams)
    assert info["offsets"].tolist() == ref_off
    assert same_bits(got, ref) and np.all(np.isfinite(got))
    assert s["windows_run"] == A and s["windows_skipped"] == 10 - A and s["ms_analysis"] > 0
    assert not np.any(got[: 54 * ZC])                          # the leading silent window: zeros met by a zero tail
    f0 = e.convert_f0()
    skipped = f0_rows_of_skipped(a, 493)
    assert f0.shape == (493,) and not np.any(f0[skipped]) and np.any(f0[~skipped] > 0)
    assert same_bits(f0[~skipped], f0_ungated[~skipped])      # (a tracker may well call room tone unvoiced: nothing is claimed of the ungated rows elsewhere)
    e.close()


# ---------------------------------------------------------------- 2b. an f0 curve acts on the windows that run, by absolute frame
CURVE_T = np.array([1.1037, 1.6021, 2.2013, 3.0079])          # frames 111 .. 300: active window 2, the skipped windows 3 and 4, the head of active window 5
CURVE_HZ = np.array([150.0, 220.0, 0.0, 180.0], np.float32)


def test_gated_convert_under_a_curve():
    e = engine(3)
    x = recording10()
    geo = RvcInfer.convert_geometry(len(x), RATE, K, CTX, XF)
    og = OV.geometry(K, CTX, XF, 493)
    assert og["H"] == H and og["W"] == 10 and OV.grid_margin(CURVE_T, 493) >= 1e-6
    a = SR.analyze(x, DB, HANG, K, CTX, XF)
    skipped = f0_rows_of_skipped(a, 493)
    e.set_convert_silence(DB, HANG)
    conv = lambda: guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)[0]
    y0 = conv(); f0_0 = e.convert_f0()
    e.set_f0_curve(CURVE_T, CURVE_HZ)
    grid = e.f0_curve_grid(493)
    cov = ~np.isnan(grid)
    assert cov.sum() == 190 and (cov & ~skipped).sum() > 40 and (cov & skipped).sum() > 40 and (~cov & ~skipped).sum() > 40
    y1 = conv(); f0_1 = e.convert_f0(); off1 = e.convert_info()["offsets"].tolist()
    assert e.convert_info()["batches"] == 2 and not same_bits(y1, y0)
    assert not np.any(f0_1[skipped])                                                      # a skipped window's rows stay 0, curve or not
    assert same_bits(f0_1[cov & ~skipped], grid[cov & ~skipped] * np.float32(2.0))        # covered rows of windows that ran: the curve, an octave up
    assert same_bits(f0_1[~cov & ~skipped], f0_0[~cov & ~skipped])                        # uncovered ones: the tracker's, as without the curve
    # the composition: the compacted batches with each stream's override rows taken from the grid at ITS window's absolute frames
    win_of = np.flatnonzero(a["active"])
    win = R.gather_windows(np.asarray(x, np.float32), geo)[a["active"]]
    A, S = len(win), 3
    pad = np.concatenate([win, np.zeros(((-A) % S, geo["n"]), np.float32)])
    e.reset_state()
    ys = []
    for i in range(0, len(pad), S):
        for s_ in range(S):
            e.set_f0_override(s_, OV.window_override(grid, og, int(win_of[i + s_])) if i + s_ < A else None)
        ys.append(guard(e.infer_batch, pad[i: i + S], geo["sample_frame_16k_size"], SHIFT, geo["skip_head"], geo["return_length"]))
    full = SR.insert_zero_windows(np.concatenate(ys)[:A], a["place"], RL * ZC)
    audio, off = guard(e.sola_stitch, full, XF * ZC, ZC, H * ZC)
    assert same_bits(audio[: geo["output_samples"]], y1) and off.tolist() == off1
    e.close()


# ---------------------------------------------------------------- 3. nothing active
def test_all_silent_recording_runs_nothing():
    e = engine(3)
    x = masked(N10, ())
    e.set_convert_silence(DB, HANG)
    got, _ = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    info, s = e.convert_info(), e.convert_silence_info()
    assert got.shape == (493 * ZC,) and not np.any(got) and same_bits(got, np.zeros(493 * ZC, np.float32))
    assert info["windows"] == 10 and info["batches"] == 0 and info["ms_model"] == 0.0 and info["offsets"].tolist() == [ZC] * 10
    assert s["windows_run"] == 0 and s["windows_skipped"] == 10 and s["frames_loud"] == 0 and s["frames_kept"] == 0
    assert not np.any(e.convert_f0())
    hz = guard(e.analyze_f0, x, window=K, context=CTX, crossfade=XF, highpass=False)
    assert hz.shape == (493,) and not np.any(hz)
    e.close()


# ---------------------------------------------------------------- 4. many files
def test_gated_convert_many_is_the_composition():
    e = engine(3)
    # file 0: 4 windows, active 1, 2 (and 3 through voice near its end); file 1: all silent, 2 windows; file 2: 5 windows whose active ones straddle the batch
    # boundary at place 3; file 3: a single active window
    xs = [masked(160 * 200, ((64, 100), (120, 151), (180, 196)), seed=1), masked(160 * 100 + 5, (), seed=2),
          masked(160 * 260, ((10, 40), (70, 100), (230, 250)), seed=3), masked(160 * 30 + 9, ((5, 25),), seed=4)]
    wins = M.gather_windows_many(xs, RATE, K, CTX, XF)
    wpf = [len(w) for w in wins]
    assert wpf == [4, 2, 5, 1]
    maps = [SR.analyze(x, DB, HANG, K, CTX, XF) for x in xs]
    for x in xs:
        assert SR.margin(x, DB) > 1e-9
    act = np.concatenate([m["active"] for m in maps])
    assert act.tolist() == [False, True, True, True, False, False, True, True, False, False, True, True]
    A, S = int(act.sum()), 3
    assert A == 7 and not maps[1]["active"].any()
    allw = np.concatenate(wins)[act]
    pad = np.concatenate([allw, np.zeros(((-A) % S, allw.shape[1]), np.float32)])
    e.reset_state()
    ys = [guard(e.infer_batch, pad[i: i + S], 5120 * (K - 1), SHIFT, CTX, RL) for i in range(0, len(pad), S)]
    full = SR.insert_zero_windows(np.concatenate(ys)[:A], SR.places(act), RL * ZC)
    ref, ref_off, g = [], [], 0
    for f, Wf in enumerate(wpf):
        au, o = guard(e.sola_stitch, full[g: g + Wf], XF * ZC, ZC, H * ZC)
        ref.append(au[: -(-len(xs[f]) // 160) * ZC]); ref_off += o.tolist()
        g += Wf
    au_many, off_many = guard(e.sola_stitch_many, full, wpf, XF * ZC, ZC, H * ZC)
    assert off_many.tolist() == ref_off
    e.set_convert_silence(DB, HANG)
    got = guard(e.convert_many, xs, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    info, s = e.convert_many_info(), e.convert_silence_info()
    assert info["windows"] == 12 and info["batches"] == 3 and info["offsets"].tolist() == ref_off
    for f in range(4):
        assert same_bits(got[f], ref[f]), f
    assert not np.any(got[1]) and np.any(got[3])
    assert s["windows_run"] == 7 and s["windows_skipped"] == 5
    # every file silent: no batch, zeros
    quiet = [masked(160 * 100 + 5, (), seed=2), masked(31, (), seed=3)]
    out = guard(e.convert_many, quiet, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    assert e.convert_many_info()["batches"] == 0 and not np.any(out[0]) and not np.any(out[1]) and [len(o) for o in out] == [101 * ZC, ZC]
    e.close()


# ---------------------------------------------------------------- 5. a file at 44.1 kHz with the envelope
def test_gated_convert_file_is_the_composition():
    e = engine(3)
    rate_in, rms_mix = 44100, 0.5
    n_in = N10 * rate_in // 16000
    x = voice_signal(n_in, seed=11, sr=rate_in)
    m = np.zeros(n_in, bool)
    for a, b in SPEECH:
        m[a * rate_in // 100: b * rate_in // 100] = True
    x = np.where(m, x, (1e-4 * np.random.default_rng(3).standard_normal(n_in)).astype(np.float32)).astype(np.float32)
    e.set_convert_silence(DB, HANG)
    x16 = guard(e.resample, x, rate_in, 16000)
    y, sr = guard(e.convert, x16, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=True)      # the gated convert of section 2, its own high-pass
    ci = e.convert_info()
    assert 0 < ci["batches"] < -(-ci["windows"] // 3)
    y2 = guard(e.change_rms, guard(e.highpass, x16), 16000, y, sr, rms_mix)
    got, rate = guard(e.convert_file, x, rate_in, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=True, rms_mix_rate=rms_mix, out_rate=0)
    assert rate == sr == RATE and same_bits(got, y2)
    assert e.convert_info()["offsets"].tolist() == ci["offsets"].tolist() and e.convert_info()["batches"] == ci["batches"]
    e.close()


# ---------------------------------------------------------------- 6. analysis and auto-transpose
def test_gated_analysis_and_auto_transpose():
    e = engine(3, "yin")
    x = recording10()
    a = SR.analyze(x, DB, HANG, K, CTX, XF)
    skipped = f0_rows_of_skipped(a, 493)
    plain = guard(e.analyze_f0, x, window=K, context=CTX, crossfade=XF, highpass=False)
    e.set_convert_silence(DB, HANG)
    hz = guard(e.analyze_f0, x, window=K, context=CTX, crossfade=XF, highpass=False)
    assert e.convert_silence_info()["windows_run"] == 4
    assert hz.shape == (493,) and not np.any(hz[skipped]) and np.any(hz[~skipped] > 0)
    assert same_bits(hz[~skipped], plain[~skipped])            # a pitch-only window's rows depend on the window alone (neutral controls, no noise)
    med, voiced = guard(e.f0_stats, hz)
    e.set_auto_transpose(float(med[0]) * 2.0, 0, 24.0)
    guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=0, highpass=False)
    t = e.auto_transpose_info()
    assert t["median_hz"] == med[0] and t["voiced"] == voiced and abs(t["semitones"] - 12.0) < 1e-9
    e.close()


# ---------------------------------------------------------------- 7. off is off
def test_off_is_off():
    x = recording10()
    fresh = engine(3)
    want, _ = guard(fresh.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    want_info = fresh.convert_info()
    fresh.close()
    e = engine(3)
    e.set_convert_silence(-60.0)
    got, _ = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    assert same_bits(got, want) and e.convert_info()["batches"] == want_info["batches"] == 4 and e.convert_info()["offsets"].tolist() == want_info["offsets"].tolist()
    with pytest.raises(RvcInferError):
        e.convert_silence_info()                               # no call has run with the gate
    e.set_convert_silence(DB, HANG)
    gated, _ = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    assert not same_bits(gated, want) and e.convert_info()["batches"] == 2
    e.set_convert_silence(-75.0, 9)                            # at or below -60: off
    again, _ = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    assert same_bits(again, want) and e.convert_info()["batches"] == 4 and e.convert_info()["offsets"].tolist() == want_info["offsets"].tolist()
    # the setting survives a model load
    e.set_convert_silence(DB, HANG)
    e.load_model(zoo("tiny", 2)["model"])
    assert e.convert_silence() == {"threshold_db": DB, "hang_frames": HANG, "on": True}
    e.close()


# ---------------------------------------------------------------- 8. graph replay
def test_gated_convert_under_graph_replay():
    x = recording10()
    e = engine(3)
    e.set_convert_silence(DB, HANG)
    eager, _ = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    off = e.convert_info()["offsets"].tolist()
    e.set_use_graph(True)
    replay, _ = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    assert same_bits(replay, eager) and e.convert_info()["offsets"].tolist() == off and e.convert_info()["batches"] == 2
    e.close()
