"""Many recordings in one call (obs_rvc_amd/csrc/convert_many.hip.h) on the tiny zoo (sr = 4800, zc = 48) at k = 2, C = 3, X = 2 (F = 63,
H = 54, n = 10 080): rvc_sola_stitch_many against rvc_sola_stitch per file bit for bit, rvc_convert_many against the composition of public calls bit for bit
(numpy gather per file, reset_state, infer_batch per batch in the packed order, sola_stitch per file), its independence of what the engine ran before, one
stream, one file against rvc_convert, the statuses.  No tolerance anywhere: both sides of every equality run kernels the existing suites hold to float64.
A HIP error ends the session: nothing more is started on the device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import convert_many_ref as M
from common import BASELINE_160MS as g160, voice_signal, zoo
from obs_rvc_amd import _native
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError

pytestmark = pytest.mark.gpu

ZC, RATE = 48, 4800
K, CTX, XF, H = 2, 3, 2, 54
LENGTHS = (1, 320 * H + 1, 160 * H, 160 * H + 1)      # W = 1, 3, 1, 2: seven windows
WINDOWS = [1, 3, 1, 2]
OUT = [48, 109 * 48, 54 * 48, 55 * 48]
SHIFT = 12
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


def engine(streams=3, f0="rmvpe"):
    z = zoo("tiny", 2)
    e = RvcInfer(z["data"])
    e.load_contentvec(2); e.load_model(z["model"]); e.load_f0_method(f0)
    e.set_streams(streams); e.set_noise_seed(1234, 0)
    return e


def recordings():
    """four files, each with its own tone and its own large DC level: a sample read from a neighbour in the arena shows"""
    out = []
    for n, hz, dc in zip(LENGTHS, (150.0, 220.0, 330.0, 180.0), (0.45, -0.4, 0.35, -0.5)):
        t = np.arange(n) / 16000.0
        out.append((dc + 0.3 * np.sin(2 * np.pi * hz * t) + 0.1 * np.sin(2 * np.pi * 3.1 * hz * t)).astype(np.float32))
    return out


def composition(e, xs, highpass=False):
    """what rvc_convert_many computes, from public calls: (rvc_highpass of each file alone,) a numpy gather per file with zeros outside the file, reset_state,
    infer_batch per batch in the packed order (the call's last batch padded with all-zero windows whose outputs are dropped), sola_stitch per file, each cut to
    its Nf zc samples -> (list of audio, offsets in global window order)"""
    if highpass:
        xs = [guard(e.highpass, x) for x in xs]
    wins = M.gather_windows_many(xs, RATE, K, CTX, XF)
    wpf = [len(w) for w in wins]
    geo = M.geometry([len(x) for x in xs], RATE, K, CTX, XF)
    assert wpf == geo["windows"]
    allw = np.concatenate(wins)
    W, S, n = len(allw), e.n_streams, allw.shape[1]
    order = [p for b in M.packing(wpf, S) for p in b]
    assert all(np.array_equal(allw[g], wins[f][w]) for g, (f, w) in enumerate(order))      # the packed order is files in order, windows in order
    pad = np.concatenate([allw, np.zeros(((-W) % S, n), np.float32)])
    e.reset_state()
    ys = [guard(e.infer_batch, pad[i: i + S], 5120 * (K - 1), SHIFT, CTX, H + XF + 1) for i in range(0, len(pad), S)]
    y = np.concatenate(ys)[:W]
    audio, offs, g = [], [], 0
    for f, Wf in enumerate(wpf):
        a, o = guard(e.sola_stitch, y[g: g + Wf], XF * ZC, ZC, H * ZC)
        audio.append(a[: geo["output_samples"][f]]); offs += o.tolist()
        g += Wf
    return audio, offs


def check_equal(got, info, ref, ref_off, batches):
    assert info["windows"] == 7 and info["batches"] == batches
    assert info["offsets"].tolist() == ref_off
    assert [len(a) for a in got] == OUT
    for f in range(len(ref)):
        assert same_bits(got[f], ref[f]), f
        assert np.all(np.isfinite(got[f]))


# ---------------------------------------------------------------- 1. stitch-many against the stitch per file
@pytest.fixture(scope="module")
def plain_engine():
    e = RvcInfer(zoo("tiny", 2)["data"])
    yield e
    e.close()


def stitch_files(sola_len, search, frame, shift):
    """three files of 4, 2 and 1 windows.  File 0 is the single-file suite's: random; a window that repeats its predecessor's tail at lag `shift`; all zeros (every
    lag ties); random.  File 1's first window repeats file 0's LAST tail at lag `shift`: a stitch that carried the tail over the file boundary finds it there"""
    r = np.random.default_rng(2024)
    wl = search + frame + sola_len
    w = r.uniform(-0.5, 0.5, (7, wl)).astype(np.float32)
    w[1, shift: shift + sola_len] = w[0, search + frame: search + frame + sola_len]      # window 0 meets the zero tail: offset = search
    w[2] = 0.0
    # window 3 follows the zero window's zero tail: offset = search, and the tail it leaves is its samples [search + frame, + sola_len)
    w[4, shift: shift + sola_len] = w[3, search + frame: search + frame + sola_len]
    return w, [4, 2, 1]


@pytest.mark.parametrize("sola_len,search,frame", [(96, 48, 240), (48, 48, 48)])
def test_stitch_many_is_the_stitch_per_file(plain_engine, sola_len, search, frame):
    e, shift = plain_engine, 17
    w, wpf = stitch_files(sola_len, search, frame, shift)
    audio, off = guard(e.sola_stitch_many, w, wpf, sola_len, search, frame)
    assert audio.shape == (7 * frame,) and off.shape == (7,)
    g = 0
    for Wf in wpf:
        a1, o1 = guard(e.sola_stitch, w[g: g + Wf], sola_len, search, frame)
        assert off[g: g + Wf].tolist() == o1.tolist(), g
        assert same_bits(audio[g * frame: (g + Wf) * frame], a1), g
        g += Wf
    assert off[:4].tolist() == [search, shift, search, search]
    assert off[4] == search and off[6] == search      # a file's first window meets silence: every lag ties and the last maximum wins
    # ... where one chain over all seven windows finds file 0's tail in file 1's first window
    _, chained = guard(e.sola_stitch, w, sola_len, search, frame)
    assert chained[4] == shift
    assert M.stitch_many(w, wpf, sola_len, search, frame)[1].tolist() == off.tolist()      # the fp64 search agrees on these windows
    # one file is rvc_sola_stitch itself
    a1, o1 = guard(e.sola_stitch_many, w[:4], [4], sola_len, search, frame)
    a2, o2 = guard(e.sola_stitch, w[:4], sola_len, search, frame)
    assert same_bits(a1, a2) and o1.tolist() == o2.tolist()


def test_stitch_many_refusals(plain_engine):
    w = np.zeros((3, 384), np.float32)
    for wpf, a in (([2, 1], (96, 48, 241)), ([2, 1], (97, 48, 96)), ([2, 1], (0, 48, 240)), ([], (96, 48, 240)), ([3, 0], (96, 48, 240)), ([2, 2], (96, 48, 240))):
        with pytest.raises(RvcInferError) as x:
            plain_engine.sola_stitch_many(w, wpf, *a)
        assert x.value.code == 5, (wpf, a)
    with pytest.raises(RvcInferError) as x:
        plain_engine.sola_stitch_many(np.zeros((1, 2000), np.float32), [1], 96, 1024, 240)      # search > 1023
    assert x.value.code == 5


# ---------------------------------------------------------------- 2. convert_many = the composition of public calls
def configure(e, case):
    if case == "index":
        e.load_index(np.random.default_rng(5).standard_normal((64, 48)).astype(np.float32))
        e.set_index_rate(0.5); e.set_protect(0.33)


@pytest.mark.parametrize("case", ["plain", "index", "yin"])
def test_convert_many_is_the_composition(case):
    e = engine(3, "yin" if case == "yin" else "rmvpe")
    configure(e, case)
    xs = recordings()
    assert M.packing(WINDOWS, 3) == [[(0, 0), (1, 0), (1, 1)], [(1, 2), (2, 0), (3, 0)], [(3, 1)]]
    ref, ref_off = composition(e, xs)
    got = guard(e.convert_many, xs, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    info = e.convert_many_info()
    check_equal(got, info, ref, ref_off, 3)
    assert info["ms_highpass"] == 0.0 and info["ms_model"] > 0 and info["ms_stitch"] > 0 and info["ms_total"] >= info["ms_model"]
    # high-pass on: the same composition fed rvc_highpass of each file alone
    ref_h, off_h = composition(e, xs, highpass=True)
    got_h = guard(e.convert_many, xs, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=True)
    info_h = e.convert_many_info()
    check_equal(got_h, info_h, ref_h, off_h, 3)
    assert info_h["ms_highpass"] > 0 and not same_bits(got_h[1], got[1])
    e.close()


# ---------------------------------------------------------------- 3. no dependence on history
def test_convert_many_does_not_depend_on_history():
    xs = recordings()
    fresh = engine(3)
    want = guard(fresh.convert_many, xs, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    want_off = fresh.convert_many_info()["offsets"].tolist()
    fresh.close()
    e = engine(3)
    junk = np.stack([voice_signal(g160.input_buffer_16k_size, seed=s) for s in (1, 2, 3)])
    for _ in range(3):      # another geometry: pitch caches and chunk counters are left dirty
        guard(e.infer_batch, junk, g160.sample_frame_16k, 0, g160.skip_head, g160.model_return_length)
    got = guard(e.convert_many, xs, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    assert all(same_bits(a, b) for a, b in zip(got, want)) and len(got) == 4 and e.convert_many_info()["offsets"].tolist() == want_off
    e.close()


# ---------------------------------------------------------------- 4. one stream
def test_convert_many_one_stream():
    e = engine(1)
    xs = recordings()
    ref, ref_off = composition(e, xs)
    got = guard(e.convert_many, xs, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    check_equal(got, e.convert_many_info(), ref, ref_off, 7)
    e.close()


# ---------------------------------------------------------------- 5. one file is rvc_convert
@pytest.mark.parametrize("highpass", [False, True])
def test_one_file_is_convert(highpass):
    e = engine(3)
    x = voice_signal(160 * 233 + 77, seed=11)      # Nf = 234, W = 5: two batches
    want, _ = guard(e.convert, x, k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=highpass)
    want_info = e.convert_info()
    got = guard(e.convert_many, [x], k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=highpass)
    info = e.convert_many_info()
    assert len(got) == 1 and same_bits(got[0], want)
    assert info["windows"] == want_info["windows"] == 5 and info["batches"] == want_info["batches"] == 2 and info["offsets"].tolist() == want_info["offsets"].tolist()
    e.close()


# ---------------------------------------------------------------- 6. statuses
def test_convert_many_statuses():
    L, z = _native.lib(), zoo("tiny", 2)
    xs = recordings()
    outs = [np.empty(n, np.float32) for n in OUT]
    lens = (C.c_size_t * 4)()

    def call(e, F=4, short=None, null_in=None, null_out=None, empty=None):
        for i in range(4):
            lens[i] = 0
        pin = (_FP * 4)(*[None if i == null_in else x.ctypes.data_as(_FP) for i, x in enumerate(xs)])
        pout = (_FP * 4)(*[None if i == null_out else o.ctypes.data_as(_FP) for i, o in enumerate(outs)])
        n = (C.c_size_t * 4)(*[0 if i == empty else len(x) for i, x in enumerate(xs)])
        cap = (C.c_size_t * 4)(*[len(o) - (1 if i == short else 0) for i, o in enumerate(outs)])
        return L.rvc_convert_many(e._h, pin, n, F, K, CTX, XF, SHIFT, 0, pout, cap, lens)

    def message(e):
        return L.rvc_last_error_message(e._h).decode()
    e = RvcInfer(z["data"])
    with pytest.raises(RvcInferError) as err:
        e.convert_many_info()                               # before a convert_many has completed
    assert err.value.code == 5
    assert call(e) == 1                                     # RVC_MODEL_NOT_LOADED, and before the arguments are looked at:
    assert call(e, F=0) == 1
    e.load_model(z["model"])
    assert call(e) == 2                                     # RVC_CONTENTVEC_NOT_LOADED
    e.load_contentvec(2)
    assert call(e) == 3                                     # RVC_F0_NOT_LOADED
    e.load_f0_method("yin")
    e.set_streams(3)
    assert call(e, short=1) == 5 and list(lens) == OUT      # cap[1] one short: RVC_SHAPE, every out_len written
    assert "1" in message(e) and "small" in message(e)
    assert call(e, F=0) == 5 and call(e, empty=2) == 5      # no file; an empty one in the middle
    assert call(e, null_in=2) == 5 and "null" in message(e)
    assert call(e, null_out=0) == 5 and "null" in message(e)
    assert L.rvc_convert_many(e._h, None, None, 4, K, CTX, XF, SHIFT, 0, None, None, lens) == 5
    assert L.rvc_convert_many(e._h, (_FP * 4)(*[x.ctypes.data_as(_FP) for x in xs]), (C.c_size_t * 4)(*LENGTHS), 4, 1, CTX, XF, 0, 0, None, None, lens) == 5      # k = 1
    assert "k" in message(e)
    e.set_auto_transpose(220.0)
    assert call(e) == 5 and "auto-transpose" in message(e) and list(lens) == [0, 0, 0, 0]
    e.set_auto_transpose(0.0)
    e.set_f0_curve([0.0, 1.0], [200.0, 220.0])
    assert call(e) == 5 and "curve" in message(e)
    with pytest.raises(RvcInferError):
        e.convert_many(xs, k=K, context=CTX, crossfade=XF)
    e.clear_f0_curve()
    with pytest.raises(RvcInferError):
        e.convert_many_info()                               # still none: no refused call has run anything
    # a conversion of one recording first: its info is there until a convert_many completes
    guard(e.convert, xs[3], k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)
    assert e.convert_info()["windows"] == 2 and len(e.convert_f0()) == 55
    assert guard(call, e) == 0 and list(lens) == OUT
    info = e.convert_many_info()
    assert info["windows"] == 7 and info["batches"] == 3 and len(info["offsets"]) == 7
    off = (C.c_int32 * 3)()
    assert L.rvc_convert_many_info(e._h, None, None, off, 3, None) == 0 and list(off) == info["offsets"][:3].tolist()
    for fn in (e.convert_info, e.convert_f0):               # ... and then they answer as before any conversion
        with pytest.raises(RvcInferError) as err:
            fn()
        assert err.value.code == 5
    e.close()


# ---------------------------------------------------------------- 7. the two info blocks through the one driver
def test_the_info_blocks_stay_apart():
    """rvc_convert and rvc_convert_many run one driver and report to two blocks.  (The statuses test above pins the other half: rvc_convert_many_info refused before
    any many call, rvc_convert_info and rvc_convert_f0 refused behind one.)  Here a conversion of one recording FOLLOWS a many call: it reports itself, brings the
    f0 grid back, and leaves the many call's windows, batches and offsets as they were"""
    e = engine(3)
    xs = recordings()
    guard(e.convert_many, xs[:2], k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)      # 1 + 3 windows on 3 streams: two batches
    many = e.convert_many_info()
    assert many["windows"] == 4 and many["batches"] == 2 and len(many["offsets"]) == 4
    with pytest.raises(RvcInferError):
        e.convert_f0()
    want, _ = guard(e.convert, xs[3], k=K, context=CTX, crossfade=XF, pitch_shift=SHIFT, highpass=False)      # 2 windows: one batch
    one = e.convert_info()
    assert one["windows"] == 2 and one["batches"] == 1 and len(one["offsets"]) == 2 and len(want) == OUT[3]
    assert len(e.convert_f0()) == 55
    after = e.convert_many_info()
    assert after["windows"] == 4 and after["batches"] == 2 and after["offsets"].tolist() == many["offsets"].tolist()
    assert [after[k] for k in ("ms_highpass", "ms_model", "ms_stitch", "ms_total")] == [many[k] for k in ("ms_highpass", "ms_model", "ms_stitch", "ms_total")]
    e.close()
