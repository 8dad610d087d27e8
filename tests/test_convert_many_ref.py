"""rvc_convert_many's host-only parts: rvc_convert_many_geometry against the numpy restatement in tests/convert_many_ref.py and against
rvc_convert_geometry per file, its RVC_SHAPE cases, the numpy stitch-many against tests/convert_ref.py's stitch per file, and the plain functions of the
folder tool (argument parsing, file listing).  No GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import convert_many_ref as M
import convert_ref as R
from obs_rvc_amd import _native
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError

K, CTX, XF, RATE = 2, 3, 2, 4800          # F = 63, H = 54, n = 10 080, zc = 48: the composition tests' geometry
H = 54
LENGTHS = [1, 160 * H, 160 * H + 1, 320 * H + 1, 320 * H, 159, 160, 161, 160 * 233 + 77]


def c_geometry(lengths, rate, k, context, crossfade):
    F = len(lengths)
    n = (C.c_size_t * max(F, 1))(*lengths)
    w, o, tot = (C.c_size_t * max(F, 1))(), (C.c_size_t * max(F, 1))(), (C.c_size_t * 2)()
    rc = _native.lib().rvc_convert_many_geometry(n, F, rate, k, context, crossfade, w, o, tot)
    return rc, {"windows": [int(v) for v in w[:F]], "output_samples": [int(v) for v in o[:F]], "windows_total": int(tot[0]), "output_total": int(tot[1])}


def test_reference_self_checks():
    M.self_check()


@pytest.mark.parametrize("rate,k,context,crossfade", [(RATE, K, CTX, XF), (48000, 0, 0, 0), (40000, 16, 3, 1)])
def test_geometry_matches_the_restatement_and_the_single_file_call(rate, k, context, crossfade):
    rc, got = c_geometry(LENGTHS, rate, k, context, crossfade)
    want = M.geometry(LENGTHS, rate, k, context, crossfade)
    assert rc == 0 and got == want, (got, want)
    for f, n in enumerate(LENGTHS):
        one = RvcInfer.convert_geometry(n, rate, k, context, crossfade)
        assert (got["windows"][f], got["output_samples"][f]) == (one["windows"], one["output_samples"]), (f, n)
    assert got["windows_total"] == sum(got["windows"]) and got["output_total"] == sum(got["output_samples"])
    assert RvcInfer.convert_many_geometry(LENGTHS, rate, k, context, crossfade) == want
    # a file's numbers do not depend on its neighbours or its place
    rc, rev = c_geometry(LENGTHS[::-1], rate, k, context, crossfade)
    assert rc == 0 and rev["windows"] == got["windows"][::-1] and rev["output_samples"] == got["output_samples"][::-1]


def test_geometry_window_counts_at_the_hop():
    rc, g = c_geometry([1, 160 * H, 160 * H + 1, 320 * H + 1], RATE, K, CTX, XF)
    assert rc == 0 and g["windows"] == [1, 1, 2, 3] and g["output_samples"] == [48, 54 * 48, 55 * 48, 109 * 48] and g["windows_total"] == 7
    # the GPU suite's four files
    rc, g = c_geometry([1, 320 * H + 1, 160 * H, 160 * H + 1], RATE, K, CTX, XF)
    assert rc == 0 and g["windows"] == [1, 3, 1, 2] and g["windows_total"] == 7 and g["output_total"] == 219 * 48
    # NULL outputs are allowed, each on its own
    n = (C.c_size_t * 2)(1, 161)
    tot = (C.c_size_t * 2)()
    assert _native.lib().rvc_convert_many_geometry(n, 2, RATE, K, CTX, XF, None, None, tot) == 0 and list(tot) == [2, 3 * 48]
    assert _native.lib().rvc_convert_many_geometry(n, 2, RATE, K, CTX, XF, None, None, None) == 0


def test_geometry_refusals():
    L = _native.lib()
    for lengths in ([], [160, 0, 160], [0], [160, 160, 0]):      # F = 0; an empty recording in the middle, alone, at the end
        assert M.geometry(lengths, RATE, K, CTX, XF) is None
        assert c_geometry(lengths, RATE, K, CTX, XF)[0] == 5
        with pytest.raises(RvcInferError):
            RvcInfer.convert_many_geometry(lengths, RATE, K, CTX, XF)
    big = (C.c_size_t * 65537)(*([160] * 65537))
    tot = (C.c_size_t * 2)()
    assert L.rvc_convert_many_geometry(big, 65537, RATE, K, CTX, XF, None, None, tot) == 5 and M.geometry([160] * 65537, RATE, K, CTX, XF) is None
    assert L.rvc_convert_many_geometry(big, 65536, RATE, K, CTX, XF, None, None, tot) == 0 and list(tot) == [65536, 65536 * 48]
    assert L.rvc_convert_many_geometry(None, 1, RATE, K, CTX, XF, None, None, tot) == 5
    # the geometry errors of one file: k outside [2, 32], context below 3, H < X, the default context in a 63-frame window, rates
    for k, context, crossfade, rate in ((1, 3, 1, 48000), (33, 3, 1, 48000), (16, 2, 1, 48000), (2, 28, 4, 48000), (2, 0, 0, 48000), (16, 3, 1, 48050), (16, 3, 1, 0),
                                        (16, 3, 1, 102400)):
        assert M.geometry([16000, 100], rate, k, context, crossfade) is None and c_geometry([16000, 100], rate, k, context, crossfade)[0] == 5
    # the totals.  2^30 windows is the last count accepted: 65536 files of 2^14 windows, at a rate of 100 (zc = 1) so that the outputs stay under 2^40
    per = 160 * H * (1 << 14)
    rc, g = c_geometry([per] * 65536, 100, K, CTX, XF)
    assert rc == 0 and g["windows_total"] == 1 << 30 and g == M.geometry([per] * 65536, 100, K, CTX, XF)
    assert c_geometry([per] * 65535 + [per + 1], 100, K, CTX, XF)[0] == 5 and M.geometry([per] * 65535 + [per + 1], 100, K, CTX, XF) is None
    frames = (1 << 40) // 480 // 4 + 1                             # four files whose outputs pass 2^40 samples together at 48 kHz
    assert c_geometry([160 * frames] * 4, 48000, 0, 0, 0)[0] == 5 and c_geometry([160 * frames] * 3, 48000, 0, 0, 0)[0] == 0
    assert M.geometry([160 * frames] * 4, 48000, 0, 0, 0) is None


@pytest.mark.parametrize("sola_len,search,frame", [(8, 4, 16), (6, 6, 6)])
def test_numpy_stitch_many_is_the_stitch_per_file(sola_len, search, frame):
    r = np.random.default_rng(77)
    wpf = [1, 3, 1, 2]
    wl = search + frame + sola_len
    y = r.uniform(-1, 1, (sum(wpf), wl))
    # the first window of file 1 repeats file 0's last tail at lag 1: a stitch that carried the tail across the boundary would find it there
    y[1, 1: 1 + sola_len] = y[0, search + frame: search + frame + sola_len]
    # inside file 1, window 2 repeats window 1's tail at lag 2 (window 1 meets the zero tail: offset = search)
    y[2, 2: 2 + sola_len] = y[1, search + frame: search + frame + sola_len]
    audio, off = M.stitch_many(y, wpf, sola_len, search, frame)
    g = 0
    for W in wpf:
        a1, o1 = R.stitch(y[g: g + W], sola_len, search, frame)
        assert np.array_equal(audio[g * frame: (g + W) * frame], a1) and off[g: g + W].tolist() == o1.tolist()
        g += W
    assert off[0] == search and off[1] == search and off[2] == 2      # every file starts from silence: all lags tie, the last wins
    whole, whole_off = R.stitch(y, sola_len, search, frame)
    assert whole_off[1] == 1 and not np.array_equal(whole, audio)     # ... and one chain over all windows is something else
    a2, o2 = M.stitch_many(y, wpf, sola_len, search, frame, offsets=off)
    assert np.array_equal(a2, audio) and o2.tolist() == off.tolist()


def test_convert_dir_parser_and_the_class():
    from obs_rvc_amd.convert_dir import list_wavs, parse_args
    a = parse_args(["in", "-o", "out", "--model", "voice.rvcw"])
    assert (a.input, a.output, a.model, a.version, a.f0, a.index, a.streams, a.window, a.context, a.crossfade, a.highpass, a.rate, a.pitch, a.formant, a.protect,
            a.rms_mix_rate, a.sid, a.sid_mix) == ("in", "out", "voice.rvcw", 2, "rmvpe", None, 8, 0, 0, 0, True, 0, 0.0, 0.0, 0.5, 1.0, None, None)
    a = parse_args(["in", "-o", "out", "--model", "m", "--data", "d", "--version", "1", "--f0", "hybrid[rmvpe+yin]", "--f0-hybrid-mode", "median", "--index", "i.index",
                    "--index-rate", "0.5", "--index-k", "4", "--nprobe", "3", "--pitch", "-7.5", "--formant", "2", "--protect", "0.33", "--sid-mix", "0:1,2:3", "--streams", "32",
                    "--window", "8", "--context", "24", "--crossfade", "4", "--no-highpass", "--rate", "44100", "--rms-mix-rate", "0.25"])
    assert (a.data, a.version, a.f0, a.f0_hybrid_mode, a.index, a.index_rate, a.index_k, a.nprobe, a.pitch, a.formant, a.protect, a.sid_mix, a.streams, a.window, a.context,
            a.crossfade, a.highpass, a.rate, a.rms_mix_rate) == ("d", 1, "hybrid[rmvpe+yin]", "median", "i.index", 0.5, 4, 3, -7.5, 2.0, 0.33, {0: 1.0, 2: 3.0}, 32, 8, 24, 4,
                                                                 False, 44100, 0.25)
    assert parse_args(["in", "-o", "out", "--model", "m", "--sid", "3"]).sid == 3
    base = ["in", "-o", "out", "--model", "m"]
    for bad in (["--auto-pitch", "220"], ["--f0-file", "x"], ["--auto-pitch-from", "ref.wav"], ["--auto-pitch-step", "12"], ["--auto-pitch-limit", "6"], ["--f0-out", "x"],
                ["--analyze-only"], ["--pitch", "25"], ["--formant", "6"], ["--protect", "0.6"], ["--streams", "0"], ["--window", "33"], ["--window", "1"], ["--context", "2"],
                ["--index-k", "5"], ["--f0", "crepe"], ["--rate", "44150"], ["--nprobe", "65"], ["--rms-mix-rate", "1.5"], ["--sid", "1", "--sid-mix", "0:1"], ["--resampler", "device"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    for missing in (["in", "-o", "out"], ["in", "--model", "m"], ["-o", "out", "--model", "m"]):
        with pytest.raises(SystemExit):
            parse_args(missing)
    for name in ("convert_many", "convert_many_info", "sola_stitch_many", "convert_many_geometry"):
        assert callable(getattr(RvcInfer, name))
    # convert's own command line is as it was: it still takes what this one refuses
    from obs_rvc_amd.convert import parse_args as parse_one
    assert parse_one(["in.wav", "-o", "o.wav", "--model", "m", "--auto-pitch", "220"]).auto_pitch == 220.0


def test_convert_dir_lists_wavs_in_sorted_order(tmp_path):
    from obs_rvc_amd.convert_dir import list_wavs
    for f in ("b.wav", "a.WAV", "c.txt", "10.wav", "2.wav"):
        (tmp_path / f).write_bytes(b"")
    (tmp_path / "d.wav").mkdir()
    assert list_wavs(tmp_path) == ["10.wav", "2.wav", "a.WAV", "b.wav"]
