"""The silence gate's definition (tests/silence_ref.py) on the CPU: its own invariants on random loud / silent patterns, the front ends'
flags and the agreement of header, Python binding and Rust ffi on the four entry points."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import silence_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def patterns():
    r = np.random.default_rng(2025)
    for trial in range(300):
        nf = int(r.integers(1, 700))
        loud = np.zeros(nf, bool)
        for _ in range(int(r.integers(0, 6))):                      # a few stretches of sound, some of one frame
            a = int(r.integers(0, nf)); loud[a: a + int(r.integers(1, 40))] = True
        k = int(r.integers(2, 6)); X = int(r.integers(1, 6)); C = int(r.integers(3, 8))
        H = S.hop(k, C, X)
        if H < X:
            continue
        yield loud, int(r.choice([0, 1, 5, 30, 60, 1000])), H, X


def test_loud_frames_are_the_gate_measure():
    r = np.random.default_rng(1)
    x = (0.02 * r.standard_normal(160 * 50 + 37)).astype(np.float32)
    x[160 * 20: 160 * 30] = 0.0
    e = S.frame_energy(x)
    pad = np.concatenate([x.astype(np.float64), np.zeros(640)])
    for i in (0, 19, 20, 26, 27, 49, 50):
        seg = pad[160 * i: 160 * i + 640]
        assert abs(e[i] - float(np.sum(seg * seg))) <= 1e-12 * max(e[i], 1e-30)
        rms_db = 20.0 * np.log10(max(np.sqrt(np.mean(seg * seg)), 1e-5))
        assert bool(S.loud_frames(x, -40.0)[i]) == bool(rms_db >= -40.0)
    assert len(e) == 51 and S.n_frames(1) == 1 and S.n_frames(160) == 1 and S.n_frames(161) == 2
    assert S.threshold_linear(-200.0) == 640.0 * 1e-10 and not S.loud_frames(np.zeros(500, np.float32), -59.0).any()


def test_kept_is_the_dilation():
    for loud, hang, H, X in patterns():
        kept = S.kept_frames(loud, hang)
        want = np.array([loud[max(i - hang, 0): i + hang + 1].any() for i in range(len(loud))])
        assert np.array_equal(kept, want)


def test_invariants_of_the_window_map():
    seen_skip = 0
    for loud, hang, H, X in patterns():
        m = S.analyze_flags(loud, hang, H, X)
        kept, act, place = m["kept"], m["active"], m["place"]
        nf, W, R = len(loud), len(act), H + X + S.Q
        assert W == -(-nf // H)
        # place: a bijection of the active windows onto 0 .. A - 1, in order
        A = int(act.sum())
        assert place[act].tolist() == list(range(A)) and (place[~act] == -1).all()
        for w in range(W):
            # 1. a kept frame among a window's first X + Q frames: the window before returns those frames too, so it is active -- an onset is never faded in from zeros
            if w > 0 and kept[w * H: min(w * H + X + S.Q, nf)].any():
                assert act[w - 1] and act[w]
            # 2. a skipped window behind an active one: the frames it shares with it -- where the active window's tail fades to zero -- and all of its own frames
            # are at least hang + 1 away from anything loud
            if not act[w]:
                seen_skip += 1
                lo, hi = max(w * H - hang, 0), min(w * H + R, nf) + hang
                assert not loud[lo: hi].any()
    assert seen_skip > 100


def test_insert_zero_windows():
    y = np.arange(6, dtype=np.float32).reshape(2, 3) + 1
    out = S.insert_zero_windows(y, [-1, 0, -1, -1, 1], 3)
    assert out.tolist() == [[0, 0, 0], [1, 2, 3], [0, 0, 0], [0, 0, 0], [4, 5, 6]]
    assert S.insert_zero_windows(np.zeros((0, 3), np.float32), [-1, -1], 3).tolist() == [[0, 0, 0], [0, 0, 0]]


def test_argument_checks_and_flags():
    assert S.check_args(-40.0, 0) and S.check_args(-60.0, 1000) and S.check_args(-200.0, 30)
    for bad in ((float("nan"), 5), (-40.0, -1), (-40.0, 1001)):
        assert not S.check_args(*bad)
    assert not S.is_on(-60.0) and not S.is_on(-75.0) and S.is_on(-59.9)
    from obs_rvc_amd.convert import SILENCE_HANG_DEFAULT, parse_args
    from obs_rvc_amd.convert_dir import parse_args as parse_dir
    base = ["in.wav", "-o", "out.wav", "--model", "m.rvcw"]
    a = parse_args(base)
    assert a.skip_silence is None and a.silence_hang == SILENCE_HANG_DEFAULT == 30
    a = parse_args(base + ["--skip-silence", "-45", "--silence-hang", "12"])
    assert (a.skip_silence, a.silence_hang) == (-45.0, 12)
    assert parse_args(base + ["--skip-silence=-50"]).silence_hang == 30
    a = parse_args(["in.wav", "--analyze-only", "--f0-out", "f0.csv", "--skip-silence", "-40"])
    assert a.analyze_only and a.skip_silence == -40.0
    d = ["in", "-o", "out", "--model", "m.rvcw"]
    assert parse_dir(d).skip_silence is None and parse_dir(d + ["--skip-silence", "-45", "--silence-hang", "0"]).silence_hang == 0
    for parse, args in ((parse_args, base), (parse_dir, d)):
        for bad in (["--silence-hang", "5"], ["--skip-silence", "-60"], ["--skip-silence", "-80"], ["--skip-silence", "3"], ["--skip-silence", "nan"],
                    ["--skip-silence", "-40", "--silence-hang", "-1"], ["--skip-silence", "-40", "--silence-hang", "1001"], ["--skip-silence", "loud"]):
            with pytest.raises(SystemExit):
                parse(args + bad)


def test_error_texts(capsys):
    from obs_rvc_amd.convert import parse_args
    base = ["in.wav", "-o", "out.wav", "--model", "m.rvcw"]
    for bad, text in ((["--silence-hang", "5"], "--silence-hang goes with --skip-silence"), (["--skip-silence", "-60"], "--skip-silence is a level in dB above -60"),
                      (["--skip-silence", "-40", "--silence-hang", "1001"], "--silence-hang is 0..1000 frames")):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
        assert text in capsys.readouterr().err


def test_every_front_end_declares_the_entry_points():
    from obs_rvc_amd import _native
    from obs_rvc_amd.rvc import RvcInfer
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    hdr = re.sub(r"/\*.*?\*/", "", read("include", "rvc_mi355x.h"), flags=re.S)
    ffi = read("bindings", "rust", "rvc", "src", "ffi.rs")
    count = lambda text: 0 if not text.strip() else len([a for a in text.split(",") if a.strip()])
    for name, nargs in (("rvc_set_convert_silence", 3), ("rvc_convert_silence", 3), ("rvc_convert_silence_info", 6), ("rvc_silence_map", 15)):
        h = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S)
        r = re.search(r"pub fn %s\s*\((.*?)\)\s*->" % name, ffi, flags=re.S)
        assert name in _native.SYMBOLS and h and r, name
        assert count(h.group(1)) == count(r.group(1)) == nargs, name
    for method in ("set_convert_silence", "convert_silence", "convert_silence_info", "silence_map"):
        assert callable(getattr(RvcInfer, method)), method
