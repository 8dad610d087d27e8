"""CPU checks of the index builder's pieces that need no GPU: the windowing (tests/index_build_ref.py), the command line's WAV decoding and arguments
(obs_rvc_amd/build_index.py), and the new entry points' presence in the header, the export list and the Rust declarations."""
import fnmatch
import os
import re
import wave

import numpy as np
import pytest

import index_build_ref as B
from common import ROOT
from obs_rvc_amd import _native, build_index as CLI

NAMES = ["rvc_index_build_begin", "rvc_index_build_add", "rvc_index_build_add_device", "rvc_index_build_info", "rvc_index_build_finish", "rvc_index_build_abort"]


def test_frame_rule():
    assert B.frames(399) == 0 and B.frames(400) == 1 and B.frames(719) == 1 and B.frames(720) == 2
    assert B.frames(4000) == 12 and B.frames(48000) == 149 and B.frames(0) == 0
    for L in range(400, 5000, 37):
        assert B.frames(L) == (L - B.RECEPTIVE_FIELD) // B.HOP + 1


@pytest.mark.parametrize("w", [4000, 48000])
def test_windowing_cases(w):
    fw = B.frames(w)
    # below the receptive field: nothing runs, the whole recording is the dropped tail
    assert B.runs(399, w) == ([], 399)
    assert B.runs(0, w) == ([], None)
    # exactly one window, no tail
    assert B.runs(w, w) == ([(0, w, fw)], None)
    # two windows and a tail one sample short of the receptive field: dropped
    assert B.runs(2 * w + 399, w) == ([(0, w, fw), (w, w, fw)], 399)
    # ... exactly at the receptive field: kept, one frame
    assert B.runs(2 * w + 400, w) == ([(0, w, fw), (w, w, fw), (2 * w, 400, 1)], None)
    assert B.total_rows([399, w, 2 * w + 399, 2 * w + 400], w) == 5 * fw + 1


def test_gpu_test_shapes():
    # what tests/test_gpu_index_build.py relies on
    assert B.runs(3 * 4000 + 1500, 4000)[0][-1] == (12000, 1500, 4) and B.runs(4000 + 200, 4000) == ([(0, 4000, 12)], 200)
    assert B.total_rows([13500, 4200], 4000) == 52
    assert B.total_rows([32000, 32000, 32000, 2 * 4000 + 2640], 4000) == 320


def test_rows_of_concatenates_in_time_order():
    x = np.arange(9000, dtype=np.float32)
    seen = []

    def hubert(s):
        seen.append((int(s[0]), len(s)))
        return np.full((1, 3, B.frames(len(s))), s[0], np.float32)
    rows = B.rows_of([x, x[:4100]], 4000, hubert)
    assert seen == [(0, 4000), (4000, 4000), (8000, 1000), (0, 4000)]
    assert rows.shape == (12 + 12 + 2 + 12, 3) and list(rows[:, 0][[0, 12, 24, 26]]) == [0.0, 4000.0, 8000.0, 0.0]


def _write_wav(path, data, rate, width):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if data.ndim == 1 else data.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(data).astype("<i2" if width == 2 else "<i4").tobytes())


def test_wav_decoding(tmp_path):
    g = np.random.default_rng(5)
    m16 = g.integers(-32768, 32768, 1000).astype(np.int64)
    m16[:3] = (-32768, 32767, 0)
    _write_wav(tmp_path / "a16.wav", m16, 16000, 2)
    x, rate = CLI.read_wav(tmp_path / "a16.wav")
    assert rate == 16000 and x.dtype == np.float32 and np.array_equal(x, (m16 / 32768.0).astype(np.float32)) and x[0] == -1.0
    s16 = g.integers(-32768, 32768, (500, 2)).astype(np.int64)
    _write_wav(tmp_path / "b16s.wav", s16, 16000, 2)
    x, rate = CLI.read_wav(tmp_path / "b16s.wav")
    assert rate == 16000 and x.shape == (500,) and np.array_equal(x, ((s16[:, 0] + s16[:, 1]) / 65536.0).astype(np.float32))
    m32 = g.integers(-2 ** 31, 2 ** 31, 700).astype(np.int64)
    m32[:2] = (-2 ** 31, 2 ** 31 - 1)
    _write_wav(tmp_path / "c32.wav", m32, 16000, 4)
    x, rate = CLI.read_wav(tmp_path / "c32.wav")
    assert rate == 16000 and np.array_equal(x, (m32 / 2.0 ** 31).astype(np.float32))
    _write_wav(tmp_path / "d8k.wav", m16[:80], 8000, 2)
    x, rate = CLI.read_wav(tmp_path / "d8k.wav")
    assert rate == 8000 and len(x) == 80
    with wave.open(str(tmp_path / "e8bit.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(1); w.setframerate(16000); w.writeframes(bytes(range(50)))
    with pytest.raises(ValueError):
        CLI.read_wav(tmp_path / "e8bit.wav")
    # a directory names its *.wav entries in name order; a file is taken as it is
    (tmp_path / "notes.txt").write_text("x")
    assert [os.path.basename(f) for f in CLI.wav_files([str(tmp_path), "z.wav"])] == ["a16.wav", "b16s.wav", "c32.wav", "d8k.wav", "e8bit.wav", "z.wav"]


def test_arguments():
    a = CLI.parse_args(["voice", "more.wav", "-o", "added.index"])
    assert a.inputs == ["voice", "more.wav"] and a.output == "added.index" and (a.version, a.window, a.max_rows, a.reduce_to) == (2, 3.0, 0, 0)
    a = CLI.parse_args(["x.wav", "-o", "o.index", "--version", "1", "--window", "1.5", "--max-rows", "5000", "--reduce-to", "300"])
    assert (a.version, a.window, a.max_rows, a.reduce_to) == (1, 1.5, 5000, 300)
    for bad in (["x.wav"], ["-o", "o.index"], ["x.wav", "-o", "o", "--window", "0"], ["x.wav", "-o", "o", "--version", "3"], ["x.wav", "-o", "o", "--max-rows", "-1"]):
        with pytest.raises(SystemExit):
            CLI.parse_args(bad)


def test_new_entry_points_are_declared_everywhere():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rvc_mi355x.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rvc_index_build_[a-z_]+)\s*\(", hdr))
    assert declared == set(NAMES)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "rvc", "src", "ffi.rs")).read()
    # the export list names its globals by pattern: every new name must be matched by one, and by no `local` pattern before it
    emap = re.sub(r"/\*.*?\*/", "", open(os.path.join(_native.CSRC, "exports.map")).read(), flags=re.S)
    globs = [p.strip() for p in re.search(r"global:(.*?)local:", emap, flags=re.S).group(1).split(";") if p.strip()]
    assert globs
    for n in NAMES:
        assert re.search(r"pub fn %s\s*\(" % n, ffi), n
        assert any(fnmatch.fnmatchcase(n, p) for p in globs), n
        assert n in _native.SYMBOLS, n
    dbg = open(os.path.join(ROOT, "include", "rvc_mi355x_debug.h")).read()
    assert "rvc_debug_index_append" in dbg
