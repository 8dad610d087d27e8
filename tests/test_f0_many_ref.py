"""tests/f0_many_ref.py against tests/convert_many_ref.py, tests/f0_stats_ref.py and first principles, and the front ends of the per-file pitch of
rvc_convert_many: convert_dir's flags and list file, the entry points in header, export map, ffi.rs and _native.py.  No GPU."""
from __future__ import annotations

import fnmatch
import math
import os
import re

import numpy as np
import pytest

import convert_many_ref as M
import convert_ref as R
import f0_many_ref as FM
import f0_stats_ref as S
from common import ROOT

H = 54
LENGTHS = [1, 320 * H + 1, 160 * H, 160 * H + 1]
NEW = ("rvc_analyze_f0_many", "rvc_f0_stats_many", "rvc_set_convert_many_pitch", "rvc_set_convert_many_auto_transpose", "rvc_convert_many_auto_transpose",
       "rvc_convert_many_pitch_info")


def test_self_checks():
    FM.self_check()
    M.self_check()


@pytest.mark.parametrize("geo", [(4800, 2, 3, 2), (16000, 2, 28, 3), (48000, 0, 0, 0)])
def test_export_is_the_single_file_export_per_file(geo):
    rate, k, C, X = geo
    hop = R.geometry(1, rate, k, C, X)["hop"]
    r = np.random.default_rng(hop)
    for lengths in (LENGTHS if hop == H else [1, 320 * hop + 1, 160 * hop, 160 * hop + 1], [160 * hop * 3 + 7], [int(v) for v in r.integers(1, 160 * hop * 4, 9)]):
        g = M.geometry(lengths, rate, k, C, X)
        off = FM.grid_offsets(lengths)
        assert [off[f + 1] - off[f] for f in range(len(lengths))] == [o // (rate // 100) for o in g["output_samples"]]      # Nf_f = out_f / zc
        emap = FM.export_map(lengths, rate, k, C, X)
        assert emap.shape == (g["windows_total"], hop)
        # every arena row is written exactly once, and the regions tile the arena
        assert sorted(emap[emap >= 0].tolist()) == list(range(off[-1]))
        # a window's rows are those the packing gives it: global g = (f, w) in convert_many_ref's order writes rows [w H, min((w + 1) H, Nf_f)) of file f
        order = [p for b in M.packing(g["windows"], 3) for p in b]
        for gi, (f, w) in enumerate(order):
            nf = off[f + 1] - off[f]
            want = [off[f] + w * hop + h if w * hop + h < nf else -1 for h in range(hop)]
            assert emap[gi].tolist() == want, (gi, f, w)
        # scatter = the single-file export of each file: row j of file f is hop row j % H of its window j // H
        rows = r.uniform(50, 500, (g["windows_total"], hop)).astype(np.float32)
        got = FM.scatter(lengths, rows, rate, k, C, X)
        P = np.concatenate([[0], np.cumsum(g["windows"])])
        for f, n in enumerate(lengths):
            nf = -(-n // 160)
            want = np.array([rows[P[f] + j // hop, j % hop] for j in range(nf)], np.float32)
            assert np.array_equal(got[f], want), f
        # the gate: a skipped window leaves zeros, its neighbours' rows are untouched
        active = [gi % 3 != 1 for gi in range(g["windows_total"])]
        gated = FM.scatter(lengths, rows, rate, k, C, X, active=active)
        for f in range(len(lengths)):
            for j in range(off[f + 1] - off[f]):
                assert gated[f][j] == (got[f][j] if active[P[f] + j // hop] else 0.0)


def test_segmented_select_is_the_select_per_segment():
    r = np.random.default_rng(3)
    segs = [S.select_inputs(n, seed=i)[name] for i, (n, name) in enumerate(((1, "one voiced row"), (2, "all unvoiced"), (255, "NaN, +inf and negative rows"),
                                                                            (257, "two values one ulp apart"), (1000, "log-uniform 50-1100 Hz, 40 % zeros")))]
    out, v = FM.select_many(segs, S.QUANTILES)
    assert out.shape == (5, 5) and out.dtype == np.float32
    for f, x in enumerate(segs):
        q, vv = S.select(x, S.QUANTILES)
        assert np.array_equal(out[f].view(np.uint32), q.view(np.uint32)) and v[f] == vv
    assert v[1] == 0 and not np.any(out[1]) and v[0] == 1
    # a segment's answer does not depend on its neighbours
    out2, v2 = FM.select_many([segs[3], r.uniform(1, 2, 77).astype(np.float32), segs[0]], (0.5,))
    assert out2[0, 0] == S.select(segs[3])[0][0] and out2[2, 0] == np.float32(220.5)


def test_per_file_semitone_rule():
    med, voiced = np.float32([0.0, 110.0, 165.0, 370.0]), [0, 100, 50, 20]
    a, t = FM.file_semitones(None, 220.0, med, voiced, step=0, limit=24.0)
    assert a[0] == 0.0 and a[1] == 12.0 and a[2] == 12.0 * math.log2(220.0 / 165.0) and a[3] == 12.0 * math.log2(220.0 / 370.0) and np.array_equal(a, t)
    a, t = FM.file_semitones([0, 3, -5, 12], 220.0, med, voiced, step=12, limit=24.0)
    assert a.tolist() == [0.0, 12.0, 0.0, -12.0] and t.tolist() == [0.0, 15.0, -5.0, 0.0]
    a, t = FM.file_semitones([1, 0, 0, 0], 220.0, med, voiced, step=1, limit=2.0)
    assert a.tolist() == [0.0, 2.0, 2.0, -2.0] and t[0] == 1.0          # the clamp acts on a_f alone; an unvoiced file keeps its listed value
    a, t = FM.file_semitones([0, 3, -5, 12], 0.0, med, voiced)           # the target off: the list alone
    assert not np.any(a) and t.tolist() == [0.0, 3.0, -5.0, 12.0]
    assert FM.check_pitch_list([0, -24, 24, 3.5]) and not FM.check_pitch_list([0, 24.5]) and not FM.check_pitch_list([float("nan")]) and not FM.check_pitch_list([-np.inf])
    # which stream takes which transpose: W = {1, 3, 1, 2}
    assert FM.stream_semitones([1, 3, 1, 2], 3, t) == [[0.0, 3.0, 3.0], [3.0, -5.0, 12.0], [12.0, 0.0, 0.0]]
    assert FM.stream_semitones([1, 3, 1, 2], 1, t) == [[0.0], [3.0], [3.0], [3.0], [-5.0], [12.0], [12.0]]
    assert S.factor(0.0) is None                                          # t_f = 0 multiplies by nothing


def test_convert_dir_takes_the_per_file_flags_and_keeps_its_refusals():
    from obs_rvc_amd.convert_dir import parse_args, parse_each_pitch
    base = ["in", "-o", "out", "--model", "m"]
    a = parse_args(base)
    assert (a.each_pitch, a.each_auto_pitch, a.each_auto_pitch_from, a.each_auto_pitch_step, a.each_auto_pitch_limit, a.each_f0_out, a.each_analyze_only) == \
        (None, 0.0, None, 1, 12.0, None, False)
    a = parse_args(base + ["--each-auto-pitch", "255", "--each-auto-pitch-step", "12", "--each-auto-pitch-limit", "24", "--each-pitch", "p.csv", "--each-f0-out", "f0"])
    assert (a.each_auto_pitch, a.each_auto_pitch_step, a.each_auto_pitch_limit, a.each_pitch, a.each_f0_out) == (255.0, 12, 24.0, "p.csv", "f0")
    assert parse_args(base + ["--each-auto-pitch-from", "ref.wav", "--each-auto-pitch-step", "0"]).each_auto_pitch_from == "ref.wav"
    a = parse_args(["in", "--each-analyze-only", "--each-f0-out", "f0", "--f0", "yin"])
    assert a.each_analyze_only and a.model is None and a.output is None
    for bad in (["--each-auto-pitch-step", "2"], ["--each-auto-pitch", "-1"], ["--each-auto-pitch", "20001"], ["--each-auto-pitch-limit", "24.5"],
                ["--each-auto-pitch-limit", "-1"], ["--each-auto-pitch", "155", "--each-auto-pitch-from", "ref.wav"], ["--each-analyze-only"], ["--each-auto"], ["--each-f0"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    with pytest.raises(SystemExit):
        parse_args(["in", "--each-analyze-only"])
    # every old refusal still raises, and a conversion still needs both -o and --model
    for bad in (["--auto-pitch", "220"], ["--f0-file", "x"], ["--auto-pitch-from", "ref.wav"], ["--auto-pitch-step", "12"], ["--auto-pitch-limit", "6"], ["--f0-out", "x"],
                ["--analyze-only"], ["--pitch", "25"], ["--resampler", "device"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    for missing in (["in", "-o", "out"], ["in", "--model", "m"], ["-o", "out", "--model", "m"], ["in", "--each-f0-out", "f0"]):
        with pytest.raises(SystemExit):
            parse_args(missing)
    # the list file
    names = ["a.wav", "b.WAV", "c d.wav"]
    assert parse_each_pitch("", names) == [0.0, 0.0, 0.0]
    assert parse_each_pitch("# speaker 1\nb.WAV, 3.5\n\nc d,-12  # by stem\n", names) == [0.0, 3.5, -12.0]
    for bad in ("x.wav,1", "a.wav", "a.wav,abc", "a.wav,25", "a.wav,1\na,2", "a.wav,nan"):
        with pytest.raises(ValueError):
            parse_each_pitch(bad, names)


def test_every_front_end_declares_the_entry_points():
    from obs_rvc_amd import _native
    from obs_rvc_amd.rvc import RvcInfer
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    hdr = re.sub(r"/\*.*?\*/", "", read("include", "rvc_mi355x.h"), flags=re.S)
    ffi = read("bindings", "rust", "rvc", "src", "ffi.rs")
    globs = [g.strip() for part in re.findall(r"global:\s*([^;]+);", read("obs_rvc_amd", "csrc", "exports.map")) for g in part.split()]
    for name in NEW:
        assert name in _native.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr) and re.search(r"pub fn %s\s*\(" % name, ffi), name
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), name
    for method in ("analyze_f0_many", "f0_stats_many", "set_convert_many_pitch", "set_convert_many_auto_transpose", "convert_many_auto_transpose", "convert_many_pitch_info"):
        assert callable(getattr(RvcInfer, method)), method
    # the segmented select sums integers only, as the kernel beside it: no float type in its body but the quantile itself; its loads are scalar
    src = read("obs_rvc_amd", "csrc", "f0_select_many.hip.h")
    body = src[src.index("void f0_select_many_kernel"):src.index("// one select per file")]
    assert "float" not in body and body.count("double") == 1 and "atomicAdd" in body and "uint4" not in body
    # ... and the existing kernel is as it was: its header does not mention the new one
    assert "f0_select_many" not in read("obs_rvc_amd", "csrc", "f0_select.hip.h")
