"""f0 from outside in every front end: the five entry points in the header, the export map, the Rust declarations and the Python
loader; the converter's --f0-file / --f0-out and its curve-file parser; and no new f0 method.  No GPU and no library load."""
from __future__ import annotations

import fnmatch
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rvc_set_f0_override_stream", "rvc_set_f0_override_hold", "rvc_set_f0_curve", "rvc_f0_curve_grid", "rvc_convert_f0")


def _read(*p):
    with open(os.path.join(ROOT, *p)) as fh:
        return fh.read()


def test_the_five_names_everywhere():
    from obs_rvc_amd import _native
    hdr, ffi, rs = _read("include", "rvc_mi355x.h"), _read("bindings", "rust", "rvc", "src", "ffi.rs"), _read("bindings", "rust", "rvc", "src", "rvc.rs")
    globs = re.findall(r"global:\s*([^;]+);", _read("obs_rvc_amd", "csrc", "exports.map"))
    pats = [g.strip() for s in globs for g in s.split()]
    for n in NAMES:
        assert re.search(r"^rvc_status %s\(rvc_engine \*e" % n, hdr, re.M), n
        assert re.search(r"pub fn %s\(e: \*mut RvcEngine" % n, ffi), n
        assert "ffi::%s(" % n in rs, n
        assert n in _native.SYMBOLS, n
        assert any(fnmatch.fnmatchcase(n, p) for p in pats), (n, pats)
    assert "rvc_debug_f0_override(" in _read("include", "rvc_mi355x_debug.h")
    from obs_rvc_amd.rvc import RvcInfer
    for m in ("set_f0_override", "set_f0_override_hold", "set_f0_curve", "clear_f0_curve", "convert_f0"):
        assert callable(getattr(RvcInfer, m)), m


def test_converter_flags(tmp_path):
    from obs_rvc_amd.convert import parse_args
    base = ["in.wav", "-o", "out.wav", "--model", "m.rvcw"]
    a = parse_args(base)
    assert a.f0_file is None and a.f0_out is None and a.f0_curve is None
    f = tmp_path / "curve.txt"
    f.write_text("# a take\n0.10,220\n\n0.25, 0   # unvoiced\n0.5,233.5\n")
    a = parse_args(base + ["--f0-file", str(f), "--f0-out", str(tmp_path / "o.txt")])
    assert a.f0_out == str(tmp_path / "o.txt")
    t, hz = a.f0_curve
    assert t.dtype == np.float64 and hz.dtype == np.float32
    assert np.array_equal(t, [0.10, 0.25, 0.5]) and np.array_equal(hz, np.float32([220, 0, 233.5]))
    f.write_text("0.1,220\n0.2;230\n")
    with pytest.raises(SystemExit):
        parse_args(base + ["--f0-file", str(f)])
    with pytest.raises(SystemExit):
        parse_args(base + ["--f0-file", str(tmp_path / "missing.txt")])


def test_curve_file_parser():
    from obs_rvc_amd.convert import format_f0_curve, parse_f0_curve
    t, hz = parse_f0_curve("0,100\n0.01,0\n")
    assert np.array_equal(t, [0.0, 0.01]) and np.array_equal(hz, [100.0, 0.0])
    for text, line in (("0,100\nx,1\n", 2), ("0,100\n\n# c\n0.1,2,3\n", 4), ("0.2,100\n0.2,110\n", 2), ("0.2,100\n0.1,110\n", 2), ("0,-1\n", 1), ("0,20001\n", 1),
                       ("0,nan\n", 1), ("inf,1\n", 1), ("0,100\n0.5\n", 2)):
        with pytest.raises(ValueError) as ei:
            parse_f0_curve(text)
        assert "line %d" % line in str(ei.value), (text, str(ei.value))
    with pytest.raises(ValueError):
        parse_f0_curve("# nothing\n\n")
    # what --f0-out writes is what --f0-file reads: the same float32 values on the frames' times
    f0 = np.float32([0.0, 123.456789, 440.0, 1e-3, 20000.0, 0.0, 99.99999])
    t, hz = parse_f0_curve(format_f0_curve(f0))
    assert np.array_equal(hz, f0) and np.allclose(t, np.arange(len(f0)) / 100.0, rtol=0, atol=1e-12)
    # ... and is always a file the parser accepts: no number or negative -> 0, above 20000 (a transposed value) -> 20000
    t, hz = parse_f0_curve(format_f0_curve(np.float32([np.nan, -1.0, 5e4, np.inf, -np.inf, 100.0])))
    assert np.array_equal(hz, np.float32([0.0, 0.0, 20000.0, 20000.0, 0.0, 100.0]))


def test_no_new_f0_method():
    from obs_rvc_amd import rvc_common
    from obs_rvc_amd.convert import F0_CHOICES
    from obs_rvc_amd.rvc import RvcInfer
    want = {"RVC_F0_RMVPE": 1, "RVC_F0_YIN": 2, "RVC_F0_CREPE": 4, "RVC_F0_CREPE_TINY": 5, "RVC_F0_FCPE": 7, "RVC_F0_HYBRID": 8, "RVC_F0_PM": 9}
    hdr = dict((k, int(v)) for k, v in re.findall(r"^\s*(RVC_F0_[A-Z_]+)\s*=\s*(\d+)", _read("include", "rvc_mi355x.h"), re.M))
    hdr.update((k, int(v)) for k, v in re.findall(r"#define\s+(RVC_F0_[A-Z_]+)\s+(\d+)", _read("include", "rvc_mi355x.h")))
    hdr.pop("RVC_F0_NOT_LOADED", None)
    ffi = dict((k, int(v)) for k, v in re.findall(r"pub const (RVC_F0_\w+): c_int = (\d+);", _read("bindings", "rust", "rvc", "src", "ffi.rs")))
    ffi.pop("RVC_F0_NOT_LOADED", None)
    assert hdr == want and ffi == want, (hdr, ffi)
    assert F0_CHOICES == ("rmvpe", "yin", "crepe-full", "crepe-tiny", "fcpe", "pm")
    assert sorted(RvcInfer._F0_NAMES) == sorted(["rmvpe", "yin", "crepe", "crepe-full", "crepe-tiny", "fcpe", "pm"])
    assert "harvest" not in RvcInfer._F0_NAMES and not hasattr(rvc_common, "F0_HARVEST")
