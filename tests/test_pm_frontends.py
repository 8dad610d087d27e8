"""The PM f0 method in the front ends, no GPU: the constant agrees between the C header, rvc_common.py and the Rust binding; the name "pm" is offered by the
Python engine class and the file converter's --f0, alone and as a hybrid member; "harvest" is still refused."""
from __future__ import annotations

import os
import re

import pytest

from obs_rvc_amd import rvc_common
from obs_rvc_amd.convert import F0_CHOICES, parse_args
from obs_rvc_amd.rvc_common import parse_f0_hybrid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_the_constant_agrees_everywhere():
    header = dict((k, int(v)) for k, v in re.findall(r"^#define\s+(RVC_F0_\w+)\s+(\d+)", _read("include", "rvc_mi355x.h"), re.M))
    ffi = dict((k, int(v)) for k, v in re.findall(r"pub const (RVC_F0_\w+): c_int = (\d+);", _read("bindings", "rust", "rvc", "src", "ffi.rs")))
    assert header["RVC_F0_PM"] == 9 == rvc_common.F0_PM
    assert header == {k: v for k, v in ffi.items() if k != "RVC_F0_NOT_LOADED"}          # (a status code of the same prefix, no method)
    assert header == {"RVC_F0_" + k[3:]: v for k, v in vars(rvc_common).items() if k.startswith("F0_")}
    assert sorted(header.values()) == [1, 2, 4, 5, 7, 8, 9]          # 3 and 6 stay "not a method", 8 the hybrid
    assert "RVC_F0_PM" in _read("bindings", "rust", "rvc", "src", "rvc.rs")
    assert _read("obs_rvc_amd", "csrc", "engine.hip").count("or RVC_F0_PM") >= 3          # the messages that list the methods


def test_the_engine_class_knows_the_name():
    from obs_rvc_amd.rvc import RvcInfer
    assert RvcInfer._F0_NAMES["pm"] == 9
    assert parse_f0_hybrid("hybrid[pm+rmvpe]", RvcInfer._F0_NAMES) == ["pm", "rmvpe"]
    assert RvcInfer._hybrid_args(["pm", "rmvpe"], "vote") == ([9, 1], 0)
    assert RvcInfer._hybrid_args([9, "yin", "fcpe", "crepe-tiny"], "median") == ([9, 2, 7, 5], 1)
    with pytest.raises(ValueError):
        RvcInfer._hybrid_args(["pm", "harvest"], "vote")


def test_the_converter_accepts_pm():
    base = ["in.wav", "-o", "o.wav", "--model", "m"]
    assert "pm" in F0_CHOICES and "harvest" not in F0_CHOICES
    assert parse_args(base + ["--f0", "pm"]).f0 == "pm"
    assert parse_args(base + ["--f0", "hybrid[pm+rmvpe]"]).f0 == "hybrid[pm+rmvpe]"
    assert parse_args(base + ["--f0", "Hybrid[ PM + yin ]", "--f0-hybrid-mode", "median"]).f0 == "hybrid[pm+yin]"
    for bad in ("harvest", "hybrid[pm+harvest]", "hybrid[pm+pm]", "praat"):
        with pytest.raises(SystemExit):
            parse_args(base + ["--f0", bad])
