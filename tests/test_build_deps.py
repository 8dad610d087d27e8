"""The build's dependency lists (obs_rvc_amd/_native.py: UNITS, SOURCES) are computed from the #include lines of the sources.  Checked here: they agree
with what the compiler reads, and every non-template __global__ function has one home -- a file that exactly one translation unit compiles (hipcc keeps
such a function in the device code of every unit that sees its definition, launched or not).  No GPU and no built library needed."""
from __future__ import annotations

import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from obs_rvc_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# files that are included only under a preprocessor conditional the product flags leave off: the scan takes them always, the compiler only with the flag.
# (None today.)
CONDITIONAL: set = set()


def compiler_deps(src, flags):
    """the files inside the repository that hipcc reads for the host side of csrc/<src>, as paths relative to csrc"""
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "--cuda-host-only", "-MM"] + list(flags) + [os.path.join(_native.CSRC, src)],
                         capture_output=True, text=True, check=True).stdout
    files = out.replace("\\\n", " ").split(":", 1)[1].split()
    real = [os.path.realpath(f) for f in files]
    return {os.path.normpath(os.path.relpath(f, os.path.realpath(_native.CSRC))) for f in real if f.startswith(os.path.realpath(ROOT) + os.sep)}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on PATH")
def test_computed_deps_agree_with_the_compiler():
    units = sorted({(src, tuple(flags)) for src, flags, _ in _native.UNITS})
    computed = {(src, tuple(flags)): set(deps) for src, flags, deps in _native.UNITS}
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        product = list(ex.map(lambda u: compiler_deps(u[0], u[1]), units))
        tuning = list(ex.map(lambda u: compiler_deps(u[0], u[1] + ("-DRVC_TUNING", "-DRVC_KPROBE")), units))
    for u, prod, tune in zip(units, product, tuning):
        have = computed[u]
        assert have == set(_native._include_closure(u[0])), u
        assert prod <= have and tune <= have, (u, (prod | tune) - have)
        assert have - prod <= CONDITIONAL, (u, have - prod)


GLOBAL_DEF = re.compile(r"^[ \t]*(?:static[ \t]+)?__global__\b[^;{]*", re.M)
LAUNCH_ATTR = re.compile(r"__launch_bounds__\s*\((?:[^()]|\([^()]*\))*\)|__attribute__\s*\(\((?:[^()]|\((?:[^()]|\([^()]*\))*\))*\)\)")


def plain_kernels(path):
    """names of the __global__ functions defined in a file whose definition is not preceded by a template<...> line"""
    text = open(path).read()
    names = []
    for m in GLOBAL_DEF.finditer(text):
        before = text[:m.start()].rstrip("\n").rsplit("\n", 1)[-1]
        name = re.search(r"\bvoid\s+(\w+)\s*\(", LAUNCH_ATTR.sub(" ", m.group(0)))
        assert name, (path, m.group(0))
        if not re.match(r"[ \t]*template\s*<", before):
            names.append(name.group(1))
    return names


def test_every_plain_kernel_has_one_home():
    holders = {}
    for dirpath, _, files in os.walk(_native.CSRC):
        for f in files:
            if f.endswith((".hip", ".h", ".cpp")):
                rel = os.path.normpath(os.path.relpath(os.path.join(dirpath, f), _native.CSRC))
                names = plain_kernels(os.path.join(dirpath, f))
                if names:
                    holders[rel] = names
    # the scan sees the kernels: a few that have moved homes, by name
    for f, k in (("plan_ops.hip.h", "gru_multi_kernel"), ("knn.hip.h", "knn_scan_select_kernel"), ("igemm_bf3_inst.hip", "bf3_pack_kernel"),
                 ("protect.hip.h", "protect_mix_kernel"), ("synth.hip.h", "formant_resample_kernel"), ("chunk.hip.h", "post_sola_kernel")):
        assert k in holders.get(f, ()), (f, k)
    assert not any("layernorm_ct_kernel" in v or "igemm_splitk_kernel" in v for v in holders.values())      # templates are not counted
    units = {(src, tuple(flags)): set(deps) for src, flags, deps in _native.UNITS}
    for f, names in holders.items():
        owners = [u for u, deps in units.items() if f in deps]
        assert len(owners) == 1, "%s (%s) is compiled by %d units: %s" % (f, ", ".join(names), len(owners), owners)
    seen = {}
    for f, names in holders.items():
        for k in names:
            assert k not in seen, "%s is defined in %s and in %s" % (k, seen[k], f)
            seen[k] = f
    shared = set(_native._include_closure("engine_int.h")) & set(holders)
    assert not shared, "engine_int.h reaches headers that define kernels: %s" % sorted(shared)


# one header per kernel of the implicit-GEMM family (igemm_common.hip.h holds what they share and defines no kernel)
KERNEL_HEADERS = {"igemm2.hip.h", "igemm2w.hip.h", "igemm_lds.hip.h", "igemm32.hip.h", "igemm_bf3.hip.h", "igemm_splitk.hip.h"}
# the kernel headers each unit may reach: what it instantiates (igemm32l borrows igemm32_kernel's occupancy rule); every unit not listed reaches none
EXPECTED_KERNEL_HEADERS = {"igemm2_inst.hip": {"igemm2.hip.h"}, "igemm2w_inst.hip": {"igemm2w.hip.h"}, "igemm_bf3_inst.hip": {"igemm_bf3.hip.h"},
                           "igemm_tiled_inst.hip": {"igemm_lds.hip.h", "igemm32.hip.h", "igemm_splitk.hip.h"}, "igemm32l_inst.hip": {"igemm32.hip.h"}}
ENGINE_UNITS = ("engine.hip", "retrieval.hip", "calib.hip", "debug.hip", "plan.hip", "model_cv.hip", "model_rmvpe.hip", "model_yin.hip", "model_crepe.hip",
                "model_fcpe.hip", "model_synth.hip")


def test_every_unit_reaches_only_the_kernel_headers_it_instantiates():
    assert not os.path.exists(os.path.join(_native.CSRC, "igemm.hip.h"))          # no umbrella header: it would put the whole closure back
    assert all(os.path.exists(os.path.join(_native.CSRC, h)) for h in KERNEL_HEADERS | {"igemm_common.hip.h"})
    srcs = {src for src, _, _ in _native.UNITS}
    assert set(EXPECTED_KERNEL_HEADERS) <= srcs and set(ENGINE_UNITS) <= srcs and {s for s in srcs if s.startswith("model_")} <= set(ENGINE_UNITS)
    for src, flags, deps in _native.UNITS:
        assert set(deps) & KERNEL_HEADERS == EXPECTED_KERNEL_HEADERS.get(src, set()), (src, flags, sorted(set(deps) & KERNEL_HEADERS))
    for src in ENGINE_UNITS:          # the engine, the planner, the plan builders, retrieval, the calibration and the test hooks launch through igemm_launch.h alone
        assert EXPECTED_KERNEL_HEADERS.get(src, set()) == set()


def test_an_edit_to_one_kernel_header_rebuilds_only_its_units():
    # the object cache is keyed on a unit's flags and the contents of its closure (_native._unit_key): a unit's key changes with a file iff the file is in the closure
    def touched(header):
        return {src for src, _, deps in _native.UNITS if header in deps}
    assert touched("igemm32.hip.h") == {"igemm_tiled_inst.hip", "igemm32l_inst.hip"}
    assert touched("igemm2.hip.h") == {"igemm2_inst.hip"} and touched("igemm2w.hip.h") == {"igemm2w_inst.hip"} and touched("igemm_bf3.hip.h") == {"igemm_bf3_inst.hip"}
    assert touched("igemm_lds.hip.h") == touched("igemm_splitk.hip.h") == {"igemm_tiled_inst.hip"}
    assert touched("igemm_common.hip.h") >= set(ENGINE_UNITS) - {"calib.hip"}
