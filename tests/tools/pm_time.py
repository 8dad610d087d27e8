#!/usr/bin/env python
"""RMVPE, YIN and PM as the engine's f0 method (rvc_load_f0_method) on the full-size v2 zoo, same build, same process: per stream count the device time of
a chunk (rvc_last_gpu_ms) and its wall time (host clock around a synchronous call), 30 warm-up chunks and the median of the timed ones; then, under the test
hook RVC_STAMPS, the section boundaries of the f0 branch and the chunk's last one (device timestamps, us since the chunk's first stamp, medians).
usage: pm_time.py [streams=1,8] [chunks=200]"""
import ctypes, os, sys, time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from common import BASELINE_160MS as g, set_opt, voice_signal, zoo
from obs_rvc_amd import _native
from obs_rvc_amd.rvc import RvcInfer

L, chunk, N = g.input_buffer_16k_size, g.sample_frame_16k, g.model_return_size
z = zoo("full", 2)
METHODS = ("rmvpe", "yin", "pm")


def engine(method, S):
    e = RvcInfer(z["data"], device=0); e.load_contentvec(2); e.load_f0_method(method); e.load_model(z["model"]); e.set_streams(S); e.set_noise_seed(1, 0)
    return e


def run(e, x, o, n, stamps=None):
    gm, wall = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        e.infer_device(x.data_ptr(), L, chunk, 12, g.skip_head, g.model_return_length, o.data_ptr(), N, sync=True)
        wall.append((time.perf_counter() - t0) * 1e3); gm.append(e.last_gpu_ms())
        if stamps is not None:
            buf = ctypes.create_string_buffer(1 << 16)
            e._L.rvc_debug_stamps(e._h, buf, len(buf))
            seen = {}
            for ln in buf.value.decode().splitlines():
                name, t = ln.rsplit(" ", 1)
                k = seen.get(name, 0); seen[name] = k + 1
                stamps.setdefault("%s#%d" % (name, k), []).append(float(t))
    return float(np.median(gm)), float(np.median(wall))


def inputs(S):
    return torch.from_numpy(np.stack([voice_signal(L, seed=1 + s) for s in range(S)])).cuda(), torch.empty((S, N), device="cuda")


streams = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "1,8").split(",")]
chunks = int(sys.argv[2]) if len(sys.argv) > 2 else 200
assert chunks >= 200, "medians of at least 200 chunks"
_native.clock_monitor_start(0)
for S in streams:
    x, o = inputs(S)
    for rnd in range(2):
        for method in METHODS:
            e = engine(method, S)
            run(e, x, o, 30)
            gpu, wall = run(e, x, o, chunks)
            print("streams %2d round %d  %-6s gpu p50 %8.4f ms   wall p50 %8.4f ms" % (S, rnd, method, gpu, wall), flush=True)
            e.close()
print("shader clock while timing:", _native.clock_monitor_stop(0))
set_opt("RVC_STAMPS", "1")          # test hook (rvc_debug_option): device timestamps at the section boundaries
_native.lib().rvc_debug_stamps.restype = ctypes.c_int
_native.lib().rvc_debug_stamps.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
for S in streams:
    x, o = inputs(S)
    for method in METHODS:
        e = engine(method, S)
        run(e, x, o, 30)
        st = {}
        run(e, x, o, chunks, st)
        keys = [k for k in st if k.split(".")[0] in ("rm", "yin", "pm", "f0")] + [k for k in st if k.startswith("sy.audio")]
        print("streams %2d %-6s stamps (us since the first stamp, p50): %s" % (S, method, "  ".join("%s %.1f" % (k, np.median(st[k])) for k in keys)), flush=True)
        e.close()
set_opt("RVC_STAMPS", None)
