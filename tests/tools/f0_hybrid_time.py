#!/usr/bin/env python
"""Hybrid f0 against its members alone on the full-size v2 zoo, same build, same process, the configurations alternating in two rounds
on one engine per stream count: the device time of a chunk (rvc_last_gpu_ms) and its wall time, medians of the timed chunks after warm-up; then the time of
the combine launch alone, with and without the RMVPE decode, between two HIP events (rvc_debug_f0_hybrid).
usage: f0_hybrid_time.py [streams=1,8] [chunks=200]"""
import ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from common import BASELINE_160MS as g, voice_signal, zoo
from obs_rvc_amd import _native, weights as W
from obs_rvc_amd.rvc import RvcInfer

L, chunk, N = g.input_buffer_16k_size, g.sample_frame_16k, g.model_return_size
z = zoo("full", 2)
W.write_fcpe(z["data"], "full"); W.write_crepe(z["data"], "tiny")
CONFIGS = ["rmvpe", "yin", "fcpe", "crepe-tiny", "hybrid[rmvpe+fcpe]", "hybrid[yin+fcpe]", "hybrid[rmvpe+fcpe+crepe-tiny]"]
_FP = C.POINTER(C.c_float)


def run(e, x, o, n):
    gm, wall = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        e.infer_device(x.data_ptr(), L, chunk, 12, g.skip_head, g.model_return_length, o.data_ptr(), N, sync=True)
        wall.append((time.perf_counter() - t0) * 1e3); gm.append(e.last_gpu_ms())
    return float(np.median(gm)), float(np.median(wall))


streams = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "1,8").split(",")]
chunks = int(sys.argv[2]) if len(sys.argv) > 2 else 200
_native.clock_monitor_start(0)
for S in streams:
    x = torch.from_numpy(np.stack([voice_signal(L, seed=1 + s) for s in range(S)])).cuda(); o = torch.empty((S, N), device="cuda")
    e = RvcInfer(z["data"], device=0); e.load_contentvec(2); e.load_model(z["model"]); e.set_streams(S); e.set_noise_seed(1, 0)
    for rnd in range(2):
        for name in CONFIGS:
            e.load_f0_method(name)
            run(e, x, o, 30)
            gpu, wall = run(e, x, o, chunks)
            print("streams %2d round %d  %-30s gpu p50 %8.4f ms   wall p50 %8.4f ms" % (S, rnd, name, gpu, wall), flush=True)
    if S == streams[0]:
        rng = np.random.default_rng(0)
        for B in sorted({1, S}):
            rows = rng.uniform(60, 900, size=(3, B, 32)).astype(np.float32); sal = (0.5 * rng.random((B, 360, 32))).astype(np.float32); sal[:, 100, :] = 0.9          # (the peak well inside the scan range)
            out = np.empty((B, 32), np.float32)
            for what, salp, rm_at in (("combine of 3", None, -1), ("decode + combine of 3", sal.ctypes.data_as(_FP), 0)):
                ms = []
                for _ in range(60):
                    v = C.c_float()
                    assert e._L.rvc_debug_f0_hybrid(e._h, rows.ctypes.data_as(_FP), 3, B, 32, 0, salp, rm_at, out.ctypes.data_as(_FP), None, C.byref(v)) == 0
                    ms.append(v.value)
                print("f0_hybrid_kernel, %d stream(s) x 32 frames, %-22s p50 %.2f us (min %.2f)" % (B, what + ":", 1e3 * np.median(ms[10:]), 1e3 * min(ms[10:])), flush=True)
    e.close()
print("shader clock while timing:", _native.clock_monitor_stop(0))
