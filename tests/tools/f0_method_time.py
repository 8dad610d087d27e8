#!/usr/bin/env python
"""RMVPE against YIN as the engine's f0 method (rvc_load_f0_method) on the full-size v2 zoo, same build, same process: per stream count the device
time of a chunk (rvc_last_gpu_ms) and its wall time (host clock around a synchronous call), medians of the timed chunks after warm-up, the two methods
alternating in two rounds; at up to 4 streams also YIN with ContentVec on every CU instead of its partition (test hook RVC_YIN_CV_ALL_CUS).
usage: f0_method_time.py [streams=1,8,64] [chunks=200]
       f0_method_time.py --kernel STREAMS      30 YIN chunks and nothing else: the run to put behind `rocprofv3 --kernel-trace --stats -d DIR --`
                                               (the time of yin_f0_kernel and pitch_post_kernel is in DIR's *_kernel_stats.csv)"""
import os, sys, time
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


def engine(method, S):
    e = RvcInfer(z["data"], device=0); e.load_contentvec(2); e.load_f0_method(method); e.load_model(z["model"]); e.set_streams(S); e.set_noise_seed(1, 0)
    return e


def run(e, x, o, n):
    gm, wall = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        e.infer_device(x.data_ptr(), L, chunk, 12, g.skip_head, g.model_return_length, o.data_ptr(), N, sync=True)
        wall.append((time.perf_counter() - t0) * 1e3); gm.append(e.last_gpu_ms())
    return float(np.median(gm)), float(np.median(wall))


def inputs(S):
    return torch.from_numpy(np.stack([voice_signal(L, seed=1 + s) for s in range(S)])).cuda(), torch.empty((S, N), device="cuda")


if len(sys.argv) > 2 and sys.argv[1] == "--kernel":
    S = int(sys.argv[2])
    x, o = inputs(S)
    e = engine("yin", S)
    run(e, x, o, 30)
    e.close()
    sys.exit(0)

streams = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "1,8,64").split(",")]
chunks = int(sys.argv[2]) if len(sys.argv) > 2 else 200
assert chunks >= 200, "medians of at least 200 chunks"
_native.clock_monitor_start(0)
for S in streams:
    x, o = inputs(S)
    cases = [("rmvpe", "rmvpe", None), ("yin", "yin", None)] + ([("yin, ContentVec on every CU", "yin", "1")] if S <= 4 else [])
    for rnd in range(2):
        for name, method, hook in cases:
            set_opt("RVC_YIN_CV_ALL_CUS", hook)
            e = engine(method, S)
            run(e, x, o, 30)
            gpu, wall = run(e, x, o, chunks)
            print("streams %2d round %d  %-28s gpu p50 %8.4f ms   wall p50 %8.4f ms" % (S, rnd, name, gpu, wall), flush=True)
            e.close()
    set_opt("RVC_YIN_CV_ALL_CUS", None)
print("shader clock while timing:", _native.clock_monitor_stop(0))
