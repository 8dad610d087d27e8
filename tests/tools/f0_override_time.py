#!/usr/bin/env python
"""The cost of an override plan over the plain plan on the full-size v2 zoo, same build, same process: per stream count and f0 method the
device time of a chunk (rvc_last_gpu_ms), 30 warm-up chunks and the median of the timed ones, (a) no override set, (b) a held override of the whole window on
every stream, (c) new override values in front of every chunk (the block travels every chunk); the legs alternate in two rounds.
usage: f0_override_time.py [streams=1,8] [chunks=200]"""
import os, sys
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from common import BASELINE_160MS as g, voice_signal, zoo
from obs_rvc_amd import _native
from obs_rvc_amd.rvc import RvcInfer

L, chunk, N, TM = g.input_buffer_16k_size, g.sample_frame_16k, g.model_return_size, 32
z = zoo("full", 2)


def run(e, S, x, o, n, leg):
    gm = []
    for k in range(n):
        if leg == "fresh":
            for s in range(S):
                e.set_f0_override(s, np.full(TM, 150.0 + (k % 50) + s, np.float32))
        e.infer_device(x.data_ptr(), L, chunk, 12, g.skip_head, g.model_return_length, o.data_ptr(), N, sync=True)
        gm.append(e.last_gpu_ms())
    return float(np.median(gm))


streams = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "1,8").split(",")]
chunks = int(sys.argv[2]) if len(sys.argv) > 2 else 200
assert chunks >= 200, "medians of at least 200 chunks"
_native.clock_monitor_start(0)
for S in streams:
    x = torch.from_numpy(np.stack([voice_signal(L, seed=1 + s) for s in range(S)])).cuda(); o = torch.empty((S, N), device="cuda")
    for method in ("yin", "rmvpe"):
        e = RvcInfer(z["data"], device=0); e.load_contentvec(2); e.load_f0_method(method); e.load_model(z["model"]); e.set_streams(S); e.set_noise_seed(1, 0)
        for rnd in range(2):
            for leg in ("none", "held", "fresh"):
                e.set_f0_override_hold(leg == "held")
                for s in range(S):
                    e.set_f0_override(s, np.full(TM, 200.0, np.float32) if leg == "held" else None)
                run(e, S, x, o, 30, leg)
                print("streams %2d %-6s round %d  %-5s gpu p50 %8.4f ms" % (S, method, rnd, leg, run(e, S, x, o, chunks, leg)), flush=True)
        e.close()
print("shader clock while timing:", _native.clock_monitor_stop(0))
