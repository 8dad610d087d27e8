"""Formant shift cost: steady-state GPU ms per chunk (device events around each synchronised chunk, rvc_last_gpu_ms) at 1 and 64 streams,
phi = 0 and phi != 0 alternating in one process, full 48 kHz preset at the 160 ms geometry.  Writes one JSON record.

    python tests/tools/formant_probe.py [--chunks 200] [--warmup 30] [--out profiles/formant_probe.json] [--streams 1,64]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    from common import BASELINE_160MS as g, voice_signal, zoo
    from obs_rvc_amd.rvc import RvcInfer
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--streams", default="1,64")
    ap.add_argument("--phis", default="0,0.07,0,5,0,-5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "formant_probe.json"))
    a = ap.parse_args()
    z = zoo("full")
    rec = {"geometry": "160 ms, return_length %d, full 48 kHz preset" % g.model_return_length, "chunks": a.chunks, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "runs": []}
    for S in [int(v) for v in a.streams.split(",")]:
        eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"])
        if S > 1:
            eng.set_streams(S)
        eng.set_noise_seed(1, 0)
        x = torch.from_numpy(np.stack([voice_signal(g.input_buffer_16k_size, seed=s) for s in range(S)])).cuda()
        cap = g.model_return_size + 64
        out = torch.zeros((S, cap), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for phi in [float(v) for v in a.phis.split(",")]:
            eng.set_formant_shift(phi)
            t0 = time.perf_counter()
            for _ in range(a.warmup):
                eng.infer_device(x.data_ptr(), x.shape[1], g.sample_frame_16k, 12, g.skip_head, g.model_return_length, out.data_ptr(), cap, True)
            warm_s = time.perf_counter() - t0
            ms = []
            for _ in range(a.chunks):
                eng.infer_device(x.data_ptr(), x.shape[1], g.sample_frame_16k, 12, g.skip_head, g.model_return_length, out.data_ptr(), cap, True)
                ms.append(eng.last_gpu_ms())
            ms = np.array(ms)
            r = {"streams": S, "phi": phi, "median_ms": round(float(np.median(ms)), 4), "p10_ms": round(float(np.percentile(ms, 10)), 4),
                 "p90_ms": round(float(np.percentile(ms, 90)), 4), "warmup_s": round(warm_s, 2), "plans": eng.plan_cache_info(),
                 "finite": bool(torch.isfinite(out).all().item())}
            print(json.dumps(r), flush=True)
            rec["runs"].append(r)
        eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
