#!/usr/bin/env python
"""What consonant protection (rvc_set_protect; protect.hip.h, one launch behind the join of the front branches) costs per chunk: device time of a chunk
(rvc_last_gpu_ms, median of the timed chunks after 30 warm-up chunks) on the full-size v2 zoo with a 100 k index at rate 0.75, at each stream count, for
  (a) a library built from the parent commit (its path is given; loaded through RVC_LIB_OVERRIDE, twice: the two runs' difference is the spread),
  (b) this build, protect never set (the launch list of the parent),
  (c) this build, protect 0.33 on every stream.
Every leg is a process of its own (a process loads one library), the legs run one after the other in the order a, b, c, a, and each engine is fresh.
Rule: |(b) - mean of the two (a) runs| may be no more than (a)'s own first-to-last spread |a1 - a2|; (c) - (b) is reported, not bounded in advance.
usage: protect_cost.py PARENT_LIB [streams=1,8] [chunks=200] [out.json]          the four legs; prints and writes one JSON document
       protect_cost.py --leg unset|on|parent STREAMS CHUNKS                      one leg (what the driver starts); prints one JSON line"""
import json, os, subprocess, sys, time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def leg(kind, streams, chunks):
    import numpy as np
    import torch
    from common import BASELINE_160MS as g, voice_signal, zoo
    from obs_rvc_amd import _native, weights as W
    from obs_rvc_amd.rvc import RvcInfer
    L, chunk, N = g.input_buffer_16k_size, g.sample_frame_16k, g.model_return_size
    z = zoo("full", 2)
    index = W.make_index()
    out = {"leg": kind, "library": _native.lib()._name, "chunks": chunks, "gpu_ms_p50": {}, "wall_ms_p50": {}, "plan_ops": {}}
    _native.clock_monitor_start(0)
    for S in streams:
        # the second half of every stream is silence, so that about half of the rows are unvoiced and the stage has work to do
        xs = np.stack([voice_signal(L, seed=1 + s) for s in range(S)])
        xs[:, L - 2200:] = 0.0
        x = torch.from_numpy(xs).cuda()
        o = torch.empty((S, N), device="cuda")
        torch.cuda.synchronize()
        e = RvcInfer(z["data"], device=0); e.load_contentvec(2); e.load_f0(); e.load_model(z["model"]); e.set_streams(S); e.set_noise_seed(1, 0)
        e.load_index(index); e.set_index_rate(0.75)
        if kind == "on":
            e.set_protect(0.33)
        gm, wall = [], []
        for i in range(30 + chunks):
            t0 = time.perf_counter()
            e.infer_device(x.data_ptr(), L, chunk, 12, g.skip_head, g.model_return_length, o.data_ptr(), N, sync=True)
            if i >= 30:
                wall.append((time.perf_counter() - t0) * 1e3); gm.append(e.last_gpu_ms())
        out["gpu_ms_p50"][str(S)] = round(float(np.median(gm)), 5)
        out["wall_ms_p50"][str(S)] = round(float(np.median(wall)), 5)
        out["plan_ops"][str(S)] = e.plan_ops()
        e.close()
    out["shader_clock"] = _native.clock_monitor_stop(0)
    print(json.dumps(out), flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "--leg":
    leg(sys.argv[2], [int(v) for v in sys.argv[3].split(",")], int(sys.argv[4]))
    sys.exit(0)

parent = os.path.abspath(sys.argv[1])
streams = sys.argv[2] if len(sys.argv) > 2 else "1,8"
chunks = int(sys.argv[3]) if len(sys.argv) > 3 else 200
assert chunks >= 200, "medians of at least 200 chunks"
assert os.path.exists(parent), parent
legs = []
for name, kind in (("a1", "parent"), ("b", "unset"), ("c", "on"), ("a2", "parent")):
    env = dict(os.environ)
    if kind == "parent":
        env.update(RVC_TUNING="1", RVC_LIB_OVERRIDE=parent)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, streams, str(chunks)], env=env, stdout=subprocess.PIPE, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit("leg %s ended with status %d" % (name, r.returncode))        # (nothing more is started on the GPU)
    d = json.loads(r.stdout.strip().splitlines()[-1]); d["name"] = name
    d["library"] = os.path.basename(d["library"])
    legs.append(d)
    print(name, kind, d["gpu_ms_p50"], d["plan_ops"], flush=True)
by = {d["name"]: d["gpu_ms_p50"] for d in legs}
ops = {d["name"]: d["plan_ops"] for d in legs}
summary = {}
for S in by["b"]:
    a = 0.5 * (by["a1"][S] + by["a2"][S])
    spread = abs(by["a1"][S] - by["a2"][S])
    summary[S] = {"parent_ms": [by["a1"][S], by["a2"][S]], "parent_spread_ms": round(spread, 5), "unset_ms": by["b"][S], "on_ms": by["c"][S],
                  "unset_minus_parent_ms": round(by["b"][S] - a, 5), "on_minus_unset_ms": round(by["c"][S] - by["b"][S], 5),
                  "unset_within_parent_spread": bool(abs(by["b"][S] - a) <= spread),
                  "plan_ops": {"parent": ops["a1"][S], "unset": ops["b"][S], "on": ops["c"][S]}}
doc = {"tool": "tests/tools/protect_cost.py", "chunks": chunks, "summary_by_streams": summary, "legs": legs}
print(json.dumps(doc, indent=1))
if len(sys.argv) > 4:
    with open(sys.argv[4], "w") as fh:
        json.dump(doc, fh, indent=1)
