"""Time rvc_convert_many against a loop of rvc_convert on the full zoo (48 kHz synthesizer): `--clips` clips of `--seconds` of seeded
audio (default 64 x 10 s; default geometry k = 14, C = 48, X = 5; high-pass on) at each stream count of `--streams` (default 8, 32), both ways in the same
process and build, plans warmed by one call first, `--repeats` times alternating.  Writes profiles/convert_many_time.json: wall seconds, the
device-millisecond split of rvc_convert_many_info / the summed rvc_convert_info, the stitch's share, and whether the two ways give the same bits.

    python tests/tools/convert_many_time.py [--clips 64] [--seconds 10] [--streams 8,32] [--repeats 3] [--out profiles/convert_many_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MS = ("ms_highpass", "ms_model", "ms_stitch", "ms_total")


def engine(streams):
    from common import zoo
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("full")
    e = RvcInfer(z["data"], device=0)
    e.load_contentvec(2); e.load_f0(1); e.load_model(z["model"])
    e.set_streams(streams); e.set_noise_seed(7, 0)
    return e


def run_many(e, clips):
    t0 = time.perf_counter()
    ys = e.convert_many(clips)
    wall = time.perf_counter() - t0
    info = e.convert_many_info()
    return ys, {"wall_s": wall, "batches": info["batches"], "windows": info["windows"], **{k: info[k] for k in MS}}


def run_loop(e, clips):
    ys, ms, batches, windows = [], dict.fromkeys(MS, 0.0), 0, 0
    t0 = time.perf_counter()
    for x in clips:
        ys.append(e.convert(x)[0])
        info = e.convert_info()      # (host-side bookkeeping of the loop, inside its wall time as a caller's would be)
        for k in MS:
            ms[k] += info[k]
        batches += info["batches"]; windows += info["windows"]
    wall = time.perf_counter() - t0
    return ys, {"wall_s": wall, "batches": batches, "windows": windows, **ms}


def summary(runs):
    """the median run by wall time, rounded, with the spread of the wall times"""
    runs = sorted(runs, key=lambda r: r["wall_s"])
    m = dict(runs[len(runs) // 2])
    out = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in m.items()}
    out["wall_s_all"] = [round(r["wall_s"], 4) for r in runs]
    out["stitch_share"] = round(m["ms_stitch"] / m["ms_total"], 5)
    out["model_ms_per_batch"] = round(m["ms_model"] / m["batches"], 3)
    out["stitch_us_per_batch"] = round(1e3 * m["ms_stitch"] / m["batches"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--streams", default="8,32")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_many_time.json"))
    a = ap.parse_args()
    from common import voice_signal
    from obs_rvc_amd import _native
    from obs_rvc_amd.rvc_common import RvcInferError
    clips = [voice_signal(int(a.seconds * 16000), seed=500 + i) for i in range(a.clips)]
    out = {"what": "rvc_convert_many against a loop of rvc_convert, full zoo, v2, 48 kHz synthesizer, %d clips of %.1f s of seeded audio, k = 14, C = 48, X = 5, high-pass on; "
                   "the median of %d alternating runs by wall time" % (a.clips, a.seconds, a.repeats),
           "version": _native.lib().rvc_version().decode(), "runs": []}
    for S in [int(s) for s in a.streams.split(",") if s]:
        e = engine(S)
        try:
            e.convert(clips[0])              # warm-up: the plan (and its autotuning) is built outside the timed region; both ways use the same plan
            e.convert_many(clips[:2])
        except RvcInferError as err:         # a stream count whose plan the planner refuses at this window is reported, not timed
            out["runs"].append({"streams": S, "refused": str(err)})
            print(json.dumps(out["runs"][-1]), flush=True)
            e.close()
            continue
        many, loop, same = [], [], True
        for _ in range(a.repeats):
            ym, rm = run_many(e, clips)
            yl, rl = run_loop(e, clips)
            many.append(rm); loop.append(rl)
            # a clip's windows run on other streams and chunk counters in the two ways (its place in the batches differs), so the noise differs: the same
            # lengths and finite samples are what must agree here; the bitwise equality is the test suite's, against the composition in the packed order
            same = same and all(len(p) == len(q) and np.all(np.isfinite(p)) for p, q in zip(ym, yl))
        m, l = summary(many), summary(loop)
        row = {"streams": S, "clips": a.clips, "many": m, "loop": l, "same_lengths_and_finite": bool(same),
               "wall_ratio_loop_over_many": round(l["wall_s"] / m["wall_s"], 3), "device_ratio_loop_over_many": round(l["ms_total"] / m["ms_total"], 3),
               "batch_ratio_loop_over_many": round(l["batches"] / m["batches"], 3)}
        out["runs"].append(row)
        print(json.dumps(row), flush=True)
        e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
