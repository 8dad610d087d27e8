"""Time the per-file pitch pass of rvc_convert_many on the full zoo (48 kHz synthesizer, RMVPE): `--clips` clips of `--seconds` of seeded
audio (default 64 x 10 s; default geometry; high-pass on) at each stream count of `--streams` (default 8, 32), plans warmed first, `--repeats` alternating runs:
  off    rvc_convert_many with both per-file settings cleared
  on     the same with rvc_set_convert_many_auto_transpose(220, 1, 12): the packed analysis, the segmented select, a multiplier per stream and batch
  loop   a loop of rvc_convert under rvc_set_auto_transpose(220, 1, 12), what a caller had to do before
With `--parent-lib PATH` (a library built from the parent commit) the `off` runs are repeated in a child process that loads that library, so the off path can be
held against the parent's.  Writes profiles/convert_many_pitch.json: wall seconds and device milliseconds per way (the median run and every run), the analysis /
select split of rvc_convert_many_pitch_info, and the ratios.

    python tests/tools/convert_many_pitch_time.py [--clips 64] [--seconds 10] [--streams 8,32] [--repeats 3] [--parent-lib PATH] [--out profiles/convert_many_pitch.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MS = ("ms_highpass", "ms_model", "ms_stitch", "ms_total")
TARGET = (220.0, 1, 12.0)


def engine(streams):
    from common import zoo
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("full")
    e = RvcInfer(z["data"], device=0)
    e.load_contentvec(2); e.load_f0(1); e.load_model(z["model"])
    e.set_streams(streams); e.set_noise_seed(7, 0)
    return e


def run_many(e, clips, pitch_info):
    t0 = time.perf_counter()
    e.convert_many(clips)
    wall = time.perf_counter() - t0
    info = e.convert_many_info()
    r = {"wall_s": wall, "batches": info["batches"], **{k: info[k] for k in MS}}
    if pitch_info:
        p = e.convert_many_pitch_info()
        r["ms_analysis"], r["ms_select"] = p["ms_analysis"], p["ms_select"]
    return r


def run_loop(e, clips):
    ms, batches, an, sel = dict.fromkeys(MS, 0.0), 0, 0.0, 0.0
    t0 = time.perf_counter()
    for x in clips:
        e.convert(x)
        info, t = e.convert_info(), e.auto_transpose_info()
        for k in MS:
            ms[k] += info[k]
        batches += info["batches"]; an += t["ms_analysis"]; sel += t["ms_select"]
    return {"wall_s": time.perf_counter() - t0, "batches": batches, **ms, "ms_analysis": an, "ms_select": sel}


def summary(runs):
    """the median run by device total, rounded, with every run's wall time and device total"""
    runs = sorted(runs, key=lambda r: r["ms_total"])
    out = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in runs[len(runs) // 2].items()}
    out["wall_s_all"] = [round(r["wall_s"], 4) for r in runs]
    out["ms_total_all"] = [round(r["ms_total"], 2) for r in runs]
    out["spread"] = round((runs[-1]["ms_total"] - runs[0]["ms_total"]) / runs[len(runs) // 2]["ms_total"], 5)
    return out


def off_only(a, clips, S):
    """the child's work under the parent's library: warm-up, then `repeats` runs with nothing set (the parent has no per-file setting)"""
    e = engine(S)
    e.convert_many(clips[:2])
    runs = [run_many(e, clips, False) for _ in range(a.repeats)]
    e.close()
    return summary(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--streams", default="8,32")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_many_pitch.json"))
    a = ap.parse_args()
    from common import voice_signal
    from obs_rvc_amd import _native
    clips = [voice_signal(int(a.seconds * 16000), seed=500 + i) for i in range(a.clips)]
    if a.child:
        print("CHILD " + json.dumps({"version": _native.lib().rvc_version().decode(), "off": off_only(a, clips, a.child)}), flush=True)
        return
    out = {"what": "the per-file pitch pass of rvc_convert_many, full zoo, v2, 48 kHz synthesizer, RMVPE, %d clips of %.1f s of seeded audio, default geometry, high-pass on; "
                   "target %.0f Hz, step %d, limit %.0f; the median of %d alternating runs by device total" % (a.clips, a.seconds, *TARGET, a.repeats),
           "version": _native.lib().rvc_version().decode(), "runs": []}
    for S in [int(s) for s in a.streams.split(",") if s]:
        e = engine(S)
        e.convert_many(clips[:2])                                   # warm-ups: every plan of the three ways is built outside the timed region
        e.set_convert_many_auto_transpose(*TARGET); e.convert_many(clips[:2]); e.set_convert_many_auto_transpose(0.0)
        e.set_auto_transpose(*TARGET); e.convert(clips[0]); e.set_auto_transpose(0.0)
        off, on, loop = [], [], []
        for _ in range(a.repeats):
            off.append(run_many(e, clips, False))
            e.set_convert_many_auto_transpose(*TARGET)
            on.append(run_many(e, clips, True))
            e.set_convert_many_auto_transpose(0.0)
            e.set_auto_transpose(*TARGET)
            loop.append(run_loop(e, clips))
            e.set_auto_transpose(0.0)
        e.close()
        row = {"streams": S, "clips": a.clips, "off": summary(off), "on": summary(on), "loop": summary(loop)}
        row["on_over_off_device"] = round(row["on"]["ms_total"] / row["off"]["ms_total"], 4)
        row["loop_over_on_device"] = round(row["loop"]["ms_total"] / row["on"]["ms_total"], 3)
        row["loop_over_on_wall"] = round(row["loop"]["wall_s"] / row["on"]["wall_s"], 3)
        if a.parent_lib:
            env = dict(os.environ, RVC_TUNING="1", RVC_LIB_OVERRIDE=os.path.abspath(a.parent_lib))
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(S), "--clips", str(a.clips), "--seconds", str(a.seconds), "--repeats", str(a.repeats)]
            res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("CHILD ")]
            if res.returncode == 0 and line:
                child = json.loads(line[-1][6:])
                row["parent"] = child
                row["off_over_parent_device"] = round(row["off"]["ms_total"] / child["off"]["ms_total"], 5)
            else:
                row["parent"] = {"failed": res.returncode, "stderr": res.stderr[-400:]}
        out["runs"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
