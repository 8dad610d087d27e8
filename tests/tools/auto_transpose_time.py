#!/usr/bin/env python
"""What auto-transpose costs a conversion on the full-size v2 zoo: `minutes` of voice_signal, RMVPE, k = 14, C = 48, X = 5, per stream
count the wall time and the rvc_convert_info total of rvc_convert with the target off and on (three runs each behind a warm-up, alternating), the two device
times of rvc_auto_transpose_info, the run-to-run spread of the target-off runs, and -- with --parent-lib, a library built from the parent commit, timed in a
child process -- the same target-off conversion there.  Then the select alone: rvc_f0_stats_stream (1024 rows where they lie, one launch) and rvc_f0_stats at
3.6 M rows (10 h of audio; the wall time includes the upload of the rows).
usage: auto_transpose_time.py [streams=1,8,32] [minutes=10] [--out profiles/auto_transpose.json] [--parent-lib PATH]"""
import json, os, subprocess, sys, time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from common import voice_signal, zoo
from obs_rvc_amd import _native
from obs_rvc_amd.rvc import RvcInfer

K, CTX, XF, RUNS = 14, 48, 5, 3


def opt(name, dflt=None):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i: i + 2]
        return v
    return dflt


def engine(S):
    z = zoo("full", 2)
    e = RvcInfer(z["data"], device=0); e.load_contentvec(2); e.load_f0_method("rmvpe"); e.load_model(z["model"]); e.set_streams(S); e.set_noise_seed(1, 0)
    return e


def timed(e, x):
    t0 = time.perf_counter()
    e.convert(x, k=K, context=CTX, crossfade=XF, highpass=True)
    return 1e3 * (time.perf_counter() - t0), e.convert_info()["ms_total"]


def off_leg(S, x):
    """the target-off conversion alone (also what the child process runs on the parent's library) -> [(wall ms, device ms)] * RUNS"""
    e = engine(S)
    timed(e, x[: 16000 * 20]); timed(e, x)
    out = [timed(e, x) for _ in range(RUNS)]
    e.close()
    return out


if __name__ == "__main__":
    out_path, parent, child = opt("--out", os.path.join(ROOT, "profiles", "auto_transpose.json")), opt("--parent-lib"), opt("--child")
    streams = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "1,8,32").split(",")]
    minutes = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    x = voice_signal(int(minutes * 60 * 16000), seed=5)
    if child is not None:          # the parent's library, in a process of its own: one stream count, one JSON line
        print("CHILD " + json.dumps(off_leg(int(child), x)), flush=True)
        sys.exit(0)
    res = {"library": _native.lib().rvc_version().decode(), "minutes": minutes, "k": K, "context": CTX, "crossfade": XF, "f0": "rmvpe", "runs": RUNS, "streams": {}}
    for S in streams:
        e = engine(S)
        timed(e, x[: 16000 * 20]); e.set_auto_transpose(155.0, 1, 12.0); timed(e, x[: 16000 * 20]); timed(e, x)          # both plans built, everything warm
        off, on, info = [], [], []
        for _ in range(RUNS):
            e.set_auto_transpose(0.0); off.append(timed(e, x))
            e.set_auto_transpose(155.0, 1, 12.0); on.append(timed(e, x)); info.append(e.auto_transpose_info())
        e.close()
        med = lambda rows, i: float(np.median([r[i] for r in rows]))
        r = {"off_wall_ms": [a for a, _ in off], "off_device_ms": [b for _, b in off], "on_wall_ms": [a for a, _ in on], "on_device_ms": [b for _, b in on],
             "analysis_ms": [t["ms_analysis"] for t in info], "select_ms": [t["ms_select"] for t in info], "median_hz": float(info[0]["median_hz"]),
             "voiced": info[0]["voiced"], "semitones": info[0]["semitones"]}
        r["off_spread"] = (max(r["off_wall_ms"]) - min(r["off_wall_ms"])) / med(off, 0)
        r["on_over_off_wall"] = med(on, 0) / med(off, 0); r["on_over_off_device"] = med(on, 1) / med(off, 1)
        if parent:
            env = dict(os.environ, RVC_TUNING="1", RVC_LIB_OVERRIDE=os.path.abspath(parent))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), str(S), str(minutes), "--child", str(S)], env=env, capture_output=True, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")]
            if p.returncode == 0 and line:
                rows = json.loads(line[0][6:])
                r["parent_wall_ms"] = [a for a, _ in rows]; r["parent_device_ms"] = [b for _, b in rows]
                r["off_over_parent_wall"] = med(off, 0) / med(rows, 0); r["off_over_parent_device"] = med(off, 1) / med(rows, 1)
            else:
                r["parent_error"] = (p.stderr or p.stdout)[-400:]
        res["streams"][str(S)] = r
        print("streams %2d  off wall %.1f ms (spread %.2f %%), on wall %.1f ms = %.3f x; analysis %.1f ms, select %.3f ms%s"
              % (S, med(off, 0), 100 * r["off_spread"], med(on, 0), r["on_over_off_wall"], np.median(r["analysis_ms"]), np.median(r["select_ms"]),
                 "; off / parent wall %.3f" % r["off_over_parent_wall"] if "off_over_parent_wall" in r else ""), flush=True)
    # the select alone
    e = RvcInfer(zoo("full", 2)["data"], device=0)
    rows = np.exp(np.random.default_rng(3).uniform(np.log(50.0), np.log(1100.0), 3600000)).astype(np.float32); rows[::5] = 0.0
    sel = {}
    for name, fn in (("stream_1024_rows", lambda: e.f0_stats_stream(0)), ("host_3600000_rows_with_upload", lambda: e.f0_stats(rows))):
        fn(); fn()
        t = []
        for _ in range(20):
            t0 = time.perf_counter(); fn(); t.append(1e3 * (time.perf_counter() - t0))
        sel[name + "_wall_ms_p50"] = float(np.median(t)); sel[name + "_wall_ms_min"] = float(min(t))
    e.close()
    res["select_alone"] = sel
    print("select alone:", sel, flush=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", out_path)
