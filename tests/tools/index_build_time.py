"""Time the index builder on the full zoo: 10 minutes of seeded audio at the default window (3 s), one add per minute of audio.
Writes profiles/index_build.json: rows, the three device-millisecond figures of rvc_index_build_info, seconds of audio per second of build (wall clock, begin
to finish), and the append's bytes moved (each stored float read once and written once) divided by its device time, next to the read stream rvc_calibrate
reports in the same run.

    python tests/tools/index_build_time.py [--minutes 10] [--out profiles/index_build.json]"""
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_build.json"))
    a = ap.parse_args()
    from common import voice_signal, zoo
    from obs_rvc_amd import _native
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("full")
    e = RvcInfer(z["data"], device=0)
    e.load_contentvec(2)
    cal = _native.calibrate(0)
    recs = [voice_signal(60 * 16000, seed=100 + i) for i in range(a.minutes)]
    # warm-up: the window's plan (and the tail-free recordings need no other) is built outside the timed region, as a server would have it
    e.index_build_begin(0, 0); e.index_build_add(recs[0][:48000]); e.index_build_abort()
    t0 = time.perf_counter()
    e.index_build_begin(0, 0)
    for x in recs:
        e.index_build_add(x)
    info = e.index_build_info()
    rows = e.index_build_finish(0, 0)
    wall = time.perf_counter() - t0
    dim = e._index_shape[1]
    moved = 2.0 * info["rows"] * dim * 4
    out = {
        "what": "index builder, full zoo, v2, window 48000, %d minutes of seeded audio, one add per minute" % a.minutes,
        "version": _native.lib().rvc_version().decode(),
        "rows": rows, "dim": dim, "windows": info["windows"], "capacity": info["capacity"], "dropped_nonfinite": info["dropped_nonfinite"],
        "ms_contentvec": round(info["ms_contentvec"], 3), "ms_append": round(info["ms_append"], 3), "ms_reduce": round(info["ms_reduce"], 3),
        "wall_s": round(wall, 4), "audio_seconds_per_build_second": round(a.minutes * 60.0 / wall, 1),
        "append_bytes": moved, "append_us_per_window": round(1e3 * info["ms_append"] / max(info["windows"], 1), 2),
        "append_gbs": round(moved / (info["ms_append"] * 1e-3) / 1e9, 2),
        "calibrate_hbm_read_gbs": round(cal["hbm_read_tbs"] * 1e3, 1),
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    e.close()


if __name__ == "__main__":
    main()
