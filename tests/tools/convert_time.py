"""Time the file converter on the full zoo (48 kHz synthesizer): `--minutes` of seeded audio through RvcInfer.convert at each stream
count of `--streams` (default 1, 8, 64; default geometry k = 14, C = 48, X = 5; high-pass on), and -- `--session` -- the same audio through
NativeStreamingSession at the baseline 160 ms geometry on one stream, which is what a user could do before the converter existed.  Writes
profiles/convert_time.json: wall seconds, the device-millisecond split of rvc_convert_info, the stitch's share, frames of 10 ms per second.

    python tests/tools/convert_time.py [--minutes 10] [--streams 1,8,64] [--session] [--out profiles/convert_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def engine(streams):
    from common import zoo
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("full")
    e = RvcInfer(z["data"], device=0)
    e.load_contentvec(2); e.load_f0(1); e.load_model(z["model"])
    e.set_streams(streams); e.set_noise_seed(7, 0)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--streams", default="1,8,64")
    ap.add_argument("--session", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_time.json"))
    a = ap.parse_args()
    from common import voice_signal
    from obs_rvc_amd import _native
    from obs_rvc_amd.rvc_common import RvcInferError
    n16 = int(a.minutes * 60 * 16000)
    x = np.concatenate([voice_signal(min(60 * 16000, n16 - i), seed=100 + i // (60 * 16000)) for i in range(0, n16, 60 * 16000)])
    frames = -(-len(x) // 160)
    out = {"what": "file converter, full zoo, v2, 48 kHz synthesizer, %.2f minutes of seeded audio, k = 14, C = 48, X = 5, high-pass on" % a.minutes,
           "version": _native.lib().rvc_version().decode(), "frames_10ms": frames, "convert": [], "session": None}
    for S in [int(s) for s in a.streams.split(",") if s]:
        e = engine(S)
        try:
            e.convert(x[: 16000 * 6])        # warm-up: the plan (and its autotuning) is built outside the timed region, as a server would have it
        except RvcInferError as err:         # a stream count whose plan the planner refuses at this window is reported, not timed
            out["convert"].append({"streams": S, "refused": str(err)})
            print(json.dumps(out["convert"][-1]), flush=True)
            e.close()
            continue
        t0 = time.perf_counter()
        y, rate = e.convert(x)
        wall = time.perf_counter() - t0
        info = e.convert_info()
        out["convert"].append({
            "streams": S, "windows": info["windows"], "batches": info["batches"], "model_rate": rate, "output_samples": int(len(y)),
            "wall_s": round(wall, 4), "x_real_time": round(a.minutes * 60.0 / wall, 1), "frames_per_s_wall": round(frames / wall, 1),
            "ms_highpass": round(info["ms_highpass"], 3), "ms_model": round(info["ms_model"], 3), "ms_stitch": round(info["ms_stitch"], 3),
            "ms_total": round(info["ms_total"], 3), "stitch_share": round(info["ms_stitch"] / info["ms_total"], 5),
            "stitch_us_per_batch": round(1e3 * info["ms_stitch"] / info["batches"], 2), "model_ms_per_batch": round(info["ms_model"] / info["batches"], 3),
            "frames_per_s_device": round(frames / (info["ms_total"] * 1e-3), 1), "finite": bool(np.all(np.isfinite(y))),
        })
        print(json.dumps(out["convert"][-1]), flush=True)
        e.close()
    if a.session:
        from obs_rvc_amd.streaming import NativeStreamingSession
        e = engine(1)
        s = NativeStreamingSession(e, 48000, 0.16, 0.07, 2.0, 48000, 0, 1.0)
        f = s.sample_frame_size
        # the session takes host-rate audio: the same signal generated at 48 kHz, chunk by chunk
        x48 = np.concatenate([voice_signal(min(60 * 48000, 3 * n16 - i), seed=100 + i // (60 * 48000), sr=48000) for i in range(0, 3 * n16, 60 * 48000)])
        for i in range(4):
            s.process_one_frame(x48[i * f:(i + 1) * f])
        chunks = len(x48) // f
        t0 = time.perf_counter()
        for i in range(chunks):
            s.process_one_frame(x48[i * f:(i + 1) * f])
        wall = time.perf_counter() - t0
        out["session"] = {"geometry": "48 kHz host rate, 160 ms chunks, 70 ms crossfade, 2 s extra context", "chunks": chunks, "wall_s": round(wall, 4),
                          "ms_per_chunk": round(1e3 * wall / chunks, 4), "x_real_time": round(chunks * 0.16 / wall, 1), "frames_per_s_wall": round(16 * chunks / wall, 1)}
        print(json.dumps(out["session"]), flush=True)
        del s
        e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
