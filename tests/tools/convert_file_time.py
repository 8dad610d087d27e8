"""Time a file at a rate other than 16 kHz through both routes on the full zoo (48 kHz synthesizer): `--minutes` of seeded audio at
`--rate-in` in and `--rate-out` out, at each stream count of `--streams`:
  device   RvcInfer.convert_file: both rate conversions, the envelope (`--rms-mix-rate`) and the peak on the device, one upload and one download;
  blocks   RvcInfer.convert(x, rate) + convert._resample: the streaming converter block by block on both sides (no envelope: that route has none).
Writes wall seconds of each route, the block loops' own wall seconds and the seven device times of rvc_convert_file_info to `--out`.

    python tests/tools/convert_file_time.py [--minutes 10] [--streams 8,32] [--rate-in 48000] [--rate-out 44100] [--rms-mix-rate 0.25] [--out profiles/convert_file_time.json]"""
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
    ap.add_argument("--streams", default="8,32")
    ap.add_argument("--rate-in", type=int, default=48000)
    ap.add_argument("--rate-out", type=int, default=44100)
    ap.add_argument("--rms-mix-rate", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_file_time.json"))
    a = ap.parse_args()
    from common import voice_signal
    from obs_rvc_amd import _native
    from obs_rvc_amd.convert import _resample
    n = int(a.minutes * 60 * a.rate_in)
    minute = 60 * a.rate_in
    x = np.concatenate([voice_signal(min(minute, n - i), seed=100 + i // minute, sr=a.rate_in) for i in range(0, n, minute)])
    out = {"what": "a file through both routes, full zoo, v2, 48 kHz synthesizer, %.2f minutes of seeded audio at %d Hz in, %d Hz out, k = 14, C = 48, X = 5, high-pass on"
                   % (a.minutes, a.rate_in, a.rate_out), "version": _native.lib().rvc_version().decode(), "runs": []}
    for S in [int(s) for s in a.streams.split(",") if s]:
        e = engine(S)
        warm = x[: a.rate_in * 6]          # the plan (and its autotuning) and the filter tables are built outside the timed region, as a server would have them
        e.convert_file(warm, a.rate_in, rms_mix_rate=a.rms_mix_rate, out_rate=a.rate_out)
        t0 = time.perf_counter()
        y, rate = e.convert_file(x, a.rate_in, rms_mix_rate=a.rms_mix_rate, out_rate=a.rate_out)
        wall_dev = time.perf_counter() - t0
        f = e.convert_file_info()
        side = f["ms_resample_in"] + f["ms_envelope"] + f["ms_resample_out"]
        run = {"streams": S, "device": {"wall_s": round(wall_dev, 4), "output_samples": int(len(y)), "rate": rate, "peak": float(f["peak"]),
                                         **{k: round(v, 3) for k, v in f.items() if k.startswith("ms_")},
                                         "resamplers_and_envelope_share": round(side / f["ms_total"], 5), "finite": bool(np.all(np.isfinite(y)))}}
        print(json.dumps(run), flush=True)
        # without the envelope: what the device route costs for exactly the work the block route does
        t0 = time.perf_counter()
        e.convert_file(x, a.rate_in, rms_mix_rate=1.0, out_rate=a.rate_out)
        run["device_no_envelope_wall_s"] = round(time.perf_counter() - t0, 4)
        e.convert(warm, rate=a.rate_in)
        t0 = time.perf_counter()
        x16 = e._to_16k(x, a.rate_in)
        t_in = time.perf_counter() - t0
        t0 = time.perf_counter()
        yb, model_rate = e.convert(x, rate=a.rate_in)
        t_conv = time.perf_counter() - t0          # (runs _to_16k again: the route as a caller has it)
        t0 = time.perf_counter()
        yb = _resample(e, yb, model_rate, a.rate_out) if a.rate_out != model_rate else yb
        t_out = time.perf_counter() - t0
        info = e.convert_info()
        run["blocks"] = {"wall_s": round(t_conv + t_out, 4), "to_16k_loop_wall_s": round(t_in, 4), "out_loop_wall_s": round(t_out, 4),
                         "convert_device_ms_total": round(info["ms_total"], 3), "output_samples": int(len(yb)), "blocks_in": int(-(-len(x) // max(a.rate_in // 50, 1)) + 1),
                         "len_16k": int(len(x16))}
        run["speedup_wall"] = round(run["blocks"]["wall_s"] / run["device_no_envelope_wall_s"], 2)
        print(json.dumps(run), flush=True)
        out["runs"].append(run)
        e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
