"""Measurement behind DESIGN.md section 16: k-means training of an IVF structure over the 100 000 x 768 seeded index (nlist 2 564, the seeded default init,
iters 10), and what the trained structure does to the per-chunk retrieval next to the sampled one (iters 0 = centroids sampled from the rows, section 15's
stand-in).  One process for everything; the per-chunk settings are measured twice, interleaved.  Writes profiles/kmeans_train.json (or --out)."""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from common import BASELINE_160MS as g, voice_signal, zoo
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc import RvcInfer

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_train.json"))
ap.add_argument("--rows", type=int, default=100000)
ap.add_argument("--nlist", type=int, default=2564)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--streams", type=int, nargs="+", default=[1, 8])
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--chunks", type=int, default=24)
args = ap.parse_args()

z = zoo("full")
index = W.make_index(args.rows)
R, skip = g.model_return_length, g.skip_head
result = {"index": [args.rows, 768], "nlist": args.nlist, "iters": args.iters, "seed": 0}


def engine(streams):
    e = RvcInfer(z["data"], device=0)
    e.load_contentvec(2); e.load_f0_method("yin"); e.load_model(z["model"])
    e.set_plan_autotune(False)              # (the retrieval launches are not among what the tuner picks; plan builds stay short)
    if streams > 1:
        e.set_streams(streams)
    e.set_noise_seed(1, 0)
    e.load_index(index); e.set_index_rate(0.75)
    return e


def stats(v):
    v = np.asarray(v) * 1e3
    return {"median_us": round(float(np.median(v)), 2), "min_us": round(float(v.min()), 2), "max_us": round(float(v.max()), 2)}


e = engine(1)
# ---- training: iters 0 (the sampled structure) and the full run ----
before = e.train_index_ivf(nlist=args.nlist, iters=0, seed=0)
sampled = e.index_ivf()
runs = [e.train_index_ivf(nlist=args.nlist, iters=args.iters, seed=0) for _ in range(2)]          # (the first run also loads the code objects)
after = runs[1]
trained = e.index_ivf()
steps = after["iters_run"]
result["sampled"] = {k: before[k] for k in ("longest_list", "empty_lists", "objective", "ms_assign", "ms_total")}
result["trained"] = {k: after[k] for k in ("longest_list", "empty_lists", "iters_run", "moved_last", "objective", "ms_assign", "ms_update", "ms_total")}
result["trained"]["ms_assign_per_step"] = after["ms_assign"] / (steps + 1)
result["trained"]["ms_update_per_step"] = after["ms_update"] / max(steps, 1)
result["trained"]["first_run_ms_total"] = runs[0]["ms_total"]
pair_dims = float(args.rows) * args.nlist * 768
result["trained"]["assign_pair_dimensions_per_s"] = pair_dims / (result["trained"]["ms_assign_per_step"] * 1e-3)
print(json.dumps(result["trained"]), flush=True)
e.close()

# ---- per chunk: flat, sampled nprobe 1 / 8, trained nprobe 1 / 8; two interleaved passes ----
result["per_chunk"] = {}
for streams in args.streams:
    e = engine(streams)
    xs = np.stack([voice_signal(g.input_buffer_16k_size, seed=1 + s) for s in range(streams)])

    def chunk():
        e.reset_state(); e.set_noise_seed(1, 0)
        if streams > 1:
            e.infer_batch(xs, g.sample_frame_16k, 12, skip, R)
        else:
            e.infer(xs[0], g.sample_frame_16k, 12, skip, R)

    def measure():
        for _ in range(args.warmup):
            chunk()
        e.set_profile(True)
        ms, launches, nbytes = [], 0, 0.0
        for _ in range(args.chunks):
            chunk()
            launches, kms, nbytes = e.profile_last_knn()
            ms.append(kms)
        e.set_profile(False)
        idx, _ = e.knn(rows_cap=streams * R)
        return dict(stats(ms), launches=launches, bytes=nbytes), idx

    table, top1 = {}, None
    for p in (1, 2):
        for name, structure, nprobe in (("flat", None, 0), ("sampled nprobe 1", sampled, 1), ("sampled nprobe 8", sampled, 8),
                                        ("trained nprobe 1", trained, 1), ("trained nprobe 8", trained, 8)):
            if structure is not None and nprobe == 1:
                e.set_index_ivf(*structure)
            e.set_index_nprobe(nprobe)
            row, idx = measure()
            if name == "flat":
                top1 = idx[:, 0]
            else:
                row["flat_top1_among_hits"] = float(np.mean([top1[r] in idx[r] for r in range(len(top1))]))
            table.setdefault(name, {})["pass%d" % p] = row
            print(streams, name, p, row, flush=True)
    result["per_chunk"]["%d streams" % streams] = table
    e.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", args.out)
