#!/usr/bin/env python
"""rocprofv3 --kernel-trace --stats CSV of `bench.py --only-headline --streams S --serial-branches` -> profiles/<round>_serial_<S>streams.json:
the sum of implicit-GEMM kernel time per step as rocprofv3 saw it (and, for the record, the HIP-event sum the same traced process printed), with the build hash
of the library.  bench.py divides the event sum of its own, unprofiled run by this pass's rocprofv3 sum (`this_run_events_over_committed_rocprof`): on the same build
and box that ratio validates the event method; it never withholds a figure because of it.

usage: serial_pass.py <kernel_stats.csv> <streams> <out.json> [csv name as committed] [bench line of the same process (json)]"""
import csv, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from obs_rvc_amd import _native

IGEMM = ("igemm_splitk_kernel", "igemm2_kernel", "igemm2w_kernel", "igemm_lds_kernel", "igemm32_kernel", "igemm32l_kernel", "igemm32w_kernel", "igemm_bf3_kernel", "conv_tile_kernel", "conv32s_kernel", "conv32s_buf_kernel", "rm_block_kernel", "splitk_epilogue_kernel")
rows = list(csv.DictReader(open(sys.argv[1])))
steps = sum(int(r["Calls"]) for r in rows if "advance_chunk_kernel" in r["Name"])
if steps < 3:
    raise SystemExit("no chunks in the trace")
ig = [r for r in rows if any(k in r["Name"] for k in IGEMM)]
tot_ns = sum(float(r["TotalDurationNs"]) for r in ig)
launches = sum(int(r["Calls"]) for r in ig)
out = {"source": "rocprofv3 --kernel-trace of `bench.py --only-headline --no-cpu --streams %s --serial-branches` (tests/tools/profile_round.sh)" % sys.argv[2],
       "csv": sys.argv[4] if len(sys.argv) > 4 else os.path.basename(sys.argv[1]), "build": _native.binary_hash(), "streams": int(sys.argv[2]),
       "steps_in_trace": steps, "igemm_launches_per_step": launches / steps, "sum_igemm_ms_per_step": tot_ns / steps * 1e-6,
       "kernel_class": ", ".join(IGEMM)}
if len(sys.argv) > 5:
    try:
        line = [ln for ln in open(sys.argv[5]).read().splitlines() if ln.startswith("{")][-1]
        roof = json.loads(line).get("roofline") or {}
        out["events_sum_igemm_ms_per_step"] = roof.get("sum_kernel_ms")
        out["events_launches_per_step"] = roof.get("launches_per_step")
        if roof.get("sum_kernel_ms"):
            out["events_under_rocprofv3_over_rocprof"] = roof["sum_kernel_ms"] / out["sum_igemm_ms_per_step"]
            out["events_note"] = ("the HIP-event sum printed by THIS process, i.e. taken while rocprofv3 traced it: the tool's dispatch interception adds ~4 us to every "
                                  "event pair (round 6: +3.9-4.6 us per launch at 8-64 streams), so this ratio is NOT the validation of the event method.  The validation "
                                  "is bench.py's `this_run_events_over_committed_rocprof`: the event sum of an UNPROFILED run over `sum_igemm_ms_per_step` of this pass "
                                  "(same build, same box: 1.001 at 64 streams in round 6)")
    except Exception as ex:
        out["events_note"] = "bench line unreadable: %s" % ex
json.dump(out, open(sys.argv[3], "w"), indent=1)
print(json.dumps(out, indent=1))
