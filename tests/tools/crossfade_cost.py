"""Cost of the SOLA stage with the linear and with the phase-vocoder crossfade (DESIGN.md "Phase-vocoder crossfade and input gate"): HIP events around
the stage (rvc_debug_session_sola_ms) and the wall time of the whole chunk, pass-through sessions at 48 kHz (seam of 1 920 samples) at 1 and 64
streams, the two modes alternating in one process.  The stage does not depend on the model, so none is loaded.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from common import voice_signal, zoo  # noqa: E402
from obs_rvc_amd.rvc import RvcInfer  # noqa: E402
from obs_rvc_amd.streaming import NativeStreamingSession  # noqa: E402

WARM, ROUNDS, PER_ROUND = 10, 6, 20
res = {}
for S in (1, 64):
    e = RvcInfer(zoo("tiny")["data"])
    if S > 1:
        e.set_streams(S)
    s = NativeStreamingSession(e, 48000, 0.16, 0.07, 2.0, 40000, 12, 1.0, skip_inference=True)
    F = s.sample_frame_size
    x = np.stack([np.interp(np.arange(F) / 48000.0, np.arange(F // 3 + 8) / 16000.0, voice_signal(F // 3 + 8, seed=b)).astype(np.float32) for b in range(S)])
    s._L.rvc_debug_session_sola_ms(s._h, 1)
    t = {0: ([], []), 1: ([], []), 2: ([], [])}       # 0 linear, 1 phase vocoder, 2 phase vocoder + gate
    for rnd in range(ROUNDS + 1):
        for mode in (0, 1, 2):
            s.set_crossfade(1 if mode else 0)
            s.set_input_gate(-40.0 if mode == 2 else -60.0)
            for i in range(WARM if rnd == 0 else PER_ROUND):
                t0 = time.perf_counter(); s.process_one_frame(x if S > 1 else x[0]); t1 = time.perf_counter()
                if rnd:
                    t[mode][0].append(float(s._L.rvc_debug_session_sola_ms(s._h, 1))); t[mode][1].append((t1 - t0) * 1e3)
    res["streams_%d" % S] = {name: {"sola_stage_ms_median": float(np.median(t[m][0])), "sola_stage_ms_min": float(np.min(t[m][0])), "sola_stage_ms_max": float(np.max(t[m][0])),
                                    "chunk_wall_ms_median": float(np.median(t[m][1]))} for m, name in ((0, "linear"), (1, "phase_vocoder"), (2, "phase_vocoder_gate"))}
    del s, e
print(json.dumps({"seam": 1920, "sample_rate": 48000, "chunks_per_mode": ROUNDS * PER_ROUND, **res}))
