"""Cost of the session's spectral-gate noise reduction (DESIGN.md "Spectral-gate noise reduction"): HIP events around the two stages
(rvc_debug_session_denoise_ms) and the wall time of the whole chunk, pass-through sessions at 48 kHz (160 ms chunks = 16 frames of 960 samples) at 1 and
64 streams, the modes -- off, input side, output side, both -- alternating in one process.  The stage does not depend on the model, so none is loaded.
With the stage off a chunk runs the parent's launches.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from common import voice_signal, zoo  # noqa: E402
from obs_rvc_amd.rvc import RvcInfer  # noqa: E402
from obs_rvc_amd.rvc_common import DENOISE_INPUT, DENOISE_OUTPUT  # noqa: E402
from obs_rvc_amd.streaming import NativeStreamingSession  # noqa: E402

WARM, ROUNDS, PER_ROUND = 10, 6, 20
MODES = ((0, "off", 0.0, 0.0), (1, "input", 1.0, 0.0), (2, "output", 0.0, 1.0), (3, "both", 1.0, 1.0))
res = {}
for S in (1, 64):
    e = RvcInfer(zoo("tiny")["data"])
    if S > 1:
        e.set_streams(S)
    s = NativeStreamingSession(e, 48000, 0.16, 0.07, 2.0, 40000, 12, 1.0, skip_inference=True)
    F = s.sample_frame_size
    x = np.stack([np.interp(np.arange(F) / 48000.0, np.arange(F // 3 + 8) / 16000.0, voice_signal(F // 3 + 8, seed=b)).astype(np.float32) for b in range(S)])
    s._L.rvc_debug_session_denoise_ms(s._h, 1)
    t = {m: ([], []) for m, _, _, _ in MODES}
    for rnd in range(ROUNDS + 1):
        for m, _, s_in, s_out in MODES:
            s.set_noise_reduction(DENOISE_INPUT, s_in); s.set_noise_reduction(DENOISE_OUTPUT, s_out)
            s.process_one_frame(x if S > 1 else x[0])          # the chunk after a setter call uploads the settings: not timed
            for i in range(WARM if rnd == 0 else PER_ROUND):
                t0 = time.perf_counter(); s.process_one_frame(x if S > 1 else x[0]); t1 = time.perf_counter()
                if rnd:
                    t[m][0].append(float(s._L.rvc_debug_session_denoise_ms(s._h, 1)) if m else 0.0); t[m][1].append((t1 - t0) * 1e3)
    res["streams_%d" % S] = {name: {"denoise_ms_median": float(np.median(t[m][0])), "denoise_ms_min": float(np.min(t[m][0])), "denoise_ms_max": float(np.max(t[m][0])),
                                    "chunk_wall_ms_median": float(np.median(t[m][1])), "chunk_wall_ms_min": float(np.min(t[m][1])), "chunk_wall_ms_max": float(np.max(t[m][1]))}
                             for m, name, _, _ in MODES}
    del s, e
print(json.dumps({"frame": 960, "frames_per_chunk": 16, "sample_rate": 48000, "chunks_per_mode": ROUNDS * PER_ROUND, **res}))
