"""The per-stream control block (csrc/state.hip.h StreamCtl, csrc/engine.hip push_call_params) and the plan key (csrc/engine_int.h PlanKey) from the ABI:
the pinned ring behind unsynchronised calls that each change a control, the key members no other file counts builds for, and the call that changes nothing.

Every comparison is bit for bit: both sides run the same plan and the same kernels (the tiny zoo, YIN, the 160 ms geometry, at most 3 streams: the planner's
rules, no timing trials), so nothing but the order of host calls differs between them."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from common import BASELINE_160MS as g, voice_signal, zoo
from obs_rvc_amd import _native, weights as W
from obs_rvc_amd.rvc import SCALE_C_MAJOR

pytestmark = pytest.mark.gpu

FRAME16K, R, L, SKIP, CAP = g.sample_frame_16k, g.model_return_length, g.input_buffer_16k_size, g.skip_head, g.model_return_size      # (CAP: room for any zoo's rate)
SEED = 4321


def _engine(streams=1, index=False):
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("tiny")
    e = RvcInfer(z["data"])
    e.load_contentvec(2); e.load_model(z["model"]); e.load_f0_method("yin")
    if streams > 1:
        e.set_streams(streams)
    e.set_noise_seed(SEED, 0)
    if index:
        e.load_index(W.make_index(3000, 48, seed=5)); e.set_index_rate(0.75)
    return e


# ---- 1. ten unsynchronised calls, each with another control changed: more than the ring's 8 blocks ----
S = 3
# (call, what changes in front of it): a different control on a different stream than the call before; protect leaves 0.5 once (call 5) and stays below
STEPS = [
    lambda e, sh: sh.__setitem__(0, 12),
    lambda e, sh: e.set_pitch_semitones(3.5, stream=1),
    lambda e, sh: e.set_f0_range(100.0, 300.0, stream=2),
    lambda e, sh: e.set_f0_median(2, stream=0),
    lambda e, sh: e.set_f0_snap(SCALE_C_MAJOR, 0.8, stream=1),
    lambda e, sh: e.set_protect(0.2, stream=2),
    lambda e, sh: sh.__setitem__(1, -12),
    lambda e, sh: e.set_pitch_semitones(-2.25, stream=2),
    lambda e, sh: e.set_f0_range(80.0, 400.0, stream=0),
    lambda e, sh: e.set_f0_median(3, stream=1),
]


def _ten_calls(d_in, sync):
    import torch
    e = _engine(S, index=True)
    lib = _native.lib()
    d_out = torch.zeros((len(STEPS), S, CAP), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    shifts = np.zeros(S, np.int32)
    n = C.c_size_t()
    for k, step in enumerate(STEPS):
        step(e, shifts)
        rc = lib.rvc_infer_device_v(e._h, C.c_void_p(d_in[k].data_ptr()), L, FRAME16K, shifts.ctypes.data_as(C.POINTER(C.c_int32)), SKIP, R,
                                    C.c_void_p(d_out[k].data_ptr()), CAP, C.byref(n), 1 if sync else 0)
        assert rc == 0 and 0 < n.value <= CAP, (k, rc, n.value)
    e.synchronize()
    res = d_out[:, :, :n.value].cpu().numpy(), [e.pitch_cache(s) for s in range(S)], e.plan_cache_info()["builds"]
    e.close()
    return res


def test_ring_wrap_under_unsynchronised_calls():
    import torch
    xs = np.stack([np.stack([voice_signal(L, seed=1 + S * k + s) for s in range(S)]) for k in range(len(STEPS))])
    d_in = torch.from_numpy(xs).cuda()
    ya, ca, ba = _ten_calls(d_in, sync=False)
    ys, cs, bs = _ten_calls(d_in, sync=True)
    print("builds: unsynchronised %d, synchronous %d" % (ba, bs))
    assert np.all(np.isfinite(ya)) and np.any(ya != 0.0)
    for k in range(len(STEPS)):
        assert np.array_equal(ya[k], ys[k]), "call %d" % k
        if k:
            assert not np.array_equal(ya[k], ya[k - 1]), "call %d" % k
    assert all(np.array_equal(p, q) for p, q in zip(ca, cs)) and np.any(ca[0] > 0)
    # the keys the sequence visits: without and with the protect launch; no control, whichever stream it changes on, is part of a key
    assert ba == 2 and bs == 2, (ba, bs)


# ---- 2. key members no other file counts builds for: the GEMM precision, the taps level ----
@pytest.mark.parametrize("member", ["gemm_precision", "taps"])
def test_toggle_costs_one_build_out_and_none_back(member):
    e = _engine()
    x = voice_signal(L, seed=3)
    toggle = (lambda v: e.set_gemm_precision(1 if v else 0)) if member == "gemm_precision" else (lambda v: e.enable_taps(2 if v else False))

    def call():
        e.reset_state()
        return e.infer(x, FRAME16K, 12, SKIP, R), e.plan_cache_info()["builds"]
    y0, b0 = call()
    toggle(True)
    y1, b1 = call()
    toggle(False)
    y2, b2 = call()
    e.close()
    print("%s: builds %d -> %d -> %d" % (member, b0, b1, b2))
    assert b1 == b0 + 1 and b2 == b1, (b0, b1, b2)
    assert y1.shape == y0.shape and np.all(np.isfinite(y1))
    assert np.array_equal(y2, y0)


# ---- 3. a call that changes nothing copies nothing, and computes what a call behind a full copy computes ----
def test_second_identical_call_takes_the_fast_path():
    x0 = x1 = voice_signal(L, seed=5)                    # two identical calls (the second differs by the state the first left: chunk counter, pitch cache)
    e = _engine()
    e.set_pitch_semitones(1.5); e.set_f0_median(1)
    ya0 = e.infer(x0, FRAME16K, 12, SKIP, R)
    builds = e.plan_cache_info()["builds"]
    ya1 = e.infer(x1, FRAME16K, 12, SKIP, R)              # same settings, same shift, same seed: push_call_params returns at its comparison
    assert e.plan_cache_info()["builds"] == builds
    e.close()
    # a fresh engine, advanced by one chunk; rvc_set_pipeline(off) forgets what the device was sent, so its second call copies everything again
    f = _engine()
    f.set_pitch_semitones(1.5); f.set_f0_median(1)
    yf0 = f.infer(x0, FRAME16K, 12, SKIP, R)
    f.set_pipeline(False)
    yf1 = f.infer(x1, FRAME16K, 12, SKIP, R)
    f.close()
    assert np.array_equal(ya0, yf0) and np.array_equal(ya1, yf1) and not np.array_equal(ya0, ya1) and np.all(np.isfinite(ya1))
