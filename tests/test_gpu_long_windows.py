"""One window of a converted file, stage by stage, against float64 (DESIGN.md "Long windows: what is tested").

The file converter (rvc_convert) runs every model at window lengths the streaming suites never reach: by default (k = 14, context 48,
crossfade 5) Tm = 448 f0 frames, T = 223 ContentVec frames and return_length R = 351 (the last length the full models' relative attention holds in LDS; the
tiny zoo's head size 8 is far inside that limit, which only the single-op cases of tests/test_gpu_ops.py reach).  Its
own tests compare rvc_convert with the composition of public calls bit for bit; both sides run the same kernels.  Here a converter batch's first call is taken
apart: reset_state, then ONE infer_batch with taps on over inputs of exactly n = 5120 k - 160 samples (n == the f0 frame), one signal, pitch shift and Philox
stream id per stream, and

  * the ContentVec, RMVPE and f0 taps of each checked stream against that stream's own OracleRvcInfer (1e-4 relative RMS),
  * every tapped interval of the synthesizer teacher-forced through tests/synth_ref.py: 2e-5 for one launch, max(2e-5, 4 delta32) for multi-layer stages,
    bitwise for the gathers,
  * the PCM of every stream against its oracle's at 1e-3 RMS

with the machinery and the bounds of tests/test_gpu_stream_taps.py (imported, not copied).  Tiny zoo throughout; the cases are bounded by the CPU time of their
references, which is printed."""
import functools
import time

import numpy as np
import pytest

import test_gpu_stream_taps as ST
from common import rms, voice_signal
from debug_abi import RVC_SHAPE
from long_shapes import GEOMETRIES, far_end_context, geometry
from obs_rvc_amd.rvc_common import RvcInferError

pytestmark = pytest.mark.gpu
RVC_PANIC = 6                             # include/rvc_mi355x.h


@functools.lru_cache(maxsize=None)
def _input(k, s):
    return voice_signal(5120 * k - 160, seed=1 + s)


@functools.lru_cache(maxsize=None)
def _oracle(k, C, X, s):
    """stream s of a window (k, C, X): (the oracle's ContentVec / RMVPE / f0 taps, its PCM, CPU seconds); every stream count shares it"""
    from oracle import oracle as O
    z, _, _ = ST._model("tiny")
    n, sf, skip, R = geometry(k, C, X)
    t0 = time.process_time()
    o = O.OracleRvcInfer(z["data"]); o.load_contentvec(2); o.load_f0(1); o.load_model(z["model"]); o.set_noise_seed(ST.SEED, ST.ID0 + s)
    o.enable_taps(True)
    o.reset_state()
    y = o.infer(_input(k, s), sf, ST.SHIFTS[s], skip, R)
    taps = {}
    for oname, _, _ in ST.TAP_MAP:
        if oname.startswith(("cv.", "rm.")) or oname == "f0":
            try:
                taps[oname] = o.tap(oname)
            except KeyError:
                pass
    o.close()
    return taps, y, time.process_time() - t0


def _window(k, C, X, S, check):
    n, sf, skip, R = geometry(k, C, X)
    Tm = 32 * k
    z, cfg, tens = ST._model("tiny")
    tag = "k=%d C=%d X=%d (Tm %d, T %d, R %d) S=%d" % (k, C, X, Tm, 16 * k - 1, R, S)
    xs = np.stack([_input(k, s) for s in range(S)])
    assert xs.shape == (S, n)
    for level in (1, 2):
        eng = ST._engine("tiny", S, level)
        eng.reset_state()
        y = eng.infer_batch(xs, sf, np.array(ST.SHIFTS[:S], np.int32), skip, R)
        rep = ST.Report("%s taps=%d" % (tag, level))
        t_ref = time.process_time()
        for gs in check:
            taps, yo, sec = _oracle(k, C, X, gs)
            ST._front_taps(rep, eng, gs, gs, taps, hints={"rm.cnn": Tm, "rm.gru": Tm, "rm.sal": Tm})
            ST._synth_stages(rep, cfg, tens, eng, gs, gs, R, y[gs], skip_head=skip, chunk=0)
        print("%s: float64 / float32 stage references of %d streams took %.1f s of CPU" % (rep.tag, len(check), time.process_time() - t_ref))
        for s in range(S):                                       # the PCM of EVERY stream
            taps, yo, sec = _oracle(k, C, X, s)
            e = rms(y[s] - yo)
            print("%s stream %d PCM rms error %.2e (bound %.0e); its oracle took %.1f s of CPU" % (rep.tag, s, e, ST.PCM_TOL, sec))
            if not (y[s].shape == yo.shape and e < ST.PCM_TOL):
                rep.bad.append((s, "pcm", e, ST.PCM_TOL))
        eng.close()
        rep.done()


@pytest.mark.parametrize("k,C,X,S", [(2, 3, 2, 3), (14, 48, 5, 1), (14, 48, 5, 3), (9, 3, 1, 1)], ids=lambda v: str(v))
def test_window_stage_by_stage(k, C, X, S):
    assert geometry(k, C, X)[3] == GEOMETRIES[(k, C, X)][2]
    _window(k, C, X, S, sorted({0, S - 1}))                      # the interior... and the last stream is where a stride error shows


def _try_plan(eng, k):
    """one window of k at the far-end context on the engine -> None, or the RvcInferError of the refusal"""
    C = far_end_context(k)
    n, sf, skip, R = geometry(k, C, 1)
    try:
        eng.reset_state()
        eng.infer_batch(_input(k, 0)[None], sf, 0, skip, R)
        return None
    except RvcInferError as x:
        return x


def test_the_longest_window_the_planner_accepts():
    """downwards from k = 32 at R <= 351: every refused k fails with RVC_SHAPE / RVC_PANIC and a message, the first accepted one is checked stage by stage,
    and the engine converts the default geometry afterwards.  On the tiny zoo the planner refuses no k, so the loop's refusal branch does not run and the default
    window below follows no refusal: the LDS refusals are covered by the single-op tests of tests/test_gpu_ops.py only (the full zoo is out of this
    file's reach)"""
    eng = ST._engine("tiny", 1, 0)
    found = None
    for k in range(32, 14, -1):
        err = _try_plan(eng, k)
        C = far_end_context(k)
        if err is None:
            found = k
            print("k = %d, C = %d (Tm %d, T %d, R %d): accepted" % (k, C, 32 * k, 16 * k - 1, geometry(k, C, 1)[3]))
            break
        print("k = %d, C = %d (Tm %d, T %d, R %d): refused with %d: %s" % (k, C, 32 * k, 16 * k - 1, geometry(k, C, 1)[3], err.code, err))
        assert err.code in (RVC_SHAPE, RVC_PANIC) and len(str(err)) > 10, (k, err.code, str(err))
    # Measured: 32, without a refusal.  The tiny zoo's ContentVec heads are 12 wide and its text encoder's 8, so neither attention's LDS bound is reached
    # below k = 32 (T = 511, R = 351).  At the full models' head sizes the bounds are the ops' own: ContentVec T <= 499, so k <= 31, and R <= 351
    # (tests/test_gpu_ops.py test_attention_beyond_the_lds_limit_is_refused, test_relpos_attention_beyond_the_lds_limit_is_refused)
    assert found == 32, found
    n, sf, skip, R = geometry(14, 48, 5)
    y = eng.infer_batch(_input(14, 0)[None], sf, 0, skip, R)          # the engine is still good for the default window
    assert y.shape == (1, R * 48) and np.all(np.isfinite(y))
    eng.close()
    C = far_end_context(found)
    _window(found, C, 1, 1, [0])
