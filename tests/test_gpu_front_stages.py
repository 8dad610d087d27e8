"""ContentVec and RMVPE of every stream of a batched plan, stage by stage, against float64 -- the scheme of test_gpu_stream_taps.py (whose helpers
are used) carried to the two networks that feed the synthesizer.  Every stream has its own signal and pitch shift, two chunks are run, and every interval
between two taps is TEACHER-FORCED: its float64 value (tests/front_stage_ref.py) is computed from the GPU's own upstream tap of the same stream, so an
error is charged to the stage that made it -- build_contentvec's halo / dropped column / aliased residual / folded-LayerNorm hand-overs, build_rmvpe's
concat halves, folded poolings, GRU-layout head and streams folded into N.  Metric: e = max |gpu - ref64| / rms(ref64).

  * single launches (conv0, final_proj, mel, head conv, salience): e <= TOL = 2e-5 (tests/test_gpu_tiles.py)
  * multi-launch stages (stem, proj, pos, every transformer layer, every U-Net level, the GRU): e <= max(TOL, 4 delta32), delta32 = torch's own fp32
    evaluation of the stage on the same inputs against the fp64 one; on plans that fold their LayerNorms (cv.pos.raw published) the larger of that and of
    the fp32 folded algebra restated in torch (front_stage_ref.folded_linear).  Neither involves the engine; 4 = two summation reorderings, each of the
    order of delta32 (as the synthesizer's test).
  * cv.out of a v2 model: the last layer's tap, bitwise.
tests/test_front_stage_ref.py shows on the CPU that a wrong pad, a column dropped at the wrong end, a swapped concat, a missing pooling, a missing pending
LayerNorm or ONE wrong element each miss these bounds by more than 200 x.

Cases sit on the thresholds of the two builders and the planner (CU partition and fused RMVPE blocks up to 4 streams, conv0 channels per workgroup at 4
and 16, gru_multi up to 8, LayerNorm strips / LDS GEMMs from 16, LayerNorm folds at one stream of the wide models, the 2-XCD ContentVec partition of v1),
not at workload size; each hooked case asserts that its plan is not the default one.  Every (stage, e, delta32, e / delta32) is printed; DESIGN.md
"ContentVec and RMVPE stages: what is tested" records the worst per stage and plan."""
import functools

import numpy as np
import pytest

import front_stage_ref as FS
from common import BASELINE_160MS as g, set_opt, zoo
from obs_rvc_amd import weights as W
from test_gpu_stream_taps import ID0, SEED, Report, _has, _inputs, _run

pytestmark = pytest.mark.gpu
R = g.model_return_length


@functools.lru_cache(maxsize=None)
def _models(preset, version):
    z = zoo(preset, version)
    ccfg, ct = W.read_blob("%s/contentvec/%s" % (z["data"], W.cv_blob_name(version)))
    rcfg, rt = W.read_blob("%s/f0/rmvpe.rvcw" % z["data"])
    return z, ccfg, ct, rcfg, rt


@functools.lru_cache(maxsize=None)
def _audio_refs(preset, version, s, c=1):
    """what depends on the stream's audio alone, computed once per (preset, stream): (cv.conv0, rm.mel) in float64 of chunk c"""
    _, ccfg, ct, _, _ = _models(preset, version)
    x = _inputs(s + 1)[c][s]
    return FS.cv_conv0(ccfg, ct, x), FS.rm_mel(x, FS.mel_frame(g.sample_frame_16k)[0])


def _engine(preset, version, S, level):
    from obs_rvc_amd.rvc import RvcInfer
    z = _models(preset, version)[0]
    eng = RvcInfer(z["data"]); eng.load_contentvec(version); eng.load_f0(); eng.load_model(z["model"])
    if S > 1:
        eng.set_streams(S)
    eng.set_noise_seed(SEED, ID0)
    eng.enable_taps(level)
    return eng


def _check_stream(rep, preset, version, eng, S, s):
    _, ccfg, ct, rcfg, rt = _models(preset, version)
    audio = _inputs(S)[1][s]
    assert np.array_equal(audio, _inputs(s + 1)[1][s])          # (a stream's signal does not depend on how many streams there are)
    ref_conv0, ref_mel = _audio_refs(preset, version, s)

    def get(name, shape):
        return eng.tap(name, s).reshape(shape)

    stages = FS.cv_stages(ccfg, ct, audio, get, lambda n: _has(eng, n, s)) + FS.rm_stages(rcfg, rt, audio, g.sample_frame_16k, get)
    for stage, kind, got, fn, args, fold in stages:
        if kind == "bits":
            rep.bits(s, stage, got, args[0])
        elif stage in ("cv.conv0", "rm.mel"):
            rep.add(s, stage, FS.max_over_rms(got, ref_conv0 if stage == "cv.conv0" else ref_mel), FS.TOL)
        else:
            e, bound, d32 = FS.judge(kind, got, fn, args, fold)
            rep.add(s, stage, e, bound, d32)
    return [st[0] for st in stages]


def _case(preset, version, S, level, check=None, tag=""):
    """one plan: two chunks, every stage of every stream in `check` (default: all).  -> (launches of the plan, stage names of the last stream, Report,
    cv.conv0 of stream 0)"""
    eng = _engine(preset, version, S, level)
    try:
        _run(eng, S, R)
        rep = Report("%s v%d S=%d taps=%d%s" % (preset, version, S, level, tag))
        for s in (range(S) if check is None else check):
            names = _check_stream(rep, preset, version, eng, S, s)
        ops, conv0 = eng.plan_ops(), eng.tap("cv.conv0", 0)
    finally:
        eng.close()
    return ops, names, rep, conv0


@functools.lru_cache(maxsize=None)
def _default(preset, version, S, level):
    """the plan the rules build, every stream checked: built and judged once, shared by the tests that compare a hooked plan with it"""
    return _case(preset, version, S, level)


def _n_stages(preset, version):
    _, ccfg, _, rcfg, _ = _models(preset, version)
    return 4 + int(ccfg["run_layers"]) + 1 + 1 + int(rcfg["levels"]) + 1 + int(rcfg["levels"]) + 3


# ---- tiny v2: 4 | 5 the CU partition, the fused RMVPE blocks and conv0's 2 -> 4 channels per workgroup (from 4); 8 | 9 gru_multi; 16 | 17 LayerNorm strips,
# LDS GEMMs and conv0's 16 channels per workgroup (from 16)
@pytest.mark.parametrize("S", [1, 2, 4, 5, 8, 9, 16, 17])
@pytest.mark.parametrize("level", [1, 2])
def test_tiny_every_stream_both_plans(S, level):
    ops, names, rep, _ = _default("tiny", 2, S, level)
    assert len(names) == _n_stages("tiny", 2) and "cv.pos" in names      # (the narrow model folds no LayerNorm: both plans hold normalised taps)
    rep.done()


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("level", [1, 2])
def test_tiny_v1_one_layer_and_final_proj(S, level):
    ops, names, rep, _ = _case("tiny", 1, S, level)
    assert names.count("cv.l0") == 1 and "cv.l1" not in names and "cv.out" in rep.worst     # final_proj is a measured stage, not a bitwise one
    rep.done()


# ---- full v2, the production plan: one stream folds every LayerNorm of ContentVec into the GEMMs around it; two streams launch them
@pytest.mark.parametrize("S", [1, 2])
def test_full_production_plan(S):
    ops, names, rep, _ = _default("full", 2, S, 2)
    if S == 1:
        assert "cv.pos.raw" in names and [n for n in names if n.startswith("cv.l")] == ["cv.l%d.raw" % l for l in range(11)] + ["cv.l11"]
    else:
        assert "cv.pos" in names and [n for n in names if n.startswith("cv.l")] == ["cv.l%d" % l for l in range(12)]
    rep.done()


def test_full_v1_nine_layers_and_final_proj():
    ops, names, rep, _ = _case("full", 1, 1, 2)
    assert "cv.pos.raw" in names and [n for n in names if n.startswith("cv.l")] == ["cv.l%d.raw" % l for l in range(8)] + ["cv.l8"] and "cv.out" in rep.worst
    rep.done()


# ---- hooks: each case runs a plan that is NOT the default one, asserted through what the plan publishes (raw taps), its launch count against the default
# plan's, or the bits of the stage the hook re-routes
def _hooked(name, value, preset, version, S, level=2):
    ops0, names0, rep0, conv0_0 = _default(preset, version, S, level)
    try:
        set_opt(name, value)
        ops1, names1, rep1, conv0_1 = _case(preset, version, S, level, tag=" %s=%s" % (name, value))
    finally:
        set_opt(name, None)
    return (ops0, names0, rep0, conv0_0), (ops1, names1, rep1, conv0_1)


def test_full_without_layernorm_folds():
    (ops0, names0, rep0, _), (ops1, names1, rep1, _) = _hooked("RVC_NO_LN_FUSE", "1", "full", 2, 1)
    assert "cv.pos.raw" in names0 and "cv.pos" in names1 and not any(n.endswith(".raw") for n in names1)
    assert ops1 > ops0 + 20, (ops0, ops1)            # 2 LayerNorm launches per layer and the two in front of them come back (+ the synthesizer's)
    rep0.done(); rep1.done()


@pytest.mark.parametrize("S", [1, 5])
def test_tiny_without_layernorm_folds(S):
    # the narrow model has nothing to fold (embed < 256): the hook must change NOTHING -- said here, not assumed: same stages, same launches
    (ops0, names0, rep0, _), (ops1, names1, rep1, _) = _hooked("RVC_NO_LN_FUSE", "1", "tiny", 2, S)
    assert names0 == names1 and ops0 == ops1 and "cv.pos" in names0, (ops0, ops1)
    rep0.done(); rep1.done()


# The fused ConvBlockRes needs the f0 branch on ONE XCD.  An engine whose ContentVec runs at most 9 layers gives it two up to 3 streams (configure_aux_streams:
# the v1 rule) -- `tiny` with its 2 layers is such an engine -- and beyond 4 streams there is no partition: on `tiny` the fused blocks and the poolings folded
# into them run at 4 streams only.  1 and 5 streams therefore assert what the hook still changes there (the head's layout) or that it changes nothing.
@pytest.mark.parametrize("S", [1, 4, 5])
def test_tiny_rmvpe_unfused_and_gru_input_kernel(S):
    # RVC_RM_FUSE = 0: no fused ConvBlockRes, and the head convolution writes an image that gru_input_kernel transposes: one more launch at any stream count,
    # and at 4 streams every fused block comes apart into its two or three launches as well
    (ops0, _, rep0, _), (ops1, _, rep1, _) = _hooked("RVC_RM_FUSE", 0, "tiny", 2, S)
    assert (ops1 > ops0 + 1) if S == 4 else (ops1 == ops0 + 1), (ops0, ops1)
    rep0.done(); rep1.done()


@pytest.mark.parametrize("S", [1, 4, 5])
def test_tiny_rmvpe_pooling_as_a_launch(S):
    # RVC_RM_FUSE = 3: fused blocks, but no pooling folded into them: avgpool2_kernel behind every encoder level.  Where no block is fused (1 and 5 streams)
    # every pooling is a launch already and the hook must change nothing
    (ops0, _, rep0, _), (ops1, _, rep1, _) = _hooked("RVC_RM_FUSE", 3, "tiny", 2, S)
    assert (ops1 > ops0) if S == 4 else (ops1 == ops0), (ops0, ops1)
    rep0.done(); rep1.done()


def test_full_rmvpe_pooling_as_a_launch():
    # ... and on the wide model at one stream (f0 on one XCD: fused blocks on the 16- and 32-channel levels, two poolings folded into them by default)
    (ops0, _, rep0, _), (ops1, _, rep1, _) = _hooked("RVC_RM_FUSE", 3, "full", 2, 1)
    assert ops1 == ops0 + 2, (ops0, ops1)
    rep0.done(); rep1.done()


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("kernel", ["one", "generic"])
def test_tiny_conv0_paths(S, kernel):
    # the rules pick the multi-channel kernel here (10 taps, an even channel count).  generic: convolution + groupnorm_gelu_kernel, one more launch;
    # one: the same launch count, but another reduction order over the 7167 outputs of a channel -- the tap cannot come back bit for bit
    (ops0, _, rep0, a), (ops1, _, rep1, b) = _hooked("RVC_CONV0_KERNEL", kernel, "tiny", 2, S)
    assert ops1 == ops0 + (1 if kernel == "generic" else 0), (ops0, ops1)
    assert a.shape == b.shape and not np.array_equal(a, b), "the hooked plan returned the default path's bits"
    rep0.done(); rep1.done()
