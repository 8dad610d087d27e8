"""The 32x32x2 body of the conv_tile family (conv_tile32_kernel, obs_rvc_amd/csrc/conv_tile.hip.h) against the fp64 definition, layer by layer
through rvc_debug_layer with the harness of test_gpu_layers.py (sentinel-filled allocations, layer_ref.py, the same bound TOL), forced with the test
hook RVC_CONV_TILE_MFMA = 32 together with RVC_CONV_TILE = 2 (short outputs eligible).  Every run checks the values, that every byte outside the
output interior comes back bit for bit, and that the family reported is `tile`; every run is repeated under the 16x16x4 body (hook = 16) and the
two bodies must agree within the same bound (not bitwise: the summation order differs).

Shapes: the decoder's fused ResBlock launch (three phases of kernel sizes 3 / 7 / 11 in one launch, halo 28) at the smallest sizes where the body can
go wrong -- Cout 32 / 64 / 128 and 48 (no multiple of 32: the last 16-row weight tile is clamped, the epilogue takes its guarded path), Cin 32 / 64 (one
and two staged channel blocks), output lengths that end inside a 32-column fragment (33), inside a tile (70) and one column into a third tile
(2 BN + 1), both tile sets (RVC_CONV_TILE_KS = 2: the half-height tiles with two K shares, 1: the waves split M then N), 1 / 2 / 4 streams."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_layers as TL
from common import rms, set_opt, voice_signal, zoo, BASELINE_160MS as g
from test_gpu_tiles import HOOKS, TOL

pytestmark = pytest.mark.gpu
DH, LR = TL.DH, TL.LR
MFMA = "RVC_CONV_TILE_MFMA"


def _bn(cout, ks):
    """columns of the 32x32x2 body's tile for a panel of `cout` rows (plan.hip queue_conv_tile32)"""
    if ks == 2:
        return 32 if cout > 32 else 64
    return 32 if cout > 64 else (64 if cout > 32 else 128)


def _multi(name, cout, cin, t, d, **kw):
    base = dict(form=2, cin=cin, cout=cout, n=3, kws=(3, 7, 11), dils=(d,) * 3, pads=tuple((k * d - d) // 2 for k in (3, 7, 11)), t_in=t, t_out=t, x_halo=DH,
                y_halo=DH, x_grouped=1, pre_act=LR, pre_slope=0.1)
    base.update(kw)
    return TL.Case("t32_%s_M%d_C%d_T%d_d%d" % (name, cout, cin, t, d), "model_synth.hip:204-228 (ResBlock chains)", **base)


def _variants(cout, cin, t):
    """(case, stream counts): the epilogue and operand forms of the decoder's launches"""
    return [
        # c1: input LeakyReLU + output LeakyReLU, dilations 1 / 3 / 5, shared and grouped input rows
        (_multi("c1_shared", cout, cin, t, 1, x_grouped=0, act=LR, slope=0.1), (1,)),
        (_multi("c1", cout, cin, t, 3, act=LR, slope=0.1), (1,)),
        (_multi("c1", cout, cin, t, 5, act=LR, slope=0.1), (1, 2, 4)),
        # c2: input LeakyReLU, NO output activation, residual grouped (one tensor per chain) and ungrouped (shared)
        (_multi("c2_resgrouped", cout, cin, t, 1, y_halo=0, r_halo=DH, res=1, res_grouped=1), (1,)),
        (_multi("c2_resshared", cout, cin, t, 1, r_halo=DH, res=1, res_grouped=0), (1,)),
        # the mean over the chains: scale 1 / 3 with the residual, and accumulated onto the previous output
        (_multi("scale", cout, cin, t, 1, r_halo=DH, res=1, scale=1.0 / 3), (1,)),
        (_multi("scale_acc", cout, cin, t, 3, r_halo=DH, res=1, scale=1.0 / 3, accumulate=1), (1, 2, 4)),
    ]


class _KeepOutput:
    """the library as test_gpu_layers.Layer sees it, keeping a copy of the output allocation of every rvc_debug_layer run"""

    def __init__(self, L):
        self._L, self.y, self.gy = L, None, None

    def __getattr__(self, name):
        return getattr(self._L, name)

    def rvc_debug_layer(self, h, s, w, b, x, y, r, geo):
        rc = self._L.rvc_debug_layer(h, s, w, b, x, y, r, geo)
        if y is not None:
            self.gy = list(geo[8:16])
            self.y = np.ctypeslib.as_array((C.c_float * self.gy[0]).from_address(y)).copy()
        return rc


@pytest.fixture(scope="module")
def layer():
    ly = TL.Layer()
    ly.L = _KeepOutput(ly.L)
    try:
        yield ly
    finally:
        for k in HOOKS + (MFMA,):
            set_opt(k, None)
        ly.close()


def _both_bodies(layer, case, streams, ks):
    """runs `case` under the 32x32x2 body and the 16x16x4 body; -> list of problems"""
    fails, ys = [], {}
    d = TL.data_for(case, streams)
    for body in ("32", "16"):
        set_opt("RVC_CONV_TILE", "2"); set_opt("RVC_CONV_TILE_KS", str(ks)); set_opt(MFMA, body)
        try:
            fam, bad = layer.run(case, streams)
        finally:
            for k in ("RVC_CONV_TILE", "RVC_CONV_TILE_KS", MFMA):
                set_opt(k, None)
        ys[body] = [layer.L.y[TL._y_index(case, layer.L.gy, streams, j)].astype(np.float64) for j in range(len(d.refs))]
        if fam != "tile":
            bad = bad + ["family %s, expected tile" % fam]
        fails += ["%s @ %d streams, ks %d, body %s: %s" % (case.name, streams, ks, body, b_) for b_ in bad]
    for j, (ref, scale) in enumerate(d.refs):
        e = float(np.max(np.abs(ys["32"][j] - ys["16"][j]))) / max(scale, 1e-30)
        if not e < TOL:
            fails.append("%s @ %d streams, ks %d: the two bodies differ by %.3e of rms on output %d" % (case.name, streams, ks, e, j))
    return fails


@pytest.mark.parametrize("cin", [32, 64])
@pytest.mark.parametrize("cout", [32, 64, 128, 48])
def test_resblock_launch_on_both_bodies(layer, cout, cin):
    fails = []
    for ks in (2, 1):
        for t in (33, 70, 2 * _bn(cout, ks) + 1):
            for case, stream_counts in _variants(cout, cin, t):
                for streams in stream_counts:
                    fails += _both_bodies(layer, case, streams, ks)
    assert not fails, "\n  ".join(fails[:40])


@pytest.mark.parametrize("cout", [32, 64, 128, 48])
def test_final_out_layer_on_both_bodies(layer, cout):
    # a one-phase layer that is the chunk's last (final_out: the launch may be redirected to the caller's buffer), Tanh epilogue, no bias
    fails = []
    for ks in (2, 1):
        for t in (33, 70, 2 * _bn(cout, ks) + 1):
            case = TL.Case("t32_final_M%d_T%d" % (cout, t), "model_synth.hip:247 (final_out)", cin=32, cout=cout, kw=7, pad=3, t_in=t, t_out=t, x_halo=DH,
                           pre_act=LR, pre_slope=0.01, act=TL.R.ACT_TANH, no_bias=1, final_out=1)
            for streams in (1, 2, 4):
                fails += _both_bodies(layer, case, streams, ks)
    assert not fails, "\n  ".join(fails[:40])


def test_ineligible_layers_keep_the_16x16x4_body(layer):
    # input channels in 16s but not in 32s, and a tap reach beyond the staging grid (64 columns): the hook asks for the new body, the planner
    # keeps the family's other body -- same family, same values
    fails = []
    for case in (TL.Case("t32_cin48", "planner fallback", cin=48, cout=64, kw=7, pad=3, t_in=70, t_out=70, x_halo=DH, y_halo=DH),
                 TL.Case("t32_reach70", "planner fallback", cin=32, cout=64, kw=11, pad=35, dil=7, t_in=150, t_out=150, x_halo=40, y_halo=DH)):
        fails += _both_bodies(layer, case, 1, 2)
    assert not fails, "\n  ".join(fails)


def test_one_stream_chunk_with_either_body():
    # end to end: the five-stage toy synthesizer has a 32-channel ResBlock stage (kernel sizes 3 / 7 / 11, dilations 1 / 3 / 5); the one-stream chunk
    # with the 32x32x2 body against the same chunk with the 16x16x4 body, PCM within the bound test_folded_layernorm_one_stream_full_size uses for
    # its comparison of two paths of one library (rms < 1e-5), and against the oracle within the PCM tolerance
    from oracle import oracle as O
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("tiny", 2, "tiny5")
    x = voice_signal(g.input_buffer_16k_size, seed=17)
    ora = O.OracleRvcInfer(z["data"]); ora.load_contentvec(2); ora.load_f0(1); ora.load_model(z["model"]); ora.set_noise_seed(4, 1)
    yo = ora.infer(x, 2560, 3, 200, 21)
    out = {}
    try:
        for body in ("32", "16"):
            set_opt("RVC_CONV_TILE", "2"); set_opt(MFMA, body)
            eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"]); eng.set_noise_seed(4, 1)
            out[body] = eng.infer(x, 2560, 3, 200, 21)
            eng.close()
    finally:
        set_opt("RVC_CONV_TILE", None); set_opt(MFMA, None)
    d = rms(out["32"] - out["16"])
    print("rms(32 - 16) = %.3e, rms(32 - oracle) = %.3e" % (d, rms(out["32"] - yo)))
    assert out["32"].shape == out["16"].shape == yo.shape
    assert not np.array_equal(out["32"], out["16"])          # two different bodies did run
    assert d < 1e-5 and rms(out["32"] - yo) < 1e-3 and rms(out["16"] - yo) < 1e-3
