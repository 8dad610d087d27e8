"""Every form of convolution layer the models build, one per production call site, through rvc_debug_layer (the planner calls and options the
models use) against the fp64 definitional reference of tests/layer_ref.py -- under the rules at several stream counts, under every choice the
autotuner can make (RVC_FORCE_CHOICE) and under the family hooks.  Each run checks
  * the values: max |gpu - ref| / rms < TOL, where rms is that of the largest addend when a residual or the accumulated output can cancel the
    convolution (residual, accumulate), else of the result;
  * that nothing else was written: the whole allocations of the input, residual and output tensors -- guard zones, halos, ld padding, other rows,
    other streams -- are pre-filled (the input halo with zeros, as in production, everything else with a sentinel) and must come back bit for bit;
  * which kernel family ran (rvc_debug_last_kernel): the set seen over all runs of a form must be the set the planner's eligibility rules
    (obs_rvc_amd/csrc/plan.hip) allow for it, so an eligible family that is never reached fails instead of passing silently."""
import ctypes as C
import zlib

import numpy as np
import pytest

import layer_ref as R
from common import set_opt
from debug_abi import Handle, LayerSpec, index, ptr, same_bits, stray
from test_gpu_tiles import CHOICES, HOOKS, TOL

pytestmark = pytest.mark.gpu

SENT_X, SENT_Y, SENT_R = np.float32(-7777.25), np.float32(5555.5), np.float32(3333.75)


class Case:
    """One layer form: spec fields (PyTorch-style parameters) + the interior lengths."""
    DEFAULTS = dict(form=0, cin=1, cout=1, kw=1, stride=1, pad=0, dil=1, groups=1, t_in=1, t_out=1, x_halo=0, y_halo=0, r_halo=0, act=0, slope=0.0,
                    scale=1.0, accumulate=0, pre_act=0, pre_slope=0.0, no_bias=0, final_out=0, glu=0, res=0, n=1, kws=(0,), dils=(0,), pads=(0,),
                    x_grouped=0, res_grouped=0, y_ws=0)

    def __init__(self, name, site, streams=(1, 2, 3, 6, 20), **kw):
        self.name, self.site, self.streams = name, site, streams
        self.p = dict(self.DEFAULTS, **kw)

    def spec(self, streams):
        s = LayerSpec()
        for k, v in self.p.items():
            if k in ("kws", "dils", "pads"):
                getattr(s, k)[:] = (list(v) + [0] * 4)[:4]
            else:
                setattr(s, k, v)
        s.streams = streams
        return s

    @property
    def one_by_one(self):
        """a table-free 1x1 layer (add_conv1d: KW = 1, one group, no padding, K a multiple of 16): the only layers igemm2w / igemm32l take"""
        p = self.p
        return p["form"] == 0 and p["kw"] == 1 and p["groups"] == 1 and p["pad"] == 0 and p["cin"] % 16 == 0 and not p["glu"]


# ------------------------------------------------------------------------------------------------------------------------------------------
# the forms (production channel counts, short ragged lengths; DH = 28: the decoder's halo for kernel 11 x dilation 5)
DH, LR = 28, R.ACT_LRELU
CASES = [
    Case("stem0", "model_cv.hip:51-53 (Cin 1, K 10, S 5)", cin=1, cout=512, kw=10, stride=5, t_in=5 * 36 + 10, t_out=37),
    Case("stem_gelu", "model_cv.hip:51-53 (K 3, S 2, GELU)", streams=(1, 2, 3, 6, 20, 64), cin=512, cout=512, kw=3, stride=2, t_in=75, t_out=37,
         act=R.ACT_GELU),
    Case("stem_gelu_k2", "model_cv.hip:51-53 (K 2, S 2, GELU)", cin=512, cout=512, kw=2, stride=2, t_in=75, t_out=37, act=R.ACT_GELU),
] + [
    Case("noise_sf%d" % sf, "model_synth.hip:185 (noise conv, accumulated)", cin=1, cout=co, kw=2 * sf, stride=sf, pad=sf // 2, t_in=t * sf, t_out=t,
         x_halo=sf + 2, y_halo=DH, accumulate=1)
    # (40 / 4 / 12: the v2 48k and 40k layouts; 48 / 32 / 8 / 2: the first two, a middle and the fourth stage of the v1 48k / v1 32k / v2 32k layouts)
    for (sf, co, t) in ((40, 256, 70), (4, 64, 1403), (12, 128, 250), (48, 256, 70), (32, 256, 70), (8, 128, 701), (2, 32, 1403))
] + [
    Case("noise_last_c16", "model_synth.hip:344 (last stage's noise conv: one tap onto 16 channels, accumulated)", cin=1, cout=16, kw=1, t_in=1601, t_out=1601,
         x_halo=3, y_halo=DH, accumulate=1),
] + [
    Case("pos_T%d" % t, "model_cv.hip:73 (grouped, Tout = T + 1 dropped)", cin=768, cout=768, kw=128, pad=64, groups=16, t_in=t, t_out=t, x_halo=64,
         act=R.ACT_GELU, res=4)
    for t in (48, 37)
] + [
    Case("convT_%d_%d%s%s" % (k, s, "_to16" if ci == 32 else "", "_res" if res else ""), "model_synth.hip:180-183 (polyphase ConvTranspose1d)", form=1, cin=ci, cout=ci // 2, kw=k, stride=s,
         pad=(k - s) // 2, t_in=t, t_out=(t - 1) * s - (k - s) + k, x_halo=DH, y_halo=DH, pre_act=LR, pre_slope=0.1, res=res)
    # (16 / 4 and 16 / 6: four and three taps per phase, the second stages of the v1 32k / v1 48k layouts; 4 / 2 from 32 channels: their fifth stage, 32 -> 16)
    for (k, s, ci, t) in ((24, 12, 512, 9), (20, 10, 512, 11), (16, 10, 512, 7), (16, 8, 256, 13), (8, 4, 256, 21), (7, 3, 64, 45), (4, 2, 128, 99),
                          (16, 4, 256, 21), (16, 6, 256, 13), (4, 2, 32, 99))
    for res in (0, 1)
] + [
    Case("multi_c1_%s_C%d_d%d" % ("grouped" if xg else "shared", co, d), "model_synth.hip:204 (ResBlock c1, fused chains)", form=2, cin=co, cout=co, n=3,
         kws=(3, 7, 11), dils=(d,) * 3, pads=tuple((k * d - d) // 2 for k in (3, 7, 11)), t_in=t, t_out=t, x_halo=DH, y_halo=DH, x_grouped=xg,
         pre_act=LR, pre_slope=0.1, act=LR, slope=0.1)
    for (co, t) in ((128, 203), (32, 1601), (16, 1601)) for (xg, d) in ((0, 1), (1, 3), (1, 5))
] + [
    Case("multi_c2_res%s_C%d" % ("grouped" if rg else "shared", co), "model_synth.hip:208 (ResBlock c2 + residual, fused chains)", form=2, cin=co, cout=co,
         n=3, kws=(3, 7, 11), dils=(1, 1, 1), pads=(1, 3, 5), t_in=t, t_out=t, x_halo=DH, y_halo=0 if rg else DH, r_halo=DH, x_grouped=1, res=1,
         res_grouped=rg)
    for (co, t) in ((128, 203), (64, 797), (16, 1601)) for rg in (0, 1)
] + [
    Case("pair", "model_synth.hip:138 (post + next pre, add_conv1d_two)", form=3, cin=768, cout=192, n=2, t_in=21, t_out=21, x_halo=4, y_halo=4),
    Case("pair_T37", "model_synth.hip:138 (post + next pre, add_conv1d_two)", form=3, cin=768, cout=192, n=2, t_in=37, t_out=37, x_halo=4, y_halo=4),
    Case("glu", "model_synth.hip:146 (WaveNet in-layer, gated)", cin=192, cout=384, kw=5, pad=2, t_in=37, t_out=37, x_halo=4, glu=1),
    Case("glu_composed", "model_synth.hip:137 (composed in-layer, gated)", cin=16 + 192 * 2, cout=384, kw=5, pad=2, t_in=21, t_out=21, x_halo=4, y_halo=4,
         glu=1),
    Case("rs_accumulate", "model_synth.hip:147-149 (res_skip, accumulate)", cin=192, cout=384, t_in=37, t_out=37, y_halo=4, accumulate=1),
    Case("post_scale_m1", "model_synth.hip:151 (post, scale -1, accumulate)", cin=192, cout=96, t_in=37, t_out=37, x_halo=4, y_halo=4, scale=-1.0,
         accumulate=1),
    Case("rb_mean_first", "model_synth.hip:228 (chain 0: x 1/n_rb)", cin=128, cout=128, kw=7, pad=3, t_in=203, t_out=203, x_halo=DH, y_halo=DH,
         r_halo=DH, res=1, scale=1.0 / 3),
    Case("rb_mean_acc", "model_synth.hip:228 (chain j > 0: x 1/n_rb, accumulate)", cin=128, cout=128, kw=11, pad=5, t_in=203, t_out=203, x_halo=DH,
         y_halo=DH, r_halo=DH, res=1, scale=1.0 / 3, accumulate=1),
    Case("rb_mean_first_c16", "model_synth.hip:228 (chain 0 of a five-stage decoder's last stage)", cin=16, cout=16, kw=7, pad=3, t_in=1601, t_out=1601, x_halo=DH,
         y_halo=DH, r_halo=DH, res=1, scale=1.0 / 3),
    Case("rb_mean_acc_c16", "model_synth.hip:228 (chain j > 0 of a five-stage decoder's last stage)", cin=16, cout=16, kw=11, pad=5, t_in=1601, t_out=1601,
         x_halo=DH, y_halo=DH, r_halo=DH, res=1, scale=1.0 / 3, accumulate=1),
    Case("ff1_relu", "model_synth.hip:97 (ReLU, 3 taps)", cin=192, cout=768, kw=3, pad=1, t_in=21, t_out=21, x_halo=4, y_halo=4, act=R.ACT_RELU),
    Case("ff2_res_self", "model_synth.hip:98 (residual = output tensor)", cin=768, cout=192, kw=3, pad=1, t_in=21, t_out=21, x_halo=4, y_halo=4, res=3),
    Case("dec_post_tanh", "model_synth.hip:247 (pre-LReLU 0.01, Tanh, no bias, final_out)", streams=(1, 2, 3, 6, 20, 64), cin=32, cout=1, kw=7, pad=3,
         t_in=4001, t_out=4001, x_halo=DH, pre_act=LR, pre_slope=0.01, act=R.ACT_TANH, no_bias=1, final_out=1),
    Case("dec_post_tanh_c16", "model_synth.hip:247 (behind a five-stage decoder: 16 channels, K = 112)", streams=(1, 2, 3, 6, 20, 64), cin=16, cout=1, kw=7,
         pad=3, t_in=4001, t_out=4001, x_halo=DH, pre_act=LR, pre_slope=0.01, act=R.ACT_TANH, no_bias=1, final_out=1),
    Case("fc_sigmoid", "model_rmvpe.hip:259 (Sigmoid)", cin=512, cout=360, t_in=37, t_out=37, act=R.ACT_SIGMOID),
    Case("cv_ff1_gelu", "model_cv.hip:119 (GELU)", streams=(1, 2, 3, 6, 20, 64), cin=768, cout=3072, t_in=37, t_out=37, act=R.ACT_GELU),
    Case("knn_bcast_res", "retrieval.hip:104 (broadcast residual, scale -2, no bias)", cin=768, cout=48, t_in=1001, t_out=1001, res=2, scale=-2.0,
         no_bias=1),
    Case("cnn_transposed", "model_rmvpe.hip:218 (Conv2d 3x3, output transposed)", form=4, cin=16, cout=3, t_in=37, t_out=128, y_ws=1),
    # K = 16384: the offset table (64 KiB) exceeds the 60 KiB of LDS the kernels give it, so the layer runs as two grid-level K splits of 512 chunks whose
    # partial sums splitk_epilogue_kernel finishes (plan.hip queue_reg).  M = 20 leaves a partial second row of 16 x 16 tiles, N = 37 a partial third column.
    Case("splitk", "model_crepe.hip (long-K layers: table too long for LDS, two-stage split-K)", streams=(1, 3), cin=1024, cout=20, kw=16, pad=8, t_in=37,
         t_out=37, x_halo=8),
    Case("splitk_pre_res_acc", "model_crepe.hip (the same, fused input LeakyReLU and every term of the second stage's epilogue)", streams=(1, 3), cin=1024,
         cout=20, kw=16, pad=8, t_in=37, t_out=37, x_halo=8, r_halo=4, pre_act=LR, pre_slope=0.1, res=1, accumulate=1, scale=1.0 / 3, act=LR, slope=0.1),
]
SPLITK = [c for c in CASES if c.name.startswith("splitk")]
# full-length production shapes, under the rules only
FULL = [
    Case("full_stem_gelu", "model_cv.hip:51-53", streams=(1, 64), cin=512, cout=512, kw=3, stride=2, t_in=447, t_out=223, act=R.ACT_GELU),
    Case("full_pos", "model_cv.hip:73", streams=(1, 8), cin=768, cout=768, kw=128, pad=64, groups=16, t_in=111, t_out=111, x_halo=64, act=R.ACT_GELU, res=4),
    Case("full_convT_10_10", "model_synth.hip:180-183", streams=(1, 16), form=1, cin=512, cout=256, kw=16, stride=10, pad=3, t_in=21, t_out=210, x_halo=DH,
         y_halo=DH, pre_act=LR, pre_slope=0.1, res=1),
    Case("full_multi_c1", "model_synth.hip:204", streams=(1, 8), form=2, cin=64, cout=64, n=3, kws=(3, 7, 11), dils=(3, 3, 3), pads=(3, 9, 15), t_in=4200,
         t_out=4200, x_halo=DH, y_halo=DH, x_grouped=1, pre_act=LR, pre_slope=0.1, act=LR, slope=0.1),
    Case("full_dec_post", "model_synth.hip:247", streams=(1, 64), cin=32, cout=1, kw=7, pad=3, t_in=8400, t_out=8400, x_halo=DH, pre_act=LR, pre_slope=0.01,
         act=R.ACT_TANH, no_bias=1, final_out=1),
]


# ------------------------------------------------------------------------------------------------------------------------------------------
# data and the fp64 reference (computed once per (form, streams): the forced choice does not change it)
def _rng(case, streams):
    return np.random.default_rng(zlib.crc32(("%s/%d" % (case.name, streams)).encode()))


def _weights(case, rng):
    p = case.p
    f = p["form"]
    if f == 0:
        shape = [(p["cout"], p["cin"] // p["groups"], p["kw"])]
    elif f == 1:
        shape = [(p["cin"], p["cout"], p["kw"])]
    elif f == 2:
        shape = [(p["cout"], p["cin"], k) for k in p["kws"][:p["n"]]]
    elif f == 3:
        shape = [(p["cout"], p["cin"], 1)] * 2
    else:
        shape = [(p["cout"], p["cin"], 3, 3)]
    ws = [rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(np.prod(s[1:]))) for s in shape]
    nb = p["cout"] * (2 if f == 3 else (p["n"] if f == 2 else 1))
    b = None if p["no_bias"] else rng.uniform(-0.1, 0.1, nb).astype(np.float32)
    return ws, b


def conv_of(case, xin, ws, j):
    """the convolution of output tensor j in fp64, without its bias: linear in the (activated) input xin and in the weights ws"""
    p = case.p
    f = p["form"]
    if f == 0:
        return R.conv1d(xin, ws[0], None, p["stride"], p["pad"], p["dil"], p["groups"])[:, :, :p["t_out"]]      # (Tout = T + 1: the last column is dropped)
    if f == 1:
        return R.conv_transpose1d(xin, ws[0], None, p["stride"], p["pad"])
    if f == 2:
        xj = xin[:, j * p["cin"]:(j + 1) * p["cin"]] if p["x_grouped"] else xin
        return R.conv1d(xj, ws[j], None, 1, p["pads"][j], p["dils"][j])
    if f == 3:
        return R.conv1d(xin, ws[j], None)
    return R.conv2d_3x3(xin, ws[0], None)


def finish(case, d, convs):
    """the layer's epilogue in fp64 on convs[j] (conv_of) -> per output tensor: (value, rms of the largest addend)"""
    p = case.p
    f = p["form"]
    refs = []
    for j, a in enumerate(convs):
        if d.b is not None:
            a = a + d.b[j * p["cout"]:(j + 1) * p["cout"]].astype(np.float64).reshape((1, -1) + (1,) * (a.ndim - 2))
        if p["glu"]:
            v = R.glu_gate(a)
            assert v.shape == d.y0[j].shape, (case.name, v.shape, d.y0[j].shape)
            refs.append((v, R_rms(v)))
            continue
        assert a.shape == d.y0[j].shape, (case.name, a.shape, d.y0[j].shape)
        v = R.act(a, p["act"], p["slope"])
        addends = [v]
        if p["res"] == 1:
            rr = d.r[:, j * p["cout"]:(j + 1) * p["cout"]] if (f == 2 and p["res_grouped"]) else d.r[:, :p["cout"]]
            addends.append(rr.astype(np.float64))
        elif p["res"] == 2:
            addends.append(np.broadcast_to(d.r.astype(np.float64), v.shape))
        elif p["res"] == 3:
            addends.append(d.y0[j].astype(np.float64))
        elif p["res"] == 4:
            addends.append(d.x.astype(np.float64)[:, :p["cout"], :p["t_out"]])
        v = sum(addends) * p["scale"]
        addends = [a_ * abs(p["scale"]) for a_ in addends]
        if p["accumulate"]:
            addends.append(d.y0[j].astype(np.float64))
            v = v + d.y0[j]
        refs.append((v, max([R_rms(v)] + [R_rms(a_) for a_ in addends])))
    return refs


class Data:
    pass


_CACHE = {}


def data_for(case, streams):
    key = (case.name, streams)
    if key in _CACHE:
        return _CACHE[key]
    p, B = case.p, streams
    rng = _rng(case, streams)
    d = Data()
    d.ws, d.b = _weights(case, rng)
    f = p["form"]
    xrows = p["cin"] * (p["n"] if f == 2 and p["x_grouped"] else 1)
    if f == 4:
        d.x = rng.uniform(-1, 1, (B, p["cin"], p["t_in"], p["t_out"])).astype(np.float32)
    else:
        d.x = rng.uniform(-1, 1, (B, xrows, p["t_in"])).astype(np.float32)
    outs = p["cout"] // 2 if p["glu"] else p["cout"]
    n_out = 2 if f == 3 else (p["n"] if f == 2 else 1)
    oshape = (B, outs, p["t_in"], p["t_out"]) if f == 4 else (B, outs, p["t_out"])
    d.y0 = [rng.uniform(-1, 1, oshape).astype(np.float32) for _ in range(n_out)]
    d.r = None
    if p["res"] == 1:
        rrows = p["cout"] * (p["n"] if f == 2 and p["res_grouped"] else 1)
        d.r = rng.uniform(-1, 1, (B, rrows) + oshape[2:]).astype(np.float32)
    elif p["res"] == 2:
        d.r = rng.uniform(-1, 1, (p["t_out"],)).astype(np.float32)
    xin = R.act(d.x, p["pre_act"], p["pre_slope"]) if p["pre_act"] else d.x.astype(np.float64)
    d.refs = finish(case, d, [conv_of(case, xin, d.ws, j) for j in range(n_out)])
    for k in [k for k in _CACHE if k[0] != case.name]:
        del _CACHE[k]           # (one form at a time: the cache only has to outlive the runs of one form)
    _CACHE[key] = d
    return d


def R_rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a)))


# ------------------------------------------------------------------------------------------------------------------------------------------
# tensor allocations: geo = (size, offset of element 0, C, T (2-D: W), ld, bs, cs, H) (debug_abi.index)
def _y_index(case, g, B, j):
    """element offsets of output tensor j's interior ([B][C][T] or [B][C][H][W])"""
    p = case.p
    f = p["form"]
    if f == 4 and p["y_ws"]:
        # transposed image: (b, o, h, w) at row o * W + w, column h
        H, W = p["t_in"], p["t_out"]
        o, h, w = np.meshgrid(np.arange(p["cout"]), np.arange(H), np.arange(W), indexing="ij")
        return g[1] + np.arange(B)[:, None, None, None] * g[5] + ((o * W + w) * g[4] + h)[None]
    if f == 4:
        return index(g, B, 0, p["cout"], p["t_out"], H=p["t_in"])
    if f == 3:
        return index(g, B, 16 + 2 * p["cout"] * j, p["cout"], p["t_out"])
    if f == 2:
        return index(g, B, j * p["cout"], p["cout"], p["t_out"])
    return index(g, B, 0, p["cout"] // 2 if p["glu"] else p["cout"], p["t_out"])


class Layer(Handle):
    def run(self, case, streams, tol=TOL):
        """-> (family, list of problems); self.errors = max err / rms of every output tensor (tol: the bound on it, for a family that does not compute in fp32)"""
        p, B = case.p, streams
        d = data_for(case, streams)
        s = case.spec(streams)
        geo = (C.c_longlong * 24)()
        assert self.L.rvc_debug_layer(self.h, C.byref(s), None, None, None, None, None, geo) == 0
        gx, gy, gr = list(geo[0:8]), list(geo[8:16]), list(geo[16:24])
        f = p["form"]
        # input: sentinel, the whole row of every channel zero (halo and interior), then the interior
        x = np.full(gx[0], SENT_X, np.float32)
        if f == 4:
            x[index(gx, B, 0, gx[2], gx[3] + 2, H=gx[7] + 2) - gx[4] - 1] = 0.0
            x[index(gx, B, 0, p["cin"], p["t_out"], H=p["t_in"])] = d.x
        else:
            x[index(gx, B, 0, gx[2], gx[3] + 2 * p["x_halo"]) - p["x_halo"]] = 0.0
            x[index(gx, B, 0, gx[2], gx[3])] = d.x
        y = np.full(gy[0], SENT_Y, np.float32)
        yidx = [_y_index(case, gy, B, j) for j in range(len(d.refs))]
        for j, yi in enumerate(yidx):
            if p["accumulate"] or p["res"] == 3:
                y[yi] = d.y0[j]
        r = None
        if p["res"] == 1:
            r = np.full(gr[0], SENT_R, np.float32)
            r[index(gr, B, 0, gr[2], gr[3], H=gr[7] if f == 4 else None)] = d.r
        elif p["res"] == 2:
            r = np.full(gr[0], SENT_R, np.float32)
            r[index(gr, 1, 0, 1, gr[3])] = d.r
        x0, y0, r0 = x.copy(), y.copy(), None if r is None else r.copy()
        wcat = np.concatenate([w_.ravel() for w_ in d.ws])
        rc = self.L.rvc_debug_layer(self.h, C.byref(s), ptr(wcat), ptr(d.b), ptr(x), ptr(y), ptr(r), geo)
        if rc != 0:
            return "?", ["rvc_debug_layer failed (%d): %s" % (rc, self.last_error())]
        fam = self.last_kernel()
        self.outputs = [y[yi] for yi in yidx]          # (the interiors of this run's output tensors, for the tests that compare bits)
        bad = []
        self.errors = []
        if not same_bits(x, x0):
            bad.append("input tensor changed at %d positions" % int(np.count_nonzero(x.view(np.uint32) != x0.view(np.uint32))))
        if r is not None and not same_bits(r, r0):
            bad.append("residual tensor changed")
        pos = stray(y, y0, yidx)
        if pos.size:
            col = (pos - gy[1]) % gy[4] if f != 4 else pos
            bad.append("%d floats written outside the output's interior (first at offset %d, row column %d; ld %d, T %d)" %
                       (pos.size, pos[0] - gy[1], int(col[0]), gy[4], gy[3]))
        for j, (ref, scale) in enumerate(d.refs):
            got = y[yidx[j]].astype(np.float64)
            e = float(np.max(np.abs(got - ref))) / max(scale, 1e-30) if np.all(np.isfinite(got)) else np.inf
            self.errors.append(e)
            if not e < tol:
                wi = np.unravel_index(int(np.argmax(np.abs(got - ref))), ref.shape)
                bad.append("output %d: max err / rms %.3e at %s (gpu %.6g, ref %.6g)" % (j, e, wi, got[wi], ref[wi]))
        return fam, bad


@pytest.fixture(scope="module")
def layer():
    ly = Layer()
    try:
        yield ly
    finally:
        for k in HOOKS:
            set_opt(k, None)
        ly.close()


def _fits(cin_k, cfg, ks):
    """plan.hip queue_reg fits(): the register-direct tiles / K splits the planner can build for a layer with K = cin_k"""
    kmf, knf = (1, 1, 1, 2, 2), (1, 2, 4, 2, 4)
    nchunks = (cin_k + 15) // 16
    return (ks == 1 or (nchunks // ks >= 4 and ks * kmf[cfg] * knf[cfg] <= 32)) and nchunks * 64 + (ks * kmf[cfg] * knf[cfg] * 1024 if ks > 1 else 0) <= 60 * 1024


def _k_of(case):
    p = case.p
    f = p["form"]
    if f == 1:
        return p["cin"] * -(-p["kw"] // p["stride"])
    if f == 2:
        return p["cin"] * max(p["kws"][:p["n"]])
    if f == 4:
        return p["cin"] * 9
    return p["cin"] // p["groups"] * p["kw"]


def runs_of(case):
    """(label, streams, {hook: value}) of every run of a form"""
    out = [("rules", s, {}) for s in case.streams]
    out += [("choice %d,%d,%d" % c, s, {"RVC_FORCE_CHOICE": "%d,%d,%d" % c}) for c in CHOICES for s in (6, 20)]
    out += [("conv_tile", s, {"RVC_CONV_TILE": "2"}) for s in (1, 3)]
    out += [("conv32s", 1, {"RVC_CONV32S": "2"})]
    out += [("cfg %d,%d" % (cf, ks), 1, {"RVC_FORCE_CFG": "%d,%d" % (cf, ks)}) for cf in range(5) for ks in (1, 4, 8, 16) if _fits(_k_of(case), cf, ks)]
    if case.one_by_one:
        out += [("g2w %d,%d" % (t, ks), 1, {"RVC_FORCE_G2W": "%d,%d" % (t, ks)}) for t in range(3) for ks in (1, 2, 4, 8)]
    return out


# kernel families each form must reach over its runs -- the planner's eligibility rules (plan.hip) for these shapes:
#   reg   (igemm2) takes every layer;
#   g32   (igemm32, choice 3 / the many-stream rules) needs >= 2 chunks of K, no gate, no per-phase epilogue, an offset table that fits in LDS;
#   g32t  one-phase layers with a table at one stream (after the fold), no gate;  g32l / g2w: table-free 1x1 layers only;
#   lds   (16x16x4 LDS kernel) only panels of >= 2048 or <= 64 rows with >= 384 workgroups -- of these shapes the 3072-row projection;
#   tile  (conv_tile) / c32s (conv32s): stride-1 1-D layers with a table, input channels per phase in 16s / 32s, no gate, no per-phase output; tile
#         also needs its staged rows within 100 KB of LDS (not the 768-channel 3-tap layer) and c32s a tap reach <= 64 (not the positional conv)
# 16 channels (the fifth stage of the v1 48k / v1 32k decoders, 512 >> 5) are outside every family but reg:
#   c32s  decode_taps(.., kC32sCB = 32) refuses 16 input channels (queue_conv32s);
#   tile  16 is a multiple of 16, and the LDS budget holds, but queue_conv_tile splits K over two waves ("every K share needs a chunk": cin / 16 >= kshares = 2,
#         the production value of RVC_CONV_TILE_KS, which runs_of leaves alone): one 16-channel group cannot be shared, so the family declines;
#   g32 / g32t  a 16-row weight panel has no tile (queue_tiled: bm = 0 unless M > 16; a forced choice needs M >= 17) -- the ResBlock convolutions (16 -> 16), the
#         transposed conv 32 -> 16 and the one-tap noise conv onto 16 channels alike; the last layer behind them has one row.
# Noise convs with K = 2 sf <= 16 (sf 8, 2, the one-tap last stage) are one chunk of K: reg only, as noise_sf4 (g32 needs two chunks).
# Never: strided layers on tile / c32s (the stem, the noise convs), the polyphase transposed conv on tile / c32s (its table walks taps backwards, its
# output columns are strided), the pair launch (per-phase activation and output tensor) and the gated in-layer on anything but reg; the 1-row
# weight panel of the decoder's last layer on the tiled kernels (fewer than 17 rows); the RMVPE head (3 rows, 2-D) on anything but reg.
# K = 16384 (splitk*): the offset table is 64 KiB, over the 60 KiB every family that keeps it in LDS allows -- g32 / g32t / lds (queue_tiled), every tile and K
# split of reg (queue_reg fits(): no RVC_FORCE_CFG run, and a forced choice 4,cfg,ks falls back to the rules), and the streams are not folded into N.  What is
# left under the rules, at every stream count, is reg's two-stage grid-level split-K (16 x 16 tiles, partial sums, splitk_epilogue_kernel; the batch stays a
# grid dimension): the forced-choice runs at 6 and 20 streams land there too, except the conv32s choices (1,*,*), which take the layer -- a stride-1 1-D
# convolution of 1024 = 32 x 32 channels with a tap reach of 15, no table in LDS -- as does RVC_CONV32S = 2 at one stream.  conv_tile declines: its staged rows
# (1024 channels x 79 columns) need 316 KB of LDS.  That the rules' runs really are the two-stage path is asserted in test_long_k_layer_runs_the_two_stage_split_k.
_STRIDED_TAB = {"reg", "g32", "g32t"}
_TAPS = {"reg", "g32", "g32t", "tile", "c32s"}
_ONE_BY_ONE = {"reg", "g32", "g32l", "g2w", "c32s"}
EXPECTED = dict(
    {"noise_sf48": _STRIDED_TAB, "noise_sf32": _STRIDED_TAB, "noise_sf8": {"reg"}, "noise_sf2": {"reg"}, "noise_last_c16": {"reg"}, "rb_mean_first_c16": {"reg"},
     "rb_mean_acc_c16": {"reg"}, "dec_post_tanh_c16": {"reg"},
     "stem0": {"reg"}, "stem_gelu": _STRIDED_TAB, "stem_gelu_k2": _STRIDED_TAB, "noise_sf40": _STRIDED_TAB, "noise_sf4": {"reg"},      # (K = 8: one chunk)
     "noise_sf12": _STRIDED_TAB, "pos_T48": {"reg", "tile"}, "pos_T37": {"reg", "tile"}, "pair": {"reg"}, "pair_T37": {"reg"}, "glu": {"reg"},
     "glu_composed": {"reg"}, "rs_accumulate": _ONE_BY_ONE, "post_scale_m1": _ONE_BY_ONE, "rb_mean_first": _TAPS, "rb_mean_acc": _TAPS, "ff1_relu": _TAPS,
     "ff2_res_self": _TAPS - {"tile"}, "dec_post_tanh": {"reg", "tile", "c32s"}, "fc_sigmoid": _ONE_BY_ONE, "cv_ff1_gelu": _ONE_BY_ONE | {"lds"},
     "knn_bcast_res": _ONE_BY_ONE, "cnn_transposed": {"reg"}, "splitk": {"reg", "c32s"}, "splitk_pre_res_acc": {"reg", "c32s"}},
    **{c.name: {"reg", "g32"} if c.p["cout"] > 16 else {"reg"} for c in CASES if c.p["form"] == 1},
    **{c.name: {"reg", "g32", "tile", "c32s"} if c.p["cout"] > 16 else {"reg"} for c in CASES if c.p["form"] == 2})


def _check(layer, case, runs):
    seen, fails = set(), []
    for (label, streams, hooks) in runs:
        for k, v in hooks.items():
            set_opt(k, v)
        try:
            fam, bad = layer.run(case, streams)
        finally:
            for k in hooks:
                set_opt(k, None)
        seen.add(fam)
        fails += ["%s @ %d streams [%s]: %s" % (label, streams, fam, b_) for b_ in bad]
    return seen, fails


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_layer_form(layer, case):
    seen, fails = _check(layer, case, runs_of(case))
    want = EXPECTED.get(case.name)
    assert not fails and seen == want, "%s (%s): families seen %s, expected %s\n  %s" % (case.name, case.site, sorted(seen), want, "\n  ".join(fails[:40]))


@pytest.mark.parametrize("case", FULL, ids=lambda c: c.name)
def test_full_length_layer_under_the_rules(layer, case):
    seen, fails = _check(layer, case, [("rules", s, {}) for s in case.streams])
    assert not fails, "%s (%s):\n  %s" % (case.name, case.site, "\n  ".join(fails))


@pytest.mark.parametrize("case", SPLITK, ids=lambda c: c.name)
def test_long_k_layer_runs_the_two_stage_split_k(layer, case):
    """Under the rules a layer whose offset table cannot fit in LDS is the register-direct family's grid-level split-K: the launch description says how many
    K splits wrote partial sums ("split=2": 1024 chunks in two slices of 512), on 16 x 16 tiles without the in-workgroup K split.  Values, stray writes: as
    every run.  The CRC32 of the output is printed: the path sums K in a fixed order, so the same library gives the same bits on every run."""
    for streams in case.streams:
        fam, bad = layer.run(case, streams)
        desc = layer.last_desc()
        print("%s @ %d streams: crc32 %08x  [%s]" % (case.name, streams, zlib.crc32(np.ascontiguousarray(layer.outputs[0]).tobytes()), desc))
        assert not bad, (case.name, streams, bad)
        f = dict(w.split("=", 1) for w in desc.split()[1:] if "=" in w)
        assert fam == "reg" and f["split"] == "2" and f["tile"] == "16x16" and f["ks"] == "1" and f["B"] == str(streams) and f["K"] == "16384", desc
