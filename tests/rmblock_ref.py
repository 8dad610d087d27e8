"""Float64 definition of one ConvBlockRes of RMVPE and of AvgPool2d(2, 2), a restatement of the planner's rule for which kernel
runs a block (obs_rvc_amd/csrc/model_rmvpe.hip: add_rm_block_fused, add_res_block), and the cases and data of tests/test_gpu_rmblock.py -- kept here so that
tests/test_rmblock_ref.py can measure, on the CPU and on exactly those inputs, what single precision alone costs.

    y1  = ReLU(conv3x3(x, w1) + b1)            zero padding of x
    y2  = ReLU(conv3x3(y1, w2) + b2)           zero padding of y1 ITSELF: outside the image y1 is 0, not ReLU(b1)
    out = y2 + (wsc . x + bsc | x)             1x1 shortcut, or the identity when there is none (cin = cout)

The convolution is tests/layer_ref.py's direct loop over the taps; nothing here knows about tiles, halos or fragment orders."""
import zlib
from collections import namedtuple

import numpy as np

from layer_ref import conv2d_3x3

# max |gpu - ref| / rms(ref) per stream: the project's convolution tolerance (tests/test_gpu_tiles.py: fp32 accumulation over K <= 5632; here K <= 9 x 128 +
# 9 x 64 + 128), accepted on the condition that single precision alone stays below a quarter of it on these inputs (tests/test_rmblock_ref.py)
TOL = 2e-5


def block(x, w1, b1, w2, b2, wsc=None, bsc=None):
    """x [B][cin][H][W] -> [B][cout][H][W], float64"""
    x = np.asarray(x, np.float64)
    y1 = np.maximum(conv2d_3x3(x, w1, b1), 0.0)
    y2 = np.maximum(conv2d_3x3(y1, w2, b2), 0.0)
    if wsc is None:
        assert x.shape[1] == y2.shape[1]
        return y2 + x
    return y2 + np.einsum("oc,bchw->bohw", np.asarray(wsc, np.float64), x) + np.asarray(bsc, np.float64)[None, :, None, None]


def avgpool2(x):
    """AvgPool2d(2, 2): [B][C][H][W] -> [B][C][H // 2][W // 2] (an odd last row / column is dropped, as PyTorch drops it)"""
    x = np.asarray(x, np.float64)
    H2, W2 = x.shape[2] // 2, x.shape[3] // 2
    v = x[:, :, :2 * H2, :2 * W2]
    return 0.25 * (v[:, :, 0::2, 0::2] + v[:, :, 0::2, 1::2] + v[:, :, 1::2, 0::2] + v[:, :, 1::2, 1::2])


def block_f32(x, w1, b1, w2, b2, wsc=None, bsc=None, pool_in=False):
    """the same chain in single precision (torch float32 on the CPU), pooling first if asked: what fp32 arithmetic alone does to these inputs"""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    with torch.no_grad():
        xx = t(x)
        if pool_in:
            xx = F.avg_pool2d(xx, 2, 2)
        y = F.relu(F.conv2d(xx, t(w1), t(b1), padding=1))
        y = F.relu(F.conv2d(y, t(w2), t(b2), padding=1))
        y = y + (xx if wsc is None else F.conv2d(xx, t(wsc)[:, :, None, None], t(bsc)))
        return y.numpy(), F.avg_pool2d(y, 2, 2).numpy() if min(y.shape[2:]) >= 2 else None


# ------------------------------------------------------------------------------------------------------------------------------------------
# which kernel runs a block: add_rm_block_fused's eligibility, restated
def _stride(n):
    """LDS channel stride: >= n and 16 mod 32"""
    v = n // 32 * 32 + 16
    return v + 32 if v < n else v


def fused_tile(cin, cout, H, W, has_sc, rm_fuse=True, hook=None, pool_out=False):
    """None when rm_block_kernel does not take the block, else (MT, NT1, NT2, TH, TW, LDS bytes).  hook: the value of RVC_RM_FUSE (None: not set)"""
    mode = 1 if hook is None else int(hook)
    if cout not in (16, 32) or cin > 64:                  # no fragment panels are packed (64 output channels: never fused)
        return None
    if mode == 0 or (not rm_fuse and mode != 2):
        return None
    if not has_sc and cin != cout:
        return None
    MT = cout // 16
    TH, TW = (8, 16) if MT == 1 else (4, 8)               # output tile of a workgroup, clamped to the image
    TH, TW = min(TH, H), min(TW, W)
    NT1, NT2, NWN = (3, 2, 4) if MT == 1 else (2, 1, 2)   # n-tiles of 16 pixels per wave in the two convolutions; waves that share an m panel
    if -(-(TH + 2) * (TW + 2) // 16) > NT1 * NWN or -(-TH * TW // 16) > NT2 * NWN or (TH + 4) * (TW + 4) > 256:
        return None                                       # (the 256 threads stage one tile position each)
    c16 = -(-cin // 16) * 16
    if -(-(9 * c16 * cout + 9 * cout * cout + (c16 * cout if has_sc else 0)) // 32) > 1536:      # 128-byte lines of the panels
        return None
    lds = (c16 * _stride((TH + 4) * (TW + 4)) + cout * _stride((TH + 2) * (TW + 2))) * 4
    if lds > 64 * 1024:
        return None
    if pool_out and (TW != 8 or TH % 2 or H % 2 or W % 2):
        return None
    return MT, NT1, NT2, TH, TW, lds


def expected_kernel(cin, cout, H, W, streams, has_sc, rm_fuse=True, hook=None, pool_in=False, pool_out=False, y_in_cat=False):
    """what rvc_debug_last_kernel must say after the block was queued"""
    fold = (1 if hook is None else int(hook)) != 3        # RVC_RM_FUSE = 3: no pooling folded into a block
    t = fused_tile(cin, cout, H, W, has_sc, rm_fuse, hook)
    if t:
        name = "rmb_%d_%d_%d" % t[:3]
        if pool_in and fold:
            name += "+pool_in"
        if pool_out and fold and fused_tile(cin, cout, H, W, has_sc, rm_fuse, hook, pool_out=True):
            name += "+pool_out"
        return name
    # c1 + shortcut in one launch: few streams, and one stream stride for y1 and the output (not the upper half of a concat buffer at several streams)
    return "pair" if has_sc and streams <= 4 and (streams == 1 or not y_in_cat) else "plain"


# ------------------------------------------------------------------------------------------------------------------------------------------
# the GPU suite's cases
Case = namedtuple("Case", "label cin cout H W streams sc pool_in pool_out cat next rm_fuse hooks kinds")
KINDS = ("gauss", "zero", "const")


def _case(label, cin, cout, H, W, streams, sc=None, pool_in=0, pool_out=0, cat=0, next=0, rm_fuse=1, hooks=(None, 0), kinds=KINDS):
    return Case(label, cin, cout, H, W, tuple(streams), (cin != cout) if sc is None else bool(sc), pool_in, pool_out, cat, next, rm_fuse, tuple(hooks), tuple(kinds))


def _cases():
    fam = {}
    # the model's shallow blocks (encoder levels 0 - 1, decoder levels 3 - 4 and the 64 -> 32 block behind the concat) on a 16 x 32 image
    fam["model"] = [
        _case("m_1_16", 1, 16, 16, 32, (1, 2, 3, 4)), _case("m_16_16", 16, 16, 16, 32, (1, 2, 3, 4), next=1),
        _case("m_16_32_poolin", 16, 32, 16, 32, (1, 2, 3, 4), pool_in=1, hooks=(None, 0, 3)),
        _case("m_32_32_poolout_cat", 32, 32, 16, 32, (1, 2, 3, 4), pool_out=1, cat=1, next=1, hooks=(None, 0, 3)),
        _case("m_64_32", 64, 32, 16, 32, (1, 2, 3, 4), next=1), _case("m_32_32", 32, 32, 16, 32, (1, 2, 3, 4)),
        _case("m_32_16", 32, 16, 16, 32, (1, 2, 3, 4), next=1), _case("m_16_16_cat", 16, 16, 16, 32, (1, 2, 3, 4), cat=1),
    ]
    # tile edges: exactly one 16-channel tile, one row and column past it, odd and partial both ways, smaller than a tile, degenerate images
    fam["edges"] = []
    for i, (H, W) in enumerate(((8, 16), (9, 17), (13, 37), (5, 7), (2, 2), (1, 1), (1, 40), (40, 1))):
        for j, (ci, co) in enumerate(((16, 16), (32, 16), (32, 32), (16, 32))):
            fam["edges"].append(_case("e_%dx%d_%d_%d" % (H, W, ci, co), ci, co, H, W, (1 + (i + j) % 3,), next=(i + j) & 1))
    fam["pool"] = [
        _case("p_in_6x12", 16, 32, 6, 12, (1, 3), pool_in=1), _case("p_in_4x8", 16, 32, 4, 8, (2,), pool_in=1),
        _case("p_out_12x24", 32, 32, 12, 24, (1, 3), pool_out=1, cat=1), _case("p_out_6x12", 32, 32, 6, 12, (2,), pool_out=1, cat=1),
        _case("p_out_W4", 32, 32, 6, 4, (2,), pool_out=1),                                # TW = 4: the pooling launch
        _case("p_out_16ch_W8", 16, 16, 10, 8, (2,), pool_out=1),                          # a 16-channel block whose tile is clamped to eight columns
        _case("p_out_16ch_W16", 16, 16, 8, 16, (1,), pool_out=1),                         # ... and one at its own width: the pooling launch
        _case("p_in_out_6x12", 16, 32, 6, 12, (2,), pool_in=1, pool_out=1, cat=1, hooks=(None, 0, 3)),
    ]
    # channel counts the model does not use
    fam["channels"] = [
        _case("c_8_16", 8, 16, 9, 17, (2,)), _case("c_24_32", 24, 32, 9, 17, (2,)), _case("c_48_16", 48, 16, 9, 17, (2,), next=1),
        _case("c_64_16", 64, 16, 9, 17, (1, 2)),                                          # LDS over 64 KB: declined
        _case("c_32_64", 32, 64, 9, 17, (2,)), _case("c_128_64", 128, 64, 9, 17, (1, 5)),     # never fused; 5 streams: no pair launch
        _case("c_128_64_1x40", 128, 64, 1, 40, (1, 5)),                                   # K = 1152: the one-row tap pruning of the unfused c1
    ]
    # more streams than build_rmvpe's rule allows: forced
    fam["streams5"] = [_case("s5_16_16", 16, 16, 9, 17, (5,), rm_fuse=0, hooks=(2, 0), next=1), _case("s5_16_32", 16, 32, 9, 17, (5,), rm_fuse=0, hooks=(2, 0)),
                       _case("s5_rule", 16, 32, 9, 17, (5,), rm_fuse=0, hooks=(None,))]
    return fam


FAMILIES = _cases()
CASES = [c for f in FAMILIES.values() for c in f]


def runs_of(case):
    """(streams, data kind) of every run of a case: Gaussian data at every stream count, the zero and constant inputs at the largest"""
    return [(s, k) for s in case.streams for k in case.kinds if k == "gauss" or s == case.streams[-1]]


def rng_for(label):
    return np.random.default_rng(zlib.crc32(label.encode()))


def data_for(case, streams, kind):
    """-> dict(x, w1, b1, w2, b2, wsc, bsc) in float32; x is [B][cin][2H][2W] for a pool_in case"""
    rng = rng_for("%s/%d/%s" % (case.label, streams, kind))
    ci, co = case.cin, case.cout
    H, W = (2 * case.H, 2 * case.W) if case.pool_in else (case.H, case.W)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    d = dict(w1=f32(rng.standard_normal((co, ci, 3, 3)) / np.sqrt(9 * ci)), w2=f32(rng.standard_normal((co, co, 3, 3)) / np.sqrt(9 * co)), wsc=None, bsc=None)
    sign = lambda n: np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    if kind == "zero":
        # the interior is constant per channel; the border ring differs from it only because y1 is ZERO outside the image (b1 > 0: ReLU(b1) would not be)
        d["x"] = np.zeros((streams, ci, H, W), np.float32)
        d["b1"] = f32(rng.uniform(0.5, 1.5, co))
        s = sign(co); s[::2] = 1.0
        d["b2"] = f32(rng.uniform(0.3, 1.0, co) * s)
    else:
        # clearly positive and clearly negative channels: both ReLUs cut
        d["b1"] = f32(rng.uniform(0.5, 1.0, co) * sign(co))
        d["b2"] = f32(rng.uniform(0.5, 1.0, co) * sign(co))
        if kind == "gauss":
            d["x"] = f32(rng.standard_normal((streams, ci, H, W)))
        else:
            # one distinct constant per input channel, one scale per stream: a channel or stream mix-up shows at full size
            c = rng.permutation(np.linspace(-1.0, 1.0, ci) + 0.013)
            d["x"] = f32(np.broadcast_to((1.0 + 0.37 * np.arange(streams))[:, None, None, None] * c[None, :, None, None], (streams, ci, H, W)))
    if case.sc:
        d["wsc"] = f32(rng.standard_normal((co, ci)) / np.sqrt(ci))
        d["bsc"] = f32(rng.uniform(0.2, 0.6, co) * sign(co))
    return d


def reference(case, d):
    """-> (out [B][cout][H][W], pooled [B][cout][H/2][W/2] or None) in float64"""
    x = avgpool2(d["x"]) if case.pool_in else d["x"]
    out = block(x, d["w1"], d["b1"], d["w2"], d["b2"], d["wsc"], d["bsc"])
    return out, (avgpool2(out) if case.pool_out else None)
