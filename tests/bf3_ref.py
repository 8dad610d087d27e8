"""What the split-bf16 GEMM (igemm_bf3_kernel, rvc_set_gemm_precision(e, 1)) computes, restated on the CPU: the split, the three-term product with exact
products and fp64 accumulation, what that algorithm alone costs against the fp64 definition of a layer (split_cost), the bound the device is held to, the
three broken variants the bound has to reject, and the index arithmetic of the weight panels and of the staged activation tile.  Shared by
tests/test_bf3_ref.py (CPU) and tests/test_gpu_bf3.py (device): both evaluate a case through the same functions on the same inputs (test_gpu_layers.data_for).

Names: a = the weights (the MFMA's A operand), b = the activations (B operand).  hi = bf16(v) round-to-nearest-even, lo = bf16(v - float(hi)).  The kernel
adds a_lo b_hi, a_hi b_lo and a_hi b_hi per 16-deep chunk into an fp32 accumulator; a_lo b_lo is never computed."""
import numpy as np

import layer_ref as R
from test_gpu_layers import Case, conv_of, data_for, finish
from test_gpu_tiles import TOL

FULL, NO_A_LO_B_HI, NO_A_HI_B_LO, HI_HI_ONLY = "full", "drop a_lo.b_hi", "drop a_hi.b_lo", "a_hi.b_hi only"
BROKEN = (NO_A_LO_B_HI, NO_A_HI_B_LO, HI_HI_ONLY)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the split
def bf16_rne(v):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32: numpy bit arithmetic on finite values"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split(v):
    """-> (hi, lo) as float32 arrays holding bfloat16 values; v - hi is exact in fp32 (hi keeps the leading 8 bits of v)"""
    v = np.ascontiguousarray(v, np.float32)
    hi = bf16_rne(v)
    return hi, bf16_rne(v - hi)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the emulation of a layer
def staged_input(case, d):
    """the activations as the kernel's stage() splits them: the fused input LeakyReLU in fp32 first (max(x, x * slope)), as the kernel computes it"""
    p = case.p
    x = d.x.astype(np.float32)
    if p["pre_act"]:
        assert p["pre_act"] == R.ACT_LRELU
        x = np.maximum(x, x * np.float32(p["pre_slope"]))
    return x


def terms(case, d):
    """the three products per output tensor, exact products summed in fp64 (a bf16 x bf16 product has 16 significant bits):
    -> {"hh": a_hi b_hi, "hl": a_hi b_lo, "lh": a_lo b_hi}, each a list over the output tensors"""
    b_hi, b_lo = split(staged_input(case, d))
    a = [split(w) for w in d.ws]
    a_hi, a_lo = [s[0] for s in a], [s[1] for s in a]
    n_out = len(d.refs)
    f64 = np.float64
    return {"hh": [conv_of(case, b_hi.astype(f64), a_hi, j) for j in range(n_out)],
            "hl": [conv_of(case, b_lo.astype(f64), a_hi, j) for j in range(n_out)],
            "lh": [conv_of(case, b_hi.astype(f64), a_lo, j) for j in range(n_out)]}


def emulate(case, d, t, variant=FULL):
    """the layer through the split product (or a broken variant of it) and the fp64 epilogue -> the output tensors"""
    keep = {FULL: ("hh", "hl", "lh"), NO_A_LO_B_HI: ("hh", "hl"), NO_A_HI_B_LO: ("hh", "lh"), HI_HI_ONLY: ("hh",)}[variant]
    convs = [sum(t[k][j] for k in keep) for j in range(len(d.refs))]
    return [v for (v, _) in finish(case, d, convs)]


def deviation(d, outs):
    """max |out - fp64 definition| / rms, normalised as test_gpu_layers.Layer.run normalises the device's error (the rms of the largest addend)"""
    return max(float(np.max(np.abs(np.asarray(o, np.float64) - ref))) / max(scale, 1e-30) for o, (ref, scale) in zip(outs, d.refs))


class Cost:
    """split_cost, BOUND and the deviations of the broken variants of one (case, streams)"""

    def __init__(self, case, streams):
        d = data_for(case, streams)
        t = terms(case, d)
        self.split_cost = deviation(d, emulate(case, d, t))
        # 2 x: the MFMA's own fp32 accumulation order inside a 16-deep chunk, which the emulation does not model; TOL: what the project allows the fp32
        # accumulation of these kernels (test_gpu_tiles.TOL)
        self.bound = 2.0 * self.split_cost + TOL
        self.broken = {v: deviation(d, emulate(case, d, t, v)) for v in BROKEN}


_COSTS = {}


def cost(case, streams):
    key = (case.name, streams)
    if key not in _COSTS:
        _COSTS[key] = Cost(case, streams)
    return _COSTS[key]


# ------------------------------------------------------------------------------------------------------------------------------------------
# index arithmetic: the weight panels (bf3_pack_kernel, igemm_bf3_inst.hip) and the staged activation tile (igemm_bf3_kernel: gather / stage / kstep)
CSB, BN = 48, 128                          # bytes per column and half in LDS; columns of a workgroup tile
HALF, BUF = BN * CSB, 2 * BN * CSB         # one half (hi or lo) of a buffer; one buffer
LDS_TILE_BYTES = 2 * BUF                   # two buffers: the 2 * 2 * 128 * 48 of queue_bf3's LDS rule


def fragment_index(m, k, nchunks):
    """float index of W[m][k] in the fp32 fragment-major panel [m / 16][chunk][lane 16 x 4][4] the planner's weights are uploaded in"""
    kk = k % 16
    return (((m >> 4) * nchunks + k // 16) * 64 + (kk >> 2) * 16 + (m & 15)) * 4 + (kk & 3)


def pack_source(e, i, M, nchunks):
    """bf3_pack_kernel: value i of output element e (one lane's eight bf16 of one half) -> (float index in the fragment-major panel, or -1 for a zero
    behind the panel's last 16-row fragment; half: 0 = hi, 1 = lo).  Works on integer arrays."""
    e = np.asarray(e, np.int64)
    lane, half, bc = e & 63, (e >> 6) & 1, e >> 7
    chunk, blk = bc % nchunks, bc // nchunks
    m, mt16 = blk * 32 + (lane & 31), (M + 15) >> 4
    return np.where((m >> 4) < mt16, fragment_index(m, chunk * 16 + (lane >> 5) * 8 + i, nchunks), -1), half


def panel_bytes(M, nchunks):
    return ((M + 31) // 32) * nchunks * 2048


def a_byte(blk, c, h, lane, nchunks):
    """wload: byte offset in a phase's split panel of what lane reads for 32-row block blk, chunk c, half h (wo[mt] + c * 2048 + h * 1024)"""
    return blk * nchunks * 2048 + lane * 16 + c * 2048 + h * 1024


def a_k(c, lane, i):
    """the k the MFMA's A operand takes from value i of lane (v_mfma_f32_32x32x16_bf16: row lane & 31, k = (lane >> 5) * 8 + i) in chunk c"""
    return c * 16 + (lane >> 5) * 8 + i


def stage_write(tid, c, i):
    """staging thread tid, chunk c, value i -> (byte offset inside a half of buffer, 2 * i added for the value; the k it gathered)"""
    n_s, g_s = tid % BN, tid // BN
    return n_s * CSB + g_s * 16 + 2 * i, c * 16 + g_s * 8 + i


def b_read(wn, nt, lane, i):
    """kstep: wave column wn, block nt, value i of lane -> (byte offset inside a half of buffer, column of the workgroup tile)"""
    c32, ks = lane & 31, lane >> 5
    col = (wn * 2 + nt) * 32 + c32
    return col * CSB + ks * 16 + 2 * i, col


# ------------------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_bf3.py (here, so that tests/test_bf3_ref.py evaluates their split_cost and the separation of the broken variants on the CPU).
# The kernel's rule wants ceil(M / 128) * ceil(N / 128) * phases >= 250 workgroups, N = streams * columns per stream once the streams are folded: M * N is
# ~4.1 million whatever the shape, so K is short wherever K is not the point.  Lengths are odd (no multiple of 128 or 32), and with folded streams no stream
# ends on a tile boundary.  One (case, stream count) each: the rule is a function of both.
LR = R.ACT_LRELU
ELIGIBLE = [
    # table-free 1x1 layers (LIN); the epilogues of ContentVec's four call sites (model_cv.hip: qkv, out-proj / ff2, ff1) and what else the shared epilogue has
    Case("lin_k32_qkv", "model_cv.hip qkv (bias only); K = 32: two chunks, the minimum", streams=(1,), cin=32, cout=768, t_in=5261, t_out=5261),
    Case("lin_k48_fold", "K = 48: three chunks, the odd tail step; six streams folded, tiles straddle streams", streams=(6,), cin=48, cout=768, t_in=877,
         t_out=877),
    Case("lin_k784_ff1_gelu", "model_cv.hip ff1 (GELU); K = 784: 49 chunks", streams=(1,), cin=784, cout=768, t_in=5261, t_out=5261, act=R.ACT_GELU),
    Case("lin_cv768_res_self", "model_cv.hip out-proj / ff2 (residual = the output tensor); ContentVec's own 768 x 768, six streams folded", streams=(6,),
         cin=768, cout=768, t_in=877, t_out=877, res=3),
    Case("lin_m700_nobias_scale", "M = 700: 22 blocks of 32, blocks 22 and 23 of the last tile clamp; no bias, scale 0.5", streams=(1,), cin=32, cout=700,
         t_in=5261, t_out=5261, no_bias=1, scale=0.5),
    Case("lin_m160_res", "M = 160: the second tile is one block and three clamps; residual tensor, scale 1/3, 12 streams folded", streams=(12,), cin=32,
         cout=160, t_in=1323, t_out=1323, r_halo=4, res=1, scale=1.0 / 3),
    Case("lin_m128_edge250", "M = 128: one tile; N = 249 * 128 + 1: exactly 250 workgroups", streams=(1,), cin=32, cout=128, t_in=31873, t_out=31873),
    # layers with a gather table: three dilated taps, without and with the fused input LeakyReLU (PRE); conv_tile declines more than 128 rows / more than 4 streams
    Case("tab_d3", "model_synth.hip ResBlock-like: 3 taps, dilation 3, 256 rows, one stream", streams=(1,), cin=32, cout=256, kw=3, pad=3, dil=3, t_in=15877,
         t_out=15877, x_halo=4, y_halo=4),
    Case("tab_d3_pre_fold", "the same with the fused input LeakyReLU and an output LeakyReLU, six streams folded", streams=(6,), cin=32, cout=256, kw=3, pad=3,
         dil=3, t_in=2647, t_out=2647, x_halo=4, y_halo=4, pre_act=LR, pre_slope=0.1, act=LR, slope=0.1),
    Case("tab_m128_s6_pre", "128 rows at six streams: conv_tile stops at four streams", streams=(6,), cin=32, cout=128, kw=3, pad=3, dil=3, t_in=5313,
         t_out=5313, x_halo=4, y_halo=4, pre_act=LR, pre_slope=0.1),
    # polyphase ConvTranspose1d: every phase its own weight panel and output columns; the phase count carries the launch past 250 workgroups
    Case("convT_16_8", "model_synth.hip:180-183 256 -> 128, (k, s) = (16, 8): 8 phases x 32 column tiles; 64 streams of 63 columns folded", streams=(64,), form=1,
         cin=256, cout=128, kw=16, stride=8, pad=4, t_in=62, t_out=62 * 8, x_halo=4, y_halo=4, pre_act=LR, pre_slope=0.1),
    Case("convT_24_12_res", "model_synth.hip:180-183 512 -> 256, (24, 12): 12 phases x 2 x 11 tiles; 64 streams of 21 columns folded, residual", streams=(64,),
         form=1, cin=512, cout=256, kw=24, stride=12, pad=6, t_in=20, t_out=20 * 12, x_halo=4, y_halo=4, r_halo=4, pre_act=LR, pre_slope=0.1, res=1),
]
# under mode 1 these must run what mode 0 runs, bit for bit; each fails ONE condition of the rule and has its 250 workgroups
INELIGIBLE = [
    Case("edge249", "lin_m128_edge250 one column tile shorter: 249 workgroups", streams=(1,), cin=32, cout=128, t_in=31872, t_out=31872),
    Case("tile_first", "128 rows with a table at one stream: conv_tile is queued ahead of bf3", streams=(1,), cin=32, cout=128, kw=3, pad=3, dil=3,
         t_in=31873, t_out=31873, x_halo=4, y_halo=4),
    Case("glu", "model_synth.hip:146 (WaveNet in-layer, gated)", streams=(1,), cin=192, cout=384, kw=5, pad=2, t_in=10701, t_out=10701, x_halo=4, glu=1),
    Case("accumulate", "model_synth.hip:147-149 (res_skip, accumulate)", streams=(1,), cin=192, cout=384, t_in=10701, t_out=10701, y_halo=4, accumulate=1),
    Case("m96", "96 rows (M < 128)", streams=(1,), cin=32, cout=96, t_in=31873, t_out=31873),
    Case("k16", "K = 16: one chunk", streams=(1,), cin=16, cout=256, t_in=15877, t_out=15877),
    Case("conv2d", "model_rmvpe.hip Conv2d 3x3: a 2-D layer", streams=(1,), form=4, cin=16, cout=128, t_in=250, t_out=128),
    Case("k9232_table", "K = 577 x 16 = 9232: 577 chunks, the offset table (36 928 bytes) and the tile (24 576) exceed 60 KiB of LDS", streams=(1,), cin=577,
         cout=256, kw=16, pad=8, t_in=15877, t_out=15877, x_halo=8),
]
