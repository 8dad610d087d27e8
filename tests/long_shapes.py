"""The file converter's window lengths as the suites use them (DESIGN.md "Long windows: what is tested"): the single-op shapes of tests/test_gpu_ops.py, the
window geometries of tests/test_gpu_long_windows.py and the LDS rule of the generic attention kernel.  Plain data and arithmetic, no device."""
from obs_rvc_amd.rvc import RvcInfer

# Relative attention at RVC's head size 96 up to return_length 351, the last length whose K / V and score rows fit the LDS: 156 (the first length past the
# streaming cases), the 256 | 257 row stride, 350 | 351 which share the odd-padded row Tp = 351 (the padding column in use or not); head size 16 at 351 and at
# 1025, an odd row above 1024 (133 KB).  The GRU at the default window's 448 steps and at the longest one's 1024.  (head size or H, T, streams)
LONG_RELPOS = [(96, T, B) for T in (156, 255, 256, 257, 350, 351) for B in (1, 3)] + [(16, 351, 1), (16, 1025, 1)]
LONG_GRU = [(256, T, B) for T in (448, 1024) for B in (1, 3)] + [(32, 1024, 1)]
LDS_LIMIT = 160 * 1024


def attn_valu_lds(hd, T):
    """bytes of dynamic LDS of attention_kernel (plan.hip, attn_valu_lds): K or V of one head [hd][Tp] rounded up to 4 floats, the score rows of 4 waves
    [4][Tp][4] and their queries [4][hd][4], Tp = T | 1"""
    Tp = T | 1
    return (((hd * Tp + 3) & ~3) + 16 * Tp + 16 * hd) * 4


R_MAX = 351                               # the relative attention's LDS limit at RVC's head size 96
# (k, context, crossfade) -> (Tm, T, R): the smallest geometries that reach each edge.  On the tiny zoo (text-encoder head size 8, ContentVec head size 12) these
# run the generic attention kernels far inside their LDS limits; the limit itself is reached by the single-op cases above only
GEOMETRIES = {
    (2, 3, 2): (64, 31, 57),              # what the converter's composition tests run and nothing compares with a reference
    (14, 48, 5): (448, 223, 351),         # the default: generic relative attention at 351 frames, GRU generic at 448, NSF source at 351
    (9, 3, 1): (288, 143, 281),           # the smallest context: the pitch cache read starts at 1024 - F + 3, the first row the window itself computed
}


def far_end_context(k):
    """the smallest context at which a window of k returns at most R_MAX frames: C = ceil((F - 351) / 2), at least the converter's minimum of 3"""
    F = 32 * k - 1
    return max(3, -(-(F - R_MAX) // 2))


def geometry(k, C, X):
    """rvc_convert_geometry of one window -> (n, sample_frame_16k_size, skip_head, return_length)"""
    geo = RvcInfer.convert_geometry(160, 4800, k, C, X)
    assert geo["n"] == 5120 * k - 160
    return geo["n"], geo["sample_frame_16k_size"], geo["skip_head"], geo["return_length"]
