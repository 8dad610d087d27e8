"""The split-bf16 GEMM (igemm_bf3_kernel, obs_rvc_amd/csrc/igemm_bf3.hip.h; weights split by bf3_pack_kernel) per layer form against fp64, through
rvc_debug_layer under rvc_set_gemm_precision(e, 1) -- the machinery of tests/test_gpu_layers.py (Case, the sentinel-filled allocations, the stray-write and
last-kernel checks) with the bound of tests/bf3_ref.py in place of the fp32 tolerance:

    BOUND = 2 x split_cost + TOL      split_cost: the three-term product a_hi b_hi + a_hi b_lo + a_lo b_hi with exact products and fp64 accumulation, against the
                                      fp64 definition, on this case's inputs (tests/test_bf3_ref.py shows that BOUND rejects a product with a term missing)

Eligible cases (bf3_ref.ELIGIBLE) must run the family "bf3" -- the planner's rule is restated below, so a case that falls back to an fp32 family fails --, stay
within their BOUND and leave every float outside the written interior (guard zones, halos, ld padding, the columns and rows the kernel's clamped loads stand
in for) bit for bit.  Ineligible cases (bf3_ref.INELIGIBLE: the rule's edge at 249 workgroups, conv_tile's precedence, GLU, accumulate, M < 128, one chunk
of K, a 2-D layer, a table beyond LDS) must not run bf3 and must give mode 0's bits.

Measured (max |.| / rms as test_gpu_layers normalises; split_cost and BOUND on the CPU by tests/test_bf3_ref.py, the device error on an MI355X):
    case (streams)                K      split_cost   BOUND       device error
    lin_k32_qkv (1)               32     2.621e-05    7.242e-05   2.616e-05
    lin_k48_fold (6)              48     2.596e-05    7.193e-05   2.594e-05
    lin_k784_ff1_gelu (1)         784    3.713e-05    9.426e-05   3.606e-05
    lin_cv768_res_self (6)        768    1.111e-05    4.222e-05   1.113e-05
    lin_m700_nobias_scale (1)     32     2.644e-05    7.287e-05   2.641e-05
    lin_m160_res (12)             32     1.244e-05    4.489e-05   1.252e-05
    lin_m128_edge250 (1)          32     2.492e-05    6.985e-05   2.495e-05
    tab_d3 (1)                    96     2.386e-05    6.771e-05   2.376e-05
    tab_d3_pre_fold (6)           96     3.208e-05    8.417e-05   3.212e-05
    tab_m128_s6_pre (6)           96     2.269e-05    6.538e-05   2.270e-05
    convT_16_8 (64)               512    2.061e-05    6.122e-05   2.083e-05
    convT_24_12_res (64)          1024   3.720e-06    2.744e-05   3.703e-06
The device's error is the algorithm's: within 2 % of split_cost everywhere, the fp32 accumulation adds nothing visible.  Every broken variant of
test_bf3_ref.py is 46 to 216 x BOUND away from fp64.  With one of the three MFMAs taken out of the kernel (a local check, not committed) all twelve
eligible cases and the mode-switching test failed at 1.4e-3 to 1.3e-2; no stray write was found in any case."""
import numpy as np
import pytest

import bf3_ref as B3
from debug_abi import same_bits
from test_gpu_layers import Layer, _k_of
from test_gpu_tiles import TOL

pytestmark = pytest.mark.gpu

NCU = 256           # compute units of an MI355X (plan.hip g_ncu): conv_tile's "enough items" rule counts in them
# An ineligible case whose fp32 result is not held to TOL against fp64 here: 9232 products summed in fp32 by one wave in K order (the register-direct kernel
# without a K split, in both modes) measured 2.66e-5 of the rms, and TOL = 2e-5 is the project's allowance for the K <= 6144 of its models' layers.  What this
# file asks of an ineligible case -- no bf3, mode 0's bits, no stray write -- is asserted for it as for the others; its error is printed.
FP64_NOT_ASSERTED = {"k9232_table"}


# ------------------------------------------------------------------------------------------------------------------------------------------
# the planner's rules, restated (obs_rvc_amd/csrc/plan.hip: queue_igemm_impl, queue_conv_tile, queue_bf3)
def launch_shape(case, streams):
    """the implicit GEMM a layer becomes, as queue_bf3 sees it: M rows, N columns (streams folded into N where the planner folds), K, phases"""
    p = case.p
    f = p["form"]
    K = -(-_k_of(case) // 16) * 16
    if f == 1:
        n_stream, nphase = p["t_in"] + -(-p["kw"] // p["stride"]) - 1, p["stride"]       # (polyphase: one phase per output residue, ceil(kw / s) taps each)
    elif f == 4:
        n_stream, nphase = p["t_in"] * p["t_out"], 1
    else:
        n_stream, nphase = p["t_out"], (p["groups"] if f == 0 else (p["n"] if f == 2 else 2))
    lin = f == 0 and p["kw"] == 1 and p["groups"] == 1 and p["pad"] == 0 and _k_of(case) % 16 == 0
    # more than one stream: folded into N when the offset table fits in LDS (queue_igemm_impl; the byte limits of the fold hold for every shape here)
    folded = streams > 1 and (K // 16) * 64 <= 60 * 1024
    M = p["cout"] // p["groups"] if f == 0 else p["cout"]
    N = n_stream * streams if folded else n_stream
    return dict(M=M, N=N, K=K, nphase=nphase, lin=lin, batches=1 if (folded or streams == 1) else streams,
                wgs=-(-M // 128) * -(-N // 128) * nphase)


def conv_tile_takes(case, streams):
    """queue_conv_tile under its production rule: it is tried before queue_bf3 (before the fold for 2..4 streams) and does not look at the precision mode"""
    p = case.p
    f = p["form"]
    s = launch_shape(case, streams)
    if f not in (0, 2) or s["lin"] or p["glu"] or streams > 4 or s["M"] > 128 or (f == 0 and p["stride"] != 1):
        return False
    M, n_stream = s["M"], p["t_out"]
    bm, bn = (128, 16) if M > 64 else ((64, 32) if M > 32 else (32, 64))
    if -(-M // bm) * -(-n_stream // bn) * s["nphase"] * streams < 3 * NCU // 2:
        return False
    lds = 0
    for j in range(s["nphase"] if f == 2 else 1):
        cin = p["cin"] // p["groups"] if f == 0 else p["cin"]
        kw, dil = (p["kw"], p["dil"]) if f == 0 else (p["kws"][j], p["dils"][j])
        if cin % 16 or cin // 16 < 2 or cin * kw < 32 or (kw - 1) * dil > 255:        # 16-channel groups, a chunk for each of the two K shares, two chunks of K
            return False
        rl = bn + (kw - 1) * dil
        lds = max(lds, (max(-(-cin * (rl | 1) // 64) * 64, 8 * 256) + rl * (cin + 8)) * 4)
    return lds <= 100 * 1024


def bf3_must_run(case, streams):
    """queue_bf3's eligibility under rvc_set_gemm_precision(e, 1) (the debug plan's key.bf3), behind what is queued ahead of it"""
    p = case.p
    s = launch_shape(case, streams)
    if conv_tile_takes(case, streams):
        return False
    nchunks = s["K"] // 16
    one_d = p["form"] in (0, 1, 2)               # (no row stride on either side: x_hs == 0, y_hm == 0; the pair launch of form 3 has a per-phase epilogue)
    return bool(one_d and not p["glu"] and s["batches"] == 1 and s["M"] >= 128 and nchunks >= 2 and not p["accumulate"] and
                nchunks * 64 + 2 * 2 * 128 * 48 <= 60 * 1024 and s["wgs"] >= 250)


# ------------------------------------------------------------------------------------------------------------------------------------------
class Bf3Layer(Layer):
    def run_mode(self, case, streams, mode, tol=TOL):
        """-> (family, problems, copies of the output interiors, max err / rms per output, launch description)"""
        self.set_gemm_precision(mode)
        try:
            fam, bad = self.run(case, streams, tol)
        finally:
            self.set_gemm_precision(0)
        return fam, bad, [np.array(o, copy=True) for o in self.outputs], list(self.errors), self.last_desc()


@pytest.fixture(scope="module")
def layer():
    ly = Bf3Layer()
    try:
        yield ly
    finally:
        ly.close()


def _desc_fields(desc):
    return dict(w.split("=", 1) for w in desc.split()[1:] if "=" in w)


@pytest.mark.parametrize("case", B3.ELIGIBLE, ids=lambda c: c.name)
def test_eligible_layer_runs_bf3_within_its_bound(layer, case):
    for streams in case.streams:
        assert bf3_must_run(case, streams), (case.name, streams)
        c = B3.cost(case, streams)
        fam, bad, _, errs, desc = layer.run_mode(case, streams, 1, tol=c.bound)
        print("%-24s @ %2d streams: device err %.3e  split_cost %.3e  BOUND %.3e  [%s]" % (case.name, streams, max(errs) if errs else float("nan"), c.split_cost, c.bound, desc))
        assert fam == "bf3", "%s (%s) @ %d streams ran %s" % (case.name, case.site, streams, desc)
        assert not bad, "%s (%s) @ %d streams [%s]:\n  %s" % (case.name, case.site, streams, desc, "\n  ".join(bad))
        assert max(errs) < c.bound
        # the launch is the one the restated rule counted, on the variant the layer calls for
        s, f = launch_shape(case, streams), _desc_fields(desc)
        gx, gy = (int(v) for v in f["grid"].split("x"))
        pre = int(case.p["pre_act"] != 0)
        assert (int(f["M"]), int(f["N"]), int(f["K"]), int(f["nph"])) == (s["M"], s["N"], s["K"], s["nphase"]) and gx * gy == s["wgs"] and gy == s["nphase"], desc
        assert int(f["pre"]) == pre and int(f["lin"]) == int(s["lin"] and s["nphase"] == 1 and not pre), desc


@pytest.mark.parametrize("case", B3.INELIGIBLE, ids=lambda c: c.name)
def test_ineligible_layer_keeps_mode_0_bits(layer, case):
    for streams in case.streams:
        assert not bf3_must_run(case, streams), (case.name, streams)
        tol = float("inf") if case.name in FP64_NOT_ASSERTED else TOL
        fam0, bad0, out0, err0, desc0 = layer.run_mode(case, streams, 0, tol=tol)
        fam1, bad1, out1, err1, desc1 = layer.run_mode(case, streams, 1, tol=tol)
        print("%-24s @ %2d streams: fp32 err %.3e / %.3e  mode 0 [%s]  mode 1 [%s]" % (case.name, streams, max(err0), max(err1), desc0, desc1))
        assert fam0 != "bf3" and fam1 != "bf3", (desc0, desc1)
        assert not bad0 and not bad1, "%s (%s):\n  %s" % (case.name, case.site, "\n  ".join(bad0 + bad1))
        assert all(same_bits(a, b) for a, b in zip(out0, out1)), "%s: mode 1 [%s] differs from mode 0 [%s]" % (case.name, desc1, desc0)
        if case.name == "tile_first":
            assert fam0 == fam1 == "tile", (desc0, desc1)


def test_mode_0_after_mode_1_gives_mode_0s_bits_again(layer):
    case = next(c for c in B3.ELIGIBLE if c.name == "lin_k48_fold")
    streams = case.streams[0]
    bound = B3.cost(case, streams).bound
    fam_a, bad_a, out_a, _, _ = layer.run_mode(case, streams, 0)
    fam_b, bad_b, out_b, _, _ = layer.run_mode(case, streams, 1, tol=bound)
    fam_c, bad_c, out_c, _, _ = layer.run_mode(case, streams, 0)
    assert not (bad_a or bad_b or bad_c), bad_a + bad_b + bad_c
    assert fam_b == "bf3" and fam_a == fam_c != "bf3", (fam_a, fam_b, fam_c)
    assert all(same_bits(a, c) for a, c in zip(out_a, out_c))
    assert not all(same_bits(a, b) for a, b in zip(out_a, out_b))         # (the split product is not the fp32 product: equal bits would mean bf3 did not compute them)
