"""The transformer and recurrent ops of the models -- ContentVec attention, the synthesizer's relative-position attention, LayerNorm over channels and
RMVPE's bidirectional GRU -- through rvc_debug_op (the plan helpers add_attention / add_relpos_attention / add_layernorm / add_gru the models call),
against the fp64 definitions of tests/op_ref.py, one kernel variant at a time.  Shapes straddle every dispatch threshold and tile edge of the
variants; inputs stress the arithmetic (attention logits over about +-40 with one dominant key and rows of equal scores, LayerNorm columns with a
large mean and a small spread, GRU gates driven into saturation).  Each run checks
  * the values: max |gpu - ref| / rms(ref) below the family's tolerance (TOL_* below, each with its derivation);
  * that nothing else was written: the whole allocations -- guard zones, halos, ld padding (the columns behind T that the LayerNorm strip kernel
    reads), other rows, other streams, and the input of the out-of-place ops -- are pre-filled (halos with zeros, as in production, everything
    else with a sentinel) and must come back bit for bit;
  * which variant ran (rvc_debug_last_kernel): over the shape list, the set reached under the production rules must be the set the rules allow,
    and every variant forced through its hook (RVC_ATTN_KERNEL, RVC_RELPOS_KERNEL, RVC_LN_KERNEL, RVC_GRU_KERNEL) runs on every shape it is
    eligible for and is refused (RVC_SHAPE, nothing launched) on every other one."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import op_ref as R
from common import set_opt
from debug_abi import RVC_SHAPE, Handle, OpSpec, index, ptr, same_bits, stray
from long_shapes import LDS_LIMIT, LONG_GRU, LONG_RELPOS, attn_valu_lds

pytestmark = pytest.mark.gpu

OP_MHA, OP_REL, OP_LN, OP_GRU = 0, 1, 2, 3
SENT_X, SENT_Y, SENT_STATUS = np.float32(-7777.25), np.float32(5555.5), -99
HOOK = {OP_MHA: "RVC_ATTN_KERNEL", OP_REL: "RVC_RELPOS_KERNEL", OP_LN: "RVC_LN_KERNEL", OP_GRU: "RVC_GRU_KERNEL"}
FAMILY = {OP_MHA: "attn", OP_REL: "relpos", OP_LN: "ln", OP_GRU: "gru"}
VARIANTS = {OP_MHA: ("mfma2", "mfma2_qloop", "mfma4", "mfma4_qloop", "valu"), OP_REL: ("mfma", "small", "valu"),
            OP_LN: ("ct4", "ct16", "tile", "strip4", "strip12", "strip16"), OP_GRU: ("multi", "generic")}

# Tolerances: max |gpu - ref| / rms(ref).  fp32 has eps = 6e-8; the conv tests hold 2e-5 for fp32 sums over up to 5632 products.
#  * attention: the softmax turns an absolute error of a logit into the same relative error of its weight.  A logit is a sum of hd products
#    (+ as many for the relative key) whose magnitudes add up to S = sum_d |q_d k_d| / sqrt(hd), about 77 at logits of +-40 and hd = 64, so its
#    fp32 rounding is ~sqrt(hd) u S = 8 x 6e-8 x 77 = 3.7e-5 (u = 2^-24).  The first GPU run measured 1.3e-5 .. 4.2e-5 (max / rms over all
#    variants, largest for the generic kernel with the relative terms at R = 155); 1e-4 is that with a 2.4x margin.
#  * LayerNorm: C <= 1024 summands; 2e-5 as for the convolutions (the first GPU run measured at most 1.4e-6).  For columns with a large mean m and a small spread s the computation is
#    ill-conditioned in fp32 whatever the kernel: the rounding of the mean's fp32 sums, up to (length of the longest sequential chain of adds) x u
#    x |m| with u = 2^-24, comes out amplified by 1 / s.  The chains are 16 + 64 adds in the strip kernel and C / 8 + 8 = 136 in the tile kernel,
#    so that stream is held to TOL_LN_OFFSET = 128 u x |m| / s (1e3 +- 1: ~1.3e-2).  A one-pass variance (E[x^2] - m^2, cancelling 1e6 against
#    1e6) would be off by O(1) there.
#  * GRU: each step feeds the previous h through a 256-term matrix-vector product and the gates; the recurrence is contractive (|dh'/dh| < 1 for
#    these weights), so rounding does not compound step over step.  The first GPU run measured at most 2.6e-6 (generic kernel, 256 steps);
#    2e-5, the conv tests' tolerance, leaves a 7x margin.
TOL_ATTN = 1e-4
TOL_LN = 2e-5
TOL_LN_OFFSET = 128.0
TOL_GRU = 2e-5
U32 = 2.0 ** -24                   # fp32 unit roundoff


class Ops(Handle):
    def run(self, case, reps=1, graph=0):
        """-> (rc, variant, output interior [B][C][T] as float32, list of problems, status words)"""
        s = OpSpec()
        for k, v in case.spec.items():
            setattr(s, k, v)
        s.reps, s.graph = reps, graph
        geo = (C.c_longlong * 16)()
        assert self.L.rvc_debug_op(self.h, C.byref(s), None, None, None, None, None, geo) == 0
        gx, gy = list(geo[0:8]), list(geo[8:16])
        B, T, xh = case.B, case.T, case.spec["x_halo"]
        x = np.full(gx[0], SENT_X, np.float32)
        x[index(gx, B, 0, gx[2], T + 2 * xh) - xh] = 0.0            # halos zero, as the plan's arena leaves them
        xi = index(gx, B, 0, gx[2], T)
        x[xi] = case.x
        y, yi = None, None
        if case.op != OP_LN:
            y = np.full(gy[0], SENT_Y, np.float32)
            yi = index(gy, B, 0, gy[2], T)
        status = np.full(B, SENT_STATUS, np.int32)
        x0, y0 = x.copy(), None if y is None else y.copy()
        rc = self.L.rvc_debug_op(self.h, C.byref(s), ptr(case.w0), ptr(case.w1), ptr(x), ptr(y), ptr(status), geo)
        if rc != 0:
            return rc, None, None, [self.last_error()], None
        var = self.last_kernel()
        bad = []
        # what may change: the output's interior (LayerNorm: the input's, in place)
        tgt, t0, ti, g = (x, x0, xi, gx) if case.op == OP_LN else (y, y0, yi, gy)
        pos = stray(tgt, t0, ti)
        if pos.size:
            bad.append("%d floats written outside the output's interior (first at offset %d, row column %d; ld %d, T %d)" %
                       (pos.size, pos[0] - g[1], int((pos[0] - g[1]) % g[4]), g[4], T))
        if case.op != OP_LN and not same_bits(x, x0):
            bad.append("input tensor changed at %d positions" % int(np.count_nonzero(x.view(np.uint32) != x0.view(np.uint32))))
        if case.op != OP_GRU:
            status = None
        return rc, var, tgt[ti], bad, status


class Case:
    """one op at one shape: spec fields, host data (fp32 as uploaded) and the fp64 reference"""

    def __init__(self, op, B, T, label, long=False, **spec):
        self.op, self.B, self.T, self.label, self.long = op, B, T, label, long      # long: a file converter's window length (LONG_* below)
        self.spec = dict(op=op, streams=B, E=0, heads=1, T=T, window=0, C=0, H=0, x_halo=0, y_halo=0)
        self.spec.update(spec)
        self._data, self._d32 = None, None

    def __repr__(self):
        return self.label

    def _rng(self):
        return np.random.default_rng(zlib.crc32(self.label.encode()))

    def data(self):
        if self._data is None:
            self._data = getattr(self, "_data_%s" % FAMILY[self.op])(self._rng())
        return self._data

    def _data_attn(self, rng, rel=False):
        B, T, E, heads = self.B, self.T, self.spec["E"], self.spec["heads"]
        hd = E // heads
        # q, k ~ U(-a, a): logits q.k / sqrt(hd) have a standard deviation of a^2 / 3 = 13 -> about +-40
        qkv = rng.uniform(-6.2, 6.2, (B, 3 * E, T)).astype(np.float32)
        qkv[:, 2 * E:] /= 6.2                                              # v ~ U(-1, 1)
        if T > 2:
            qkv[:, :E, 0] = 0.0                                            # query 0: a row of equal scores (uniform softmax)
            for h in range(heads):                                         # key T // 2 dominates query 1: logit 40 against the others' ~13
                q1 = qkv[:, h * hd:(h + 1) * hd, 1].astype(np.float64)
                qkv[:, E + h * hd:E + (h + 1) * hd, T // 2] = (q1 * (40.0 * np.sqrt(hd) / np.sum(q1 * q1, axis=1, keepdims=True))).astype(np.float32)
        if self.long and T > 2 * self.spec["window"] + 8:
            # converter lengths: the dominant key of query 2 sits in the last column and that of query 3 in column 0 (a dropped tail tile, a padding
            # column taken for a key or a lost first column moves the output by O(1)); query T - 1 - window / 2 is query 2 again, so its weight
            # also sits on key T - 1 -- inside its relative window, which is clamped at the end of the sequence
            for h in range(heads):
                for qi, kj in ((2, T - 1), (3, 0)):
                    qq = qkv[:, h * hd:(h + 1) * hd, qi].astype(np.float64)
                    qkv[:, E + h * hd:E + (h + 1) * hd, kj] = (qq * (40.0 * np.sqrt(hd) / np.sum(qq * qq, axis=1, keepdims=True))).astype(np.float32)
            qkv[:, :E, T - 1 - self.spec["window"] // 2] = qkv[:, :E, 2]
        w0 = w1 = None
        if rel:
            w = self.spec["window"]
            w0 = rng.uniform(-1, 1, (2 * w + 1, hd)).astype(np.float32)
            w1 = rng.uniform(-1, 1, (2 * w + 1, hd)).astype(np.float32)
            ref = R.relpos_mha(qkv, heads, w0, w1, w)
        else:
            ref = R.mha(qkv, heads)
        return qkv, w0, w1, ref, np.ones(B)

    def d32(self):
        """deviation of the float32-numpy restatement from float64, in the metric of value_error (computed once)"""
        if self._d32 is None:
            self._d32 = value_error(self, self.ref32())
        return self._d32

    def tol(self):
        """the family's tolerance; a converter-length case whose float32 restatement does not fit a quarter of it gets 4 x that deviation instead (the rule
        of tests/test_gpu_stream_taps.py) -- never a wider constant"""
        return max(TOL[self.op], 4.0 * self.d32()) if self.long else TOL[self.op]

    def ref32(self):
        """the fp64 definition of this case evaluated in float32 numpy on the same inputs (attention and GRU): the base a tolerance is judged against"""
        x, w0, w1, _, _ = self.data()
        if self.op == OP_GRU:
            H = self.spec["H"]
            return R.gru_bidir(x, w0.reshape(2, 3 * H, H), w1.reshape(2, 3 * H), dtype=np.float32)
        if self.op == OP_REL:
            return R.relpos_mha(x, self.spec["heads"], w0, w1, self.spec["window"], dtype=np.float32)
        return R.mha(x, self.spec["heads"], dtype=np.float32)

    def _data_relpos(self, rng):
        return self._data_attn(rng, rel=True)

    def _data_ln(self, rng):
        B, T, Ch = self.B, self.T, self.spec["C"]
        x = rng.uniform(-1, 1, (B, Ch, T)).astype(np.float32) * np.float32(3.0)
        cond = np.ones(B)
        if B > 1:
            # stream 1: columns of mean 1e3 and spread 1 (the condition number |m| / s enters the bound, see TOL_LN_OFFSET)
            x[1] = (np.float32(1e3) + rng.uniform(-1, 1, (Ch, T))).astype(np.float32)
        g = rng.uniform(0.5, 1.5, Ch).astype(np.float32)
        b = rng.uniform(-0.5, 0.5, Ch).astype(np.float32)
        ref = R.layernorm(x, g, b)
        if B > 1:
            xs = x[1].astype(np.float64)
            cond[1] = max(1.0, TOL_LN_OFFSET * U32 * float(np.max(np.abs(xs.mean(axis=0)) / xs.std(axis=0))) / TOL_LN)
        return x, g, b, ref, cond

    def _data_gru(self, rng):
        B, T, H = self.B, self.T, self.spec["H"]
        whh = (rng.uniform(-1, 1, (2, 3 * H, H)) * (1.5 / np.sqrt(H))).astype(np.float32)
        bhh = rng.uniform(-0.5, 0.5, (2, 3 * H)).astype(np.float32)
        gi = rng.uniform(-2, 2, (B, 6 * H, T)).astype(np.float32)
        # saturation: a quarter of the units get gate pre-activations of +-25 over the middle third of the steps
        sat = rng.choice(6 * H, 6 * H // 4, replace=False)
        gi[:, sat, T // 3:max(T // 3 + 1, 2 * T // 3)] = np.float32(25.0) * np.sign(rng.uniform(-1, 1, (B, sat.size, 1))).astype(np.float32)
        ref = R.gru_bidir(gi, whh, bhh)
        return gi, whh.ravel().copy(), bhh.ravel().copy(), ref, np.ones(B)

    @property
    def x(self):
        return self.data()[0]

    @property
    def w0(self):
        return self.data()[1]

    @property
    def w1(self):
        return self.data()[2]


TOL = {OP_MHA: TOL_ATTN, OP_REL: TOL_ATTN, OP_LN: TOL_LN, OP_GRU: TOL_GRU}


def value_error(case, got):
    """max over streams of max |gpu - ref| / rms(ref), each divided by the stream's conditioning allowance (1 except for the large-mean LayerNorm
    stream)"""
    _, _, _, ref, cond = case.data()
    got = got.astype(np.float64)
    if not np.all(np.isfinite(got)):
        return np.inf
    per_stream = np.max(np.abs(got - ref).reshape(case.B, -1), axis=1) / cond
    return float(np.max(per_stream)) / max(float(np.sqrt(np.mean(ref * ref))), 1e-30)


# ------------------------------------------------------------------------------------------------------------------------------------------
# shapes and eligibility (restated from plan.hip)
@functools.lru_cache(None)
def attn_cases():
    out = []
    for hd, E in ((64, 128), (12, 24)):
        tmax = 499 if hd == 64 else 1455                   # the VALU kernel's LDS limit: (hd (T|1) + 16 (T|1) + 16 hd) floats <= 160 KB
        for T in (1, 15, 16, 17, 111, 128, 129, 255, 256, 257, 332, tmax):
            for B in (1, 3, 16, 20):
                if T >= 332 and B > 3:
                    continue                               # (long windows: the VALU kernel at any stream count; keep the reference cheap)
                out.append(Case(OP_MHA, B, T, "attn_hd%d_T%d_B%d" % (hd, T, B), E=E, heads=2))
    return out


def attn_rule(c):
    hd, T = c.spec["E"] // c.spec["heads"], c.T
    if hd == 64 and T <= 256:
        return ("mfma2" if T <= 128 else "mfma4") + ("_qloop" if c.B >= 16 else "")
    return "valu"


def attn_eligible(c, v):
    hd, T = c.spec["E"] // c.spec["heads"], c.T
    return {"mfma2": hd == 64 and T <= 128, "mfma4": hd == 64 and T <= 256, "valu": True}[v.replace("_qloop", "")]


def long_cases():
    """the converter-length cases of relative attention and GRU (tests/long_shapes.py; tests/test_op_ref.py holds their float32 restatements against a quarter
    of the tolerance on the CPU)"""
    return [c for c in relpos_cases() + gru_cases() if c.long]


@functools.lru_cache(None)
def relpos_cases():
    out = []
    for kc in (8, 96, 16):
        for w in (4, 10):
            for T in sorted({1, 2, w, w + 1, 2 * w + 1, 16, 17, 21, 32, 33, 35, 63, 64, 65, 155}):
                for B in ((1, 4, 5, 16) if kc != 96 else (1, 5, 16)):
                    out.append(Case(OP_REL, B, T, "relpos_kc%d_w%d_T%d_B%d" % (kc, w, T, B), E=2 * kc, heads=2, window=w))
    for kc, T, B in LONG_RELPOS:
        out.append(Case(OP_REL, B, T, "relpos_kc%d_w10_T%d_B%d" % (kc, T, B), long=True, E=2 * kc, heads=2, window=10))
    return out


def relpos_rule(c):
    kc, T = c.spec["E"] // 2, c.T
    return "mfma" if T <= 64 and kc % 16 == 0 else ("small" if T <= 64 else "valu")     # (the LDS bounds hold at every shape here)


def relpos_eligible(c, v):
    kc, T = c.spec["E"] // 2, c.T
    return {"mfma": T <= 64 and kc % 16 == 0, "small": T <= 64, "valu": True}[v]


@functools.lru_cache(None)
def ln_cases():
    out = []
    for Ch in (16, 48, 192, 256, 257, 768, 769, 1024):
        for T, halo in ((37, 0), (23, 4), (1, 4), (30, 0)):          # ragged last quad of 1, 3 and 2 columns; T = 23: one strip and a part
            for B in (1, 16, 20):
                out.append(Case(OP_LN, B, T, "ln_C%d_T%d_h%d_B%d" % (Ch, T, halo, B), C=Ch, x_halo=halo))
    return out


def ln_rule(c):
    # strips are eligible for every plan tensor (make_t1: ld and halo multiples of 4), so at >= 16 streams the tile kernel is never reached
    nr = (c.spec["C"] + 63) // 64
    if c.B >= 16:
        return "strip4" if nr <= 4 else ("strip12" if nr <= 12 else "strip16")
    return "ct4" if c.spec["C"] <= 256 else "ct16"


def ln_eligible(c, v):
    nr = (c.spec["C"] + 63) // 64
    return {"ct4": c.spec["C"] <= 256, "ct16": True, "tile": True, "strip4": nr <= 4, "strip12": nr <= 12, "strip16": True}[v]


@functools.lru_cache(None)
def gru_cases():
    out = []
    for H in (32, 256):
        for T in (1, 2, 32, 64, 160, 256, 257):
            for B in (1, 8, 9):
                if H == 256 and B == 9 and T in (2, 32, 160):
                    continue
                out.append(Case(OP_GRU, B, T, "gru_H%d_T%d_B%d" % (H, T, B), H=H))
    for H, T, B in LONG_GRU:
        out.append(Case(OP_GRU, B, T, "gru_H%d_T%d_B%d" % (H, T, B), long=True, H=H))
    return out


def gru_rule(c):
    return "multi" if gru_eligible(c, "multi") else "generic"


def gru_eligible(c, v):
    return v == "generic" or (c.spec["H"] == 256 and c.B <= 8 and c.T <= 256)


FAMILIES = {OP_MHA: (attn_cases, attn_rule, attn_eligible), OP_REL: (relpos_cases, relpos_rule, relpos_eligible),
            OP_LN: (ln_cases, ln_rule, ln_eligible), OP_GRU: (gru_cases, gru_rule, gru_eligible)}


@pytest.fixture(scope="module")
def ops():
    o = Ops()
    try:
        yield o
    finally:
        for h in HOOK.values():
            set_opt(h, None)
        o.close()


def _run_checked(ops, case, forced=None, **kw):
    """one run -> (variant, list of problems)"""
    if forced:
        set_opt(HOOK[case.op], forced)
    try:
        rc, var, got, bad, status = ops.run(case, **kw)
    finally:
        if forced:
            set_opt(HOOK[case.op], None)
    tag = "%s [%s]" % (case.label, forced or "rules")
    if rc != 0:
        return None, ["%s: rvc_debug_op failed (%d): %s" % (tag, rc, bad[0])]
    bad = ["%s [%s]: %s" % (case.label, var, b) for b in bad]
    e = value_error(case, got)
    if case.long:
        print("%s [%s]: max err / rms %.3e, float32 numpy %.3e, ratio %.2f (bound %.2e)" % (tag, var, e, case.d32(), e / case.d32(), case.tol()))
    if not e < case.tol():
        _, _, _, ref, _ = case.data()
        wi = np.unravel_index(int(np.argmax(np.abs(got.astype(np.float64) - ref))), ref.shape)
        bad.append("%s [%s]: max err / rms %.3e at %s (gpu %.7g, ref %.7g)" % (tag, var, e, wi, got[wi], ref[wi]))
    if status is not None and np.any(status != 0):
        bad.append("%s [%s]: status words %s" % (tag, var, status.tolist()))
    return var, bad


@pytest.mark.parametrize("op", [OP_MHA, OP_REL, OP_LN, OP_GRU], ids=lambda o: FAMILY[o])
def test_op_under_the_rules(ops, op):
    """every shape under the production rules: values, nothing else written, and the variant the rules pick; the set of variants reached over the
    shape list is the set the rules allow (LayerNorm: the tile kernel is never reached by a plan tensor -- forced below)"""
    cases_of, rule, _ = FAMILIES[op]
    seen, fails = set(), []
    for c in cases_of():
        var, bad = _run_checked(ops, c)
        fails += bad
        want = "%s_%s" % (FAMILY[op], rule(c))
        if var is not None and var != want:
            fails.append("%s: rules chose %s, expected %s" % (c.label, var, want))
        seen.add(var)
    allowed = {"%s_%s" % (FAMILY[op], v) for v in VARIANTS[op]} - ({"ln_tile"} if op == OP_LN else set())
    assert not fails and seen == allowed, "variants seen %s, expected %s\n  %s" % (sorted(map(str, seen)), sorted(allowed), "\n  ".join(fails[:40]))


@pytest.mark.parametrize("op,variant", [(op, v) for op in VARIANTS for v in VARIANTS[op]], ids=lambda x: x if isinstance(x, str) else FAMILY[x])
def test_forced_variant(ops, op, variant):
    """the hook runs its variant on every eligible shape (at 1 and at the largest stream count of each shape group) and refuses every other one"""
    cases_of, _, eligible = FAMILIES[op]
    fails, ran = [], 0
    for c in cases_of():
        if c.B not in (1, 5, 8, 9, 20) and not c.long:
            continue
        if eligible(c, variant):
            var, bad = _run_checked(ops, c, forced=variant)
            fails += bad
            ran += 1
            if var is not None and var != "%s_%s" % (FAMILY[op], variant):
                fails.append("%s: forced %s, ran %s" % (c.label, variant, var))
        else:
            set_opt(HOOK[op], variant)
            try:
                rc = ops.run(c)[0]
            finally:
                set_opt(HOOK[op], None)
            if rc != RVC_SHAPE:
                fails.append("%s: forced %s outside its eligibility returned %d, expected RVC_SHAPE" % (c.label, variant, rc))
    assert ran > 0 and not fails, "\n  ".join(fails[:40])


def test_hook_rejects_unknown_variant(ops):
    c = Case(OP_LN, 1, 5, "ln_unknown", C=16)
    set_opt("RVC_LN_KERNEL", "nonesuch")
    try:
        assert ops.run(c)[0] == RVC_SHAPE
    finally:
        set_opt("RVC_LN_KERNEL", None)


def test_attention_beyond_the_lds_limit_is_refused(ops):
    for hd, E, T in ((64, 128, 500), (12, 24, 1456)):
        assert ops.run(Case(OP_MHA, 1, T, "attn_lds_T%d" % T, E=E, heads=2))[0] == RVC_SHAPE


def test_relpos_attention_beyond_the_lds_limit_is_refused(ops):
    """return_length 351 is the last the synthesizer's attention holds at head size 96: 352 and 353 (one odd-padded row of 353) are refused and nothing is
    launched.  The rule is restated here (attn_valu_lds), so it cannot move without this test moving"""
    assert attn_valu_lds(96, 351) == 163392 <= LDS_LIMIT < attn_valu_lds(96, 352) == attn_valu_lds(96, 353) == 164288
    assert ops.run(Case(OP_REL, 1, 16, "relpos_lds_before", E=192, heads=2, window=10))[0] == 0
    before = ops.last_kernel()
    for T in (352, 353):
        for B in (1, 3):
            c = Case(OP_REL, B, T, "relpos_lds_T%d_B%d" % (T, B), E=192, heads=2, window=10)
            c._data = (np.zeros((B, 3 * 192, T), np.float32), np.zeros((21, 96), np.float32), np.zeros((21, 96), np.float32), None, None)
            rc, _, _, msg, _ = ops.run(c)
            assert rc == RVC_SHAPE and "LDS" in msg[0], (T, B, rc, msg)
            assert ops.last_kernel() == before, (T, B, ops.last_kernel())       # nothing was launched
    for v in ("mfma", "small"):                                                # ... under a forced variant too
        set_opt("RVC_RELPOS_KERNEL", v)
        try:
            assert ops.run(c)[0] == RVC_SHAPE
        finally:
            set_opt("RVC_RELPOS_KERNEL", None)


@pytest.mark.parametrize("B,T", [(1, 64), (8, 256), (3, 17)])
def test_gru_multi_repeated_and_replayed(ops, B, T):
    """gru_multi_kernel's hand-off tags: three eager launches of one plan (the tags advance by Tm per launch, granules of the previous launch are
    stale), a captured graph replayed twice (memset node + epoch 0 each time) and a single launch agree bit for bit, within tolerance, status 0"""
    c = Case(OP_GRU, B, T, "gru_reps_T%d_B%d" % (T, B), H=256)
    outs = []
    for reps, graph in ((1, 0), (3, 0), (2, 1)):
        rc, var, got, bad, status = ops.run(c, reps=reps, graph=graph)
        assert rc == 0 and not bad and var == "gru_multi", (reps, graph, rc, var, bad)
        assert np.all(status == 0), (reps, graph, status)
        assert value_error(c, got) < TOL_GRU, (reps, graph, value_error(c, got))
        outs.append(got.copy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "eager relaunch differs"
    assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32)), "graph replay differs"


@pytest.mark.parametrize("op", [OP_MHA, OP_REL], ids=lambda o: FAMILY[o])
def test_attention_graph_replay_matches_eager(ops, op):
    c = Case(OP_MHA, 3, 111, "attn_graph", E=128, heads=2) if op == OP_MHA else Case(OP_REL, 4, 35, "relpos_graph", E=192, heads=2, window=10)
    r1 = ops.run(c)
    r2 = ops.run(c, reps=2, graph=1)
    assert r1[0] == 0 and r2[0] == 0 and not r1[3] and not r2[3]
    assert np.array_equal(r1[2].view(np.uint32), r2[2].view(np.uint32))
