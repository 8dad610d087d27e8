"""The head and the tail of the f0 branch and ContentVec's first layer -- mel_frontend_kernel, conv0_gn_gelu_kernel / conv0_gn_gelu_multi_kernel /
groupnorm_gelu_kernel, pitch_post_kernel, nsf_source_kernel -- through rvc_debug_front (the plan helpers add_mel_frontend / add_conv0_front /
add_pitch_post / add_nsf_source the models call), against the float64 definitions of tests/front_ref.py.  Each run checks the values, that nothing
else was written (every allocation is pre-filled with a sentinel, halos with zeros as the plan's arena leaves them; whatever is not the op's output
must come back bit for bit, inputs and other streams' state included), and, for conv0, which path ran against a restatement of the rule.

Tolerances (U32 = 2^-24, fp32 unit roundoff):
  * TOL_MEL: linear domain, per frame t and filter m: |exp(lm_gpu) - max(s_ref, 1e-5)| <= TOL_MEL x S, S = max(basis) x |windowed frame t|_2 x sqrt(band
    width of m): an fp32 FFT's error scales with the frame's norm, not with the bin's value.  Where s_ref > 1e3 TOL_MEL S the logarithms are compared as
    well: there the linear bound means a relative error below 1e-3, so |lm_gpu - log s_ref| <= 1.1e-3 (log(1 / (1 - 1e-3)) plus logf / expf rounding).
    TOL_MEL is 4 x the fp32 CPU oracle's own worst ratio against front_ref on exactly these inputs (radix-2 FFT, sequential projection; the kernel
    is radix-4 Stockham with shuffle folds): measured on the CPU 3.44e-6 (the 40 Hz tone on a bin centre; noise 4.0e-7, impulses up to 1.4e-6, the
    quiet stream 1.2e-6; the fp32 rounding of the stored logarithm, |lm| x 6e-8 of s, is part of it on both sides) -> 1.4e-5.  First GPU run: 4.09e-6 (the 40 Hz tone between
    two bins; noise 3.1e-7, the quiet stream 3.3e-6, impulses up to 1.7e-6); logarithms within 4.8e-6 where they are compared.
  * TOL_CONV0 = 2e-5 (max error / rms of the reference, per stream), the convolution tests' value.  The mean of a channel is an fp32 sum whose rounding,
    up to CHAIN_CONV0 x U32 x |mean|, reaches the output multiplied by gamma / sqrt(var + eps): a stream with a large mean and a small spread (the DC
    stream, the constant stream with variance 0 and sqrt(eps) = 3.2e-3 in its place) is held to CHAIN_CONV0 x U32 x max |mean| / sqrt(var + eps)
    instead, exactly as TOL_LN_OFFSET of test_gpu_ops.py (first GPU run: noise streams at most 2.3e-6, the DC and constant streams at most 0.30 of their allowance, every path).  CHAIN_CONV0 = 74: the 10 multiply-adds of an output, the longest run of sequential adds of
    a thread (one-channel kernel: 32 register values; groupnorm_gelu_kernel: 33 strided loads at To = 8193; multi kernel: 8) and the block
    reduction (6 shuffle steps + up to 16 wave partials), + the division and the subtraction: 10 + 33 + 22 + 9.
  * RTOL_F0 = 7e-6: cents = ps / ws are 9-term sums of non-negative products: relative error at most (9 + 1 + 1) U32 for ps (products, cents table entry,
    adds), 8 U32 for ws, 1 for the quotient: 20 U32.  f0 = 10 x 2^(cents / 1200) turns an absolute error d of cents into a relative ln 2 x d / 1200;
    cents <= 9000: ln 2 x 7.5 x 20 U32 = 6.2e-6; the exponent's division, powf (<= 2 ulp) and the pitch shift add 5 U32.  First GPU run: at most 2.2e-6 (64 streams, Tm = 512).
  * coarse pitch: integers equal wherever the float64 position is further than 1e-3 from a .5 boundary (fp32 logf x 1127 x 254 / 1622 carries ~1e-4);
    at most 1 % of the elements may be that close (254 boundaries x 2e-3 = 0.2 % of a sweep uniform in the position).
  * NSF sine: TOL_NSF_PHASE (turns) = 2 x the worst difference, over the tracks below at every (T, upp, f0 ratio), between a sequential single-precision
    restatement of the cumulative phase (front_ref.sine_phase(..., float32)) and the float64 one; the factor 2 is for the kernel's different grouping
    (per-thread segments + a block scan).  It is computed by the test itself on the CPU for the case at hand, so every case is held to its own
    measure (largest: 512 x 480 samples at 1100 Hz x 40 / 35).  The compared quantity, (atanh(out) - lin_b) / lin_w - 0.003 noise_ref against
    0.1 sin(2 pi phase_ref), gets 0.1 x 2 pi x TOL_NSF_PHASE + 1e-6 (sinf, tanhf and the inversion: a few ulp of values below 0.5).
    On the alternating tracks (voiced / unvoiced every frame or every 7 frames) the wraps of the interpolated phase do not follow the increments, the
    running phase reaches thousands of turns in every precision and single precision loses its fraction: the measure saturates at half a turn from
    155 frames on, so the sine of those tracks is held to nothing -- a property of the recipe in fp32, pinned on the CPU by
    test_front_ref.py::test_alternating_tracks_lose_the_phase_in_single_precision -- while their noise, halo and untouched-input checks stand; the
    test prints how many streams that is and asserts that no other track's allowance reaches the sine's amplitude.  Constant 1100 Hz over 512 x 480 samples measures 1.7e-2 turns, the glide 6.8e-5.  First GPU run: the
    largest error is 0.63 of its allowance; noise within 1.2e-6 of its amplitude.
    A wrap detected one sample early or late moves the phase by exactly 1 for one sample and is invisible behind the sine: nothing is excluded.
  * silence and every frame without signal: the floor's logarithm, exactly logf(1e-5f) as the device computes it (0xC13834F3) or correctly rounded.
  * NSF noise: |value - amplitude x normal_ref| <= 1e-5 x amplitude on unvoiced samples (fp32 logf / cosf on both sides).
"""
import ctypes as C
import zlib

import numpy as np
import pytest

import front_ref as R
from common import set_opt
from debug_abi import RVC_SHAPE, FrontSpec, Handle, StreamState, index, ptr, same_bits, stray
from oracle import oracle as O

pytestmark = pytest.mark.gpu

OP_MEL, OP_CONV0, OP_PITCH, OP_NSF = 4, 5, 6, 7
SENT = np.float32(-7777.25)
ST_PANIC = 1
U32 = 2.0 ** -24
TOL_MEL = 1.4e-5
TOL_CONV0 = 2e-5
CHAIN_CONV0 = 74.0
RTOL_F0 = 7e-6
MEASURED = {}                      # worst figures of this run, printed by every test before it asserts


def _note(key, value):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(value))


class Front(Handle):
    def run(self, fill, w0=None, w1=None, states=None, **spec):
        """fill(geo, bufs): writes the inputs into the sentinel-filled allocations.  -> (rc, bufs after, bufs before, geo [4][8], states after, kernel name)"""
        s = FrontSpec()
        for k, v in spec.items():
            setattr(s, k, v)
        geo = (C.c_longlong * 32)()
        rc = self.L.rvc_debug_front(self.h, C.byref(s), None, None, None, None, geo)
        if rc != 0:
            return rc, None, None, None, None, self.last_error()
        g = [list(geo[8 * j:8 * j + 8]) for j in range(4)]
        bufs = [np.full(max(int(q[0]), 0), SENT, np.float32) for q in g]
        fill(g, bufs)
        before = [b.copy() for b in bufs]
        B = s.streams
        st = (StreamState * B)()
        for b in range(B):
            d = (states or {}).get(b, {})
            st[b].uppower, st[b].stream_id, st[b].chunk, st[b].status = d.get("uppower", 1.0), d.get("stream_id", b), d.get("chunk", 0), 0
            C.memmove(st[b].cache, np.ascontiguousarray(d.get("cache", np.zeros(1024)), np.float32).ctypes.data, 4096)
        ptrs = (C.c_void_p * 4)(*[b.ctypes.data if b.size else None for b in bufs])
        rc = self.L.rvc_debug_front(self.h, C.byref(s), ptr(w0), ptr(w1), ptrs, st, geo)
        if rc != 0:
            return rc, None, None, g, None, self.last_error()
        out = [dict(status=int(st[b].status), cache=np.array(st[b].cache, np.float32)) for b in range(B)]
        return 0, bufs, before, g, out, self.last_kernel()


@pytest.fixture(scope="module")
def front():
    f = Front()
    try:
        yield f
    finally:
        set_opt("RVC_CONV0_KERNEL", None)
        f.close()
        print("\nmeasured: " + ", ".join("%s %.3e" % kv for kv in sorted(MEASURED.items())))


def _rng(label):
    return np.random.default_rng(zlib.crc32(label.encode()))


# ------------------------------------------------------------------------------------------------------------------------------------------
# mel front end
MEL_KINDS = ("noise", "imp0", "imp511", "imp512", "imp513", "implast", "tone40c", "tone40b", "tone1kc", "tone1kb", "tone7k9c", "tone7k9b", "silence", "quiet")
BIN_HZ = 16000.0 / 1024


def mel_signal(kind, n, frame, rng):
    """n samples whose last `frame` are the analysed signal; what lies in front of them is noise the kernel must not read"""
    x = np.zeros(frame)
    t = np.arange(frame)
    if kind == "noise":
        x = rng.uniform(-1, 1, frame)
    elif kind == "quiet":
        x = 1e-4 * rng.uniform(-1, 1, frame)
    elif kind.startswith("imp"):
        x[{"imp0": 0, "imp511": 511, "imp512": 512, "imp513": 513, "implast": frame - 1}[kind]] = 1.0
    elif kind.startswith("tone"):
        f = {"40": 40.0, "1k": 1000.0, "7k9": 7900.0}[kind[4:-1]]
        k = np.round(f / BIN_HZ) + (0.0 if kind.endswith("c") else 0.5)      # on a bin centre / between two bins
        x = 0.8 * np.sin(2 * np.pi * k * BIN_HZ * t / 16000.0 + 0.3)
    return np.concatenate([rng.uniform(-1, 1, n - frame), x]).astype(np.float32)


def mel_cases():
    out, i = [], 0
    for Tm in (32, 64, 96, 256, 1024):
        for B in (1, 3, 20):
            for extra in (0, 777):
                out.append((Tm, B, extra, i))
                i += 5
    return out


LOGF_FLOOR = np.float32(np.log(np.float64(np.float32(1e-5))))                  # logf(1e-5f), correctly rounded
# The device's logf is faithful to OpenCL's accuracy for log (<= 3 ulp), not correctly rounded: the MI355X returns 0xC13834F3 (-11.512927), two steps
# below the correctly rounded 0xC13834F1.  A floored value must be exactly one of these two constants
LOGF_FLOORS = np.array([int(LOGF_FLOOR.view(np.uint32)), 0xC13834F3], np.uint32).view(np.float32)
assert int(LOGF_FLOOR.view(np.uint32)) == 0xC13834F1


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for float32 a [..] and float32 scalars b, c: the product is exact in float64; its sum with c is rounded to 53
    bits, and where that lands exactly on the midpoint of two float32 values the residual of the sum (two-sum) decides the direction"""
    p = a.astype(np.float64) * np.float64(b)
    c = np.float64(c)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    bits = s.view(np.uint64)
    tie = ((bits & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (e != 0)
    if tie.any():
        trunc = (bits & ~np.uint64(0x1FFFFFFF)).view(np.float64).astype(np.float32)      # towards zero (exact)
        away = np.nextafter(trunc, np.where(s > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        r = np.where(tie, np.where(np.sign(e) == np.sign(s), away, trunc), r)
    return r


def mel_scale(frame_norm):
    basis = R.mel_basis()
    bw = np.count_nonzero(basis, axis=1)
    return basis.max() * np.sqrt(bw)[:, None] * frame_norm[None, :]


def mel_ratio(lm, x, frame):
    """lm [128][Tm] (fp32 logarithms of some implementation) against the reference: worst |exp(lm) - max(s, 1e-5)| / S and worst |lm - log s| where
    s > 1e3 TOL_MEL S"""
    s, norm = R.mel_linear(x, frame)
    S = np.maximum(mel_scale(norm), 1e-30)
    # (the kernel's floor is the fp32 constant: a value sitting on it is taken as that constant, not as exp of its rounded logarithm)
    lin = np.abs(np.where(np.isin(lm, LOGF_FLOORS), np.float64(np.float32(1e-5)), np.exp(lm.astype(np.float64))) - np.maximum(s, np.float64(np.float32(1e-5)))) / S
    lin = np.where(mel_scale(norm) > 0, lin, np.where(np.isin(lm, LOGF_FLOORS), 0.0, np.inf))
    big = s > 1e3 * TOL_MEL * S
    lg = np.max(np.abs(lm.astype(np.float64) - np.log(np.maximum(s, np.float64(np.float32(1e-5))))), where=big, initial=0.0)
    return float(lin.max()), float(lg)


@pytest.mark.parametrize("Tm,B,extra,k0", mel_cases(), ids=lambda v: str(v))
def test_mel_frontend(front, Tm, B, extra, k0):
    frame = 160 * (Tm - 1)
    n = frame + extra
    rng = _rng("mel_%d_%d_%d" % (Tm, B, extra))
    kinds = [MEL_KINDS[(k0 + b) % len(MEL_KINDS)] for b in range(B)]
    xs = [mel_signal(k, n, frame, rng) for k in kinds]
    scale, shift = np.float32(0.37), np.float32(-1.25)

    def fill(g, bufs):
        bufs[0][:B * n] = np.concatenate(xs)
        gi = g[2]
        for b in range(B):                                                   # the image's one-pixel halo is zero, as the arena leaves it
            base = gi[1] + b * gi[5] - gi[4] - 1
            bufs[2][base:base + (Tm + 2) * gi[4]] = 0.0

    rc, bufs, before, g, _, _ = front.run(fill, op=OP_MEL, streams=B, n=n, frame=frame, bn_scale=scale, bn_shift=shift)
    assert rc == 0
    assert g[1][0] == B * 128 * Tm and g[2][7] == Tm and g[2][3] == 128
    assert same_bits(bufs[0], before[0]), "audio changed"
    mel = bufs[1].reshape(B, 128, Tm)
    ii = g[2][1] + np.arange(B)[:, None, None] * g[2][5] + np.arange(Tm)[None, :, None] * g[2][4] + np.arange(128)[None, None, :]
    assert stray(bufs[2], before[2], ii).size == 0, "image written outside its interior"
    img = bufs[2][ii]                                                         # [B][Tm][128]
    lm_t = mel.transpose(0, 2, 1)
    unfused = (lm_t * scale).astype(np.float32) + shift
    fused = fma32(np.ascontiguousarray(lm_t), scale, shift)
    assert np.all((img.view(np.uint32) == unfused.view(np.uint32)) | (img.view(np.uint32) == fused.view(np.uint32))), "image is not log-mel * scale + shift"
    fails = []
    for b in range(B):
        assert np.all(np.isfinite(mel[b]))
        if kinds[b] == "silence":
            print("silence: values %s (logf(1e-5f) correctly rounded: %r)" % (np.unique(mel[b]).tolist(), float(LOGF_FLOOR)))
            assert np.unique(mel[b]).size == 1 and np.isin(mel[b, 0, 0], LOGF_FLOORS), "silence is not logf(1e-5f) everywhere"
            assert np.unique(img[b]).size == 1
        lin, lg = mel_ratio(mel[b], xs[b], frame)
        _note("mel_lin_" + kinds[b], lin)
        _note("mel_log", lg)
        print("mel Tm %d B %d stream %d %s: linear ratio %.3e, log diff %.3e" % (Tm, B, b, kinds[b], lin, lg))
        if not (lin <= TOL_MEL and lg <= 1.1e-3):
            fails.append((b, kinds[b], lin, lg))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------------------------------
# conv0 + GroupNorm + GELU
CONV0_TO = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8191, 8192, 8193)
CONV0_PATHS = ("conv0_multi4", "conv0_multi8", "conv0_one8", "conv0_one16", "conv0_one32", "conv0_generic")
CONV0_KINDS = ("noise", "dc", "const", "silence")


def conv0_cases(C0):
    out = []
    for To in CONV0_TO:
        for B in (1, 3, 4, 15, 16, 20):
            if C0 * To * B > 6_000_000:
                continue                                                     # (keep the float64 reference small where C and To are both large)
            out.append((C0, To, B, (To + B) % 5))
    return out


def conv0_cpw(C0, B):
    cpw = 16 if B >= 16 else (4 if B >= 4 else 2)
    while cpw > 1 and C0 % cpw:
        cpw //= 2
    return cpw


def conv0_eligible(C0, To, B, path):
    return {"multi": To <= 8192 and conv0_cpw(C0, B) > 1, "one": To <= 8192, "generic": True}[path]


def conv0_name(To, path):
    if path == "multi":
        return "conv0_multi4" if (To + 1023) // 1024 <= 4 else "conv0_multi8"
    if path == "one":
        nt = (To + 255) // 256
        return "conv0_one8" if nt <= 8 else ("conv0_one16" if nt <= 16 else "conv0_one32")
    return "conv0_generic"


def conv0_rule(C0, To, B):
    return conv0_name(To, "multi" if conv0_eligible(C0, To, B, "multi") else ("one" if To <= 8192 else "generic"))


def conv0_data(C0, To, B, extra):
    rng = _rng("conv0_%d_%d_%d" % (C0, To, B))
    L = 5 * (To - 1) + 10 + extra
    w = rng.standard_normal((C0, 10)) * 0.3
    w += (1.0 - w.sum(axis=1, keepdims=True)) / 10.0                          # every filter sums to ~1: a DC offset passes unchanged
    w = w.astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, C0).astype(np.float32), rng.uniform(-0.5, 0.5, C0).astype(np.float32)
    x = np.zeros((B, L), np.float32)
    kinds = [CONV0_KINDS[(b + To) % 4] for b in range(B)]
    for b, k in enumerate(kinds):
        if k == "noise":
            x[b] = rng.uniform(-1, 1, L)
        elif k == "dc":
            x[b] = 0.5 + 0.01 * rng.uniform(-1, 1, L)
        elif k == "const":
            x[b] = 0.25
        x[b, L - extra:] = 1e3                                                # behind the last window: must not enter the statistics
    ref = R.conv0_gn_gelu(x, w, 5, gamma, beta)
    y = R.conv0_raw(x, w, 5)
    cond = np.max(np.abs(y.mean(axis=2)) / np.sqrt(y.var(axis=2) + 1e-5), axis=1)
    cond = np.maximum(1.0, CHAIN_CONV0 * U32 * cond / TOL_CONV0)
    return L, w, gamma, beta, x, kinds, ref, cond


def conv0_run(front, C0, To, B, data, forced=None):
    L, w, gamma, beta, x, kinds, ref, cond = data

    def fill(g, bufs):
        bufs[0][:B * L] = x.ravel()

    if forced:
        set_opt("RVC_CONV0_KERNEL", forced)
    try:
        rc, bufs, before, g, _, name = front.run(fill, w0=w, w1=np.concatenate([gamma, beta]), op=OP_CONV0, streams=B, C=C0, L=L)
    finally:
        if forced:
            set_opt("RVC_CONV0_KERNEL", None)
    tag = "conv0 C %d To %d B %d [%s]" % (C0, To, B, forced or "rules")
    if rc != 0:
        return rc, None, ["%s: failed (%d): %s" % (tag, rc, name)]
    bad = []
    if not same_bits(bufs[0], before[0]):
        bad.append("%s: input changed" % tag)
    yi = index(g[1], B, 0, C0, To)
    if g[1][2] != C0 or g[1][3] != To:
        bad.append("%s: output geometry %s" % (tag, g[1]))
    n = stray(bufs[1], before[1], yi).size
    if n:
        bad.append("%s [%s]: %d floats written outside the output's interior" % (tag, name, n))
    got = bufs[1][yi].astype(np.float64)
    if not np.all(np.isfinite(got)):
        bad.append("%s [%s]: non-finite output" % (tag, name))
        return 0, name, bad
    for b in range(B):
        e = np.max(np.abs(got[b] - ref[b])) / max(float(np.sqrt(np.mean(ref[b] ** 2))), 1e-30)
        _note("conv0_%s_%s" % (kinds[b], name), e / cond[b])
        if not e / cond[b] < TOL_CONV0:
            bad.append("%s [%s]: stream %d (%s) max err / rms %.3e, allowed %.3e" % (tag, name, b, kinds[b], e, TOL_CONV0 * cond[b]))
        if kinds[b] in ("const", "silence") and not np.allclose(got[b], R.gelu(beta.astype(np.float64))[:, None], atol=TOL_CONV0 * cond[b]):
            bad.append("%s [%s]: stream %d (%s) is not gelu(beta)" % (tag, name, b, kinds[b]))
    return 0, name, bad


@pytest.mark.parametrize("C0", [512, 32, 6, 3])
def test_conv0_paths(front, C0):
    """every shape under the rules (values, nothing else written, the path the rules pick) and with every path forced through RVC_CONV0_KERNEL: run where
    eligible, refused with RVC_SHAPE elsewhere; the set of paths reached under the rules over all three channel counts is checked below"""
    fails, seen = [], set()
    for (_, To, B, extra) in conv0_cases(C0):
        data = conv0_data(C0, To, B, extra)
        rc, name, bad = conv0_run(front, C0, To, B, data)
        fails += bad
        if rc == 0:
            seen.add(name)
            if name != conv0_rule(C0, To, B):
                fails.append("C %d To %d B %d: rules chose %s, expected %s" % (C0, To, B, name, conv0_rule(C0, To, B)))
        for path in ("multi", "one", "generic"):
            rc, name, bad = conv0_run(front, C0, To, B, data, forced=path)
            if conv0_eligible(C0, To, B, path):
                fails += bad
                if rc == 0 and name != conv0_name(To, path):
                    fails.append("C %d To %d B %d: forced %s, ran %s" % (C0, To, B, path, name))
            elif rc != RVC_SHAPE:
                fails.append("C %d To %d B %d: forced %s outside its eligibility returned %d, expected RVC_SHAPE" % (C0, To, B, path, rc))
    print("conv0 C %d: paths under the rules %s; measured %s" % (C0, sorted(seen), {k: "%.2e" % v for k, v in MEASURED.items() if k.startswith("conv0")}))
    want = {conv0_rule(C0, To, B) for (_, To, B, _) in conv0_cases(C0)}
    assert not fails and seen == want, "paths seen %s, expected %s\n  %s" % (sorted(seen), sorted(want), "\n  ".join(fails[:40]))


def test_conv0_rules_reach_every_path():
    reach = {conv0_rule(C0, To, B) for C0 in (512, 32, 6, 3) for (_, To, B, _) in conv0_cases(C0)}
    assert reach == set(CONV0_PATHS)


def test_conv0_hook_rejects_unknown_variant(front):
    set_opt("RVC_CONV0_KERNEL", "nonesuch")
    try:
        assert conv0_run(front, 6, 2, 1, conv0_data(6, 2, 1, 0))[0] == RVC_SHAPE
    finally:
        set_opt("RVC_CONV0_KERNEL", None)


# ------------------------------------------------------------------------------------------------------------------------------------------
# pitch decode, cache, coarse pitch
# salience bins of the peaks: the ends, the zero padding's edge (3 / 4), both sides of every bin-group boundary of the kernel's split scan (multiples
# of 45 at Tm = 96, 90 at 256, 180 at 512), start = 44 / 45 and the last legal one (bin 347: start 351, start + 8 = 359)
PEAKS = (0, 3, 4, 40, 41, 44, 45, 89, 90, 134, 135, 179, 180, 224, 225, 269, 270, 314, 315, 347)
TH = np.float32(0.03)
COL_KINDS = tuple("peak%d" % p for p in PEAKS) + ("tie_far", "tie_4445", "tie_179180", "zero", "at_th", "above_th", "below_th")
UPPOWERS = [2.0 ** (k / 12.0) for k in range(-24, 25)] + [1.0]


def _bump(p, width=16):
    k = np.arange(360)
    return np.where(np.abs(k - p) < width, 0.5 * (1 + np.cos(np.pi * (k - p) / width)), 0.0)


def pitch_column(kind, rng):
    """-> (column [360] float32, number of tied maxima made on purpose)"""
    floor = rng.uniform(0.001, 0.003, 360)
    if kind.startswith("peak"):
        return (floor + rng.uniform(0.3, 0.95) * _bump(int(kind[4:]))).astype(np.float32), 1
    if kind.startswith("tie"):
        a, b = {"tie_far": (120, 200), "tie_4445": (44, 45), "tie_179180": (179, 180)}[kind]
        c = (floor + 0.6 * _bump(a)).astype(np.float32)
        c[b] = c[a] = np.float32(0.9)                                         # two equal maxima: the first wins
        return c, 2
    if kind == "zero":
        return np.zeros(360, np.float32), 360
    c = ((floor + 0.9 * _bump(150)) * 0.02).astype(np.float32)                 # maximum set exactly: the threshold is a strict >
    c[150] = {"at_th": TH, "above_th": np.nextafter(TH, np.float32(1)), "below_th": np.nextafter(TH, np.float32(0))}[kind]
    return c, 1


def pitch_salience(B, Tm, label, panic_stream=None):
    rng = _rng(label)
    sal = np.zeros((B, 360, Tm), np.float32)
    ties = np.ones((B, Tm), np.int64)
    for b in range(B):
        for t in range(Tm):
            sal[b, :, t], ties[b, t] = pitch_column(COL_KINDS[(t + 7 * b) % len(COL_KINDS)], rng)
    if panic_stream is not None:
        sal[panic_stream, :, Tm // 2] = (0.002 + 0.8 * _bump(348)).astype(np.float32)
    return sal, ties


def pitch_reference(sal, ties, ups):
    f0 = np.zeros((sal.shape[0], sal.shape[2]))
    panic = np.zeros(f0.shape, bool)
    for b in range(sal.shape[0]):
        f0[b], panic[b] = R.decode_pitch(sal[b], float(TH), ups[b])
        # every argmax is decided by more than 1e-4 (the maximum against the largest value that is not one of the maxima tied on purpose)
        s = np.sort(sal[b].astype(np.float64), axis=0)
        runner = np.take_along_axis(s, (359 - ties[b])[None, :].clip(0), axis=0)[0]
        margin = np.where(ties[b] >= 360, np.inf, s[-1] - runner)
        assert np.all(margin > 1e-4), (b, float(margin.min()))
    return f0, panic


def pitch_run(front, sal, ups, update=0, shift=0, read_start=0, Rr=0, caches=None, graph=0):
    B, _, Tm = sal.shape

    def fill(g, bufs):
        gs = g[0]
        rows = gs[1] + np.arange(B)[:, None] * gs[5] + np.arange(360)[None, :] * gs[6]
        bufs[0][(rows[:, :, None] + np.arange(Tm)[None, None, :])] = sal

    states = {b: dict(uppower=ups[b], stream_id=b, chunk=3, cache=None if caches is None else caches[b]) for b in range(B)}
    for d in states.values():
        if d["cache"] is None:
            del d["cache"]
    return front.run(fill, states=states, op=OP_PITCH, streams=B, Tm=Tm, update=update, shift=shift, cache_start=1028 - Tm, read_start=read_start, R=Rr, graph=graph)


def check_f0(got, ref):
    """worst relative error; zeros must be zeros"""
    assert np.all(np.isfinite(got)), "non-finite f0"
    z = ref == 0.0
    assert np.array_equal(got == 0.0, z), "unvoiced frames differ: gpu %d, reference %d" % (np.count_nonzero(got == 0), np.count_nonzero(z))
    return float(np.max(np.abs(got[~z] - ref[~z]) / ref[~z], initial=0.0))


@pytest.mark.parametrize("Tm", [30, 32, 64, 95, 96, 256, 512, 1024])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_pitch_decode(front, B, Tm):
    """(Tm = 30 and 95: rows padded to a multiple of 4, so the salience's row stride and stream stride differ from Tm and 360 Tm; the padding columns hold
    the sentinel, which is larger in magnitude than any salience and would win an argmax that read them)"""
    sal, ties = pitch_salience(B, Tm, "pitch_%d_%d" % (B, Tm))
    ups = [UPPOWERS[(3 * b + Tm) % len(UPPOWERS)] for b in range(B)]
    ref, panic = pitch_reference(sal, ties, [float(np.float32(u)) for u in ups])
    assert not panic.any()
    caches = [np.arange(1024, dtype=np.float32) + np.float32(0.25 + b) for b in range(B)]
    rc, bufs, before, g, st, _ = pitch_run(front, sal, ups, caches=caches)
    assert rc == 0
    assert g[0][4] == (Tm + 3) // 4 * 4 and g[0][5] == 360 * g[0][4]
    assert same_bits(bufs[0], before[0]), "salience changed"
    e = check_f0(bufs[1].reshape(B, Tm).astype(np.float64), ref)
    _note("f0_rel", e)
    print("pitch decode B %d Tm %d: worst relative f0 error %.3e" % (B, Tm, e))
    assert e <= RTOL_F0
    for b in range(B):                                                       # update = 0: status clear, the cache bit-identical
        assert st[b]["status"] == 0 and same_bits(st[b]["cache"], caches[b])


@pytest.mark.parametrize("Tm", [32, 96, 1024])
def test_pitch_cache(front, Tm):
    B, Rr = 5, 21
    sal, ties = pitch_salience(B, Tm, "cache_%d" % Tm)
    ups = [UPPOWERS[(5 * b + 11) % len(UPPOWERS)] for b in range(B)]
    ref, _ = pitch_reference(sal, ties, [float(np.float32(u)) for u in ups])
    caches = [(np.arange(1024, dtype=np.float32) * np.float32(0.5) + np.float32(60 + b)) for b in range(B)]
    for shift in (0, 1, 16, 30, 1024):
        for read_start in (0, 1024 - Rr):
            rc, bufs, before, g, st, _ = pitch_run(front, sal, ups, update=1, shift=shift, read_start=read_start, Rr=Rr, caches=caches)
            assert rc == 0 and same_bits(bufs[0], before[0])
            f0 = bufs[1].reshape(B, Tm)
            assert check_f0(f0.astype(np.float64), ref) <= RTOL_F0
            pitch = bufs[3].view(np.int32).reshape(B, Rr)
            for b in range(B):
                want, pf = R.update_cache(caches[b], f0[b], shift, 1028 - Tm, read_start, Rr)
                assert st[b]["status"] == 0
                assert same_bits(st[b]["cache"], want.astype(np.float32)), (shift, read_start, b)
                assert same_bits(bufs[2].reshape(B, Rr)[b], pf.astype(np.float32)), (shift, read_start, b)
                ci, dist = R.coarse_pitch(pf)
                assert np.array_equal(pitch[b][dist > 1e-3], ci[dist > 1e-3])
    # eager equals one graph launch bit for bit
    a = pitch_run(front, sal, ups, update=1, shift=16, read_start=0, Rr=Rr, caches=caches)
    b2 = pitch_run(front, sal, ups, update=1, shift=16, read_start=0, Rr=Rr, caches=caches, graph=1)
    assert a[0] == 0 and b2[0] == 0 and all(same_bits(p, q) for p, q in zip(a[1], b2[1])) and all(same_bits(p["cache"], q["cache"]) for p, q in zip(a[4], b2[4]))


def test_pitch_panic_is_per_stream(front):
    """an argmax at bin 348 (start 352: start + 8 = 360, out of bounds in the reference) in ONE stream of five raises ST_PANIC in that stream's status word
    only; the other four streams are decoded as ever"""
    B, Tm, who = 5, 64, 2
    sal, ties = pitch_salience(B, Tm, "panic", panic_stream=who)
    ref, panic = pitch_reference(sal, ties, [1.0] * B)
    assert panic.sum() == 1 and panic[who, Tm // 2]
    rc, bufs, before, g, st, _ = pitch_run(front, sal, [1.0] * B)
    assert rc == 0
    assert [s["status"] for s in st] == [ST_PANIC if b == who else 0 for b in range(B)]
    got = bufs[1].reshape(B, Tm).astype(np.float64)
    keep = np.arange(B) != who
    assert check_f0(got[keep], ref[keep]) <= RTOL_F0
    ok = ~panic[who]
    assert check_f0(got[who][ok], ref[who][ok]) <= RTOL_F0


def test_coarse_pitch(front):
    """the cache is pre-filled with chosen frequencies and read back through the coarse-pitch mapping (shift 0; the new f0 lands behind the slice)"""
    B, Tm, Rr = 64, 32, 990
    sal, _ = pitch_salience(B, Tm, "coarse")
    freqs = np.concatenate([[0.0, 49.9, 50.0, 500.0, 1100.0, 5000.0], np.geomspace(30.0, 1300.0, B * Rr - 6)]).astype(np.float32).reshape(B, Rr)
    caches = [np.concatenate([freqs[b], np.zeros(1024 - Rr, np.float32)]) for b in range(B)]
    rc, bufs, before, g, st, _ = pitch_run(front, sal, [1.0] * B, update=1, shift=0, read_start=0, Rr=Rr, caches=caches)
    assert rc == 0
    assert same_bits(bufs[2].reshape(B, Rr), freqs)
    got = bufs[3].view(np.int32).reshape(B, Rr)
    want, dist = R.coarse_pitch(freqs)
    clear = dist > 1e-3
    print("coarse pitch: %.3f %% of %d elements within 1e-3 of a boundary; mismatches elsewhere %d" % (100 * np.mean(~clear), clear.size, np.count_nonzero(got[clear] != want[clear])))
    assert np.mean(~clear) <= 0.01
    assert np.array_equal(got[clear], want[clear])
    assert got.min() >= 1 and got.max() <= 255 and got[0, 0] == 1 and got[0, 2] == 1 and got[0, 3] == 255 and got[0, 5] == 255
    assert np.all(np.abs(got - want) <= 1)


# ------------------------------------------------------------------------------------------------------------------------------------------
# NSF source
NSF_SHAPES = ((1, 480), (2, 400), (21, 480), (35, 400), (155, 320), (512, 480))
NSF_TRACKS = ("unvoiced", "c55", "c440", "c1100", "glide", "alt1", "alt7", "over_sr")
NSF_SEED = 20240611


def nsf_track(kind, T, sr):
    t = np.arange(T)
    if kind == "unvoiced":
        f = np.zeros(T)
    elif kind.startswith("c"):
        f = np.full(T, float(kind[1:]))
    elif kind == "glide":
        f = np.geomspace(80.0, 800.0, T)
    elif kind == "alt1":
        f = np.where(t % 2 == 0, 220.0, 0.0)
    elif kind == "alt7":
        f = np.where((t // 7) % 2 == 0, 330.0, 0.0)
    else:
        f = np.full(T, 150.0)
        f[T // 2] = sr * 1.25 + 100.0                                          # one frame above the sample rate: the increment is taken mod 1
    return f.astype(np.float32)


def nsf_run(front, f0, upp, sr, lin, ratio, ids, graph=0, halo=6):
    B, T = f0.shape

    def fill(g, bufs):
        bufs[0][:] = f0.ravel()
        gy = g[1]
        for b in range(B):
            row = gy[1] + b * gy[5]
            bufs[1][row - halo:row + gy[4] - halo] = 0.0                      # the row with its halos: zero, as the arena leaves it

    states = {b: dict(stream_id=ids[b][0], chunk=ids[b][1]) for b in range(B)}
    return front.run(fill, states=states, op=OP_NSF, streams=B, T=T, upp=upp, x_halo=halo, f0_num=ratio[0], f0_den=ratio[1], sr=float(sr), lin_w=lin[0], lin_b=lin[1],
                     seed=NSF_SEED, graph=graph)


def nsf_check(front, T, upp, B, lin, ratio, label):
    sr = upp * 100
    kinds = [NSF_TRACKS[(b + T) % len(NSF_TRACKS)] for b in range(B)]
    f0 = np.stack([nsf_track(k, T, sr) for k in kinds])
    ids = [(1000 + 3 * b, 7 + b % 2) for b in range(B)]
    rc, bufs, before, g, st, _ = nsf_run(front, f0, upp, sr, lin, ratio, ids)
    assert rc == 0, (label, rc)
    N = T * upp
    assert same_bits(bufs[0], before[0]), "pitch input changed"
    yi = index(g[1], B, 0, 1, N)
    assert stray(bufs[1], before[1], yi).size == 0, "source written outside its interior (halo, padding, guards)"
    out = bufs[1][yi].reshape(B, N).astype(np.float64)
    assert np.all(np.abs(out) < 1.0)
    sw = (np.arctanh(out) - np.float64(np.float32(lin[1]))) / np.float64(np.float32(lin[0]))
    worst_sine = worst_noise = worst_tol = 0.0
    vacuous = []                                                              # streams whose measured allowance reaches the sine's own amplitude
    for b in range(B):
        noise = O.philox_normal(NSF_SEED, ids[b][0], ids[b][1], 1, N).astype(np.float64)
        uv = np.repeat(f0[b] > 0, upp)
        if ratio[0] != ratio[1]:
            f64 = f0[b].astype(np.float64) * ratio[0] / ratio[1]
            f32 = (f0[b] * np.float32(ratio[0])) / np.float32(ratio[1])
        else:
            f64, f32 = f0[b].astype(np.float64), f0[b]
        ph = R.sine_phase(f64, upp, sr)
        d = R.sine_phase(f32, upp, sr, np.float32).astype(np.float64) - ph
        tol_phase = 2.0 * float(np.max(np.abs(d - np.round(d))))
        tol = 0.1 * 2 * np.pi * tol_phase + 1e-6
        if tol >= 0.1 and uv.any():
            vacuous.append(kinds[b])
        elif uv.any():
            worst_tol = max(worst_tol, tol)
        if uv.any():
            e = np.max(np.abs(sw[b][uv] - 0.003 * noise[uv] - 0.1 * np.sin(2 * np.pi * ph[uv])))
            worst_sine = max(worst_sine, e / tol)
            assert e <= tol, "%s stream %d (%s): sine error %.3e, allowed %.3e (measured fp32 phase error x 2: %.3e turns)" % (label, b, kinds[b], e, tol, tol_phase)
        if (~uv).any():
            e = np.max(np.abs(sw[b][~uv] - (0.1 / 3.0) * noise[~uv])) / (0.1 / 3.0)
            worst_noise = max(worst_noise, e)
            assert e <= 1e-5, "%s stream %d (%s): noise error %.3e of its amplitude" % (label, b, kinds[b], e)
    _note("nsf_sine_over_tol", worst_sine)
    _note("nsf_noise", worst_noise)
    print("nsf %s: sine error / allowance %.3f (largest allowance below the amplitude %.3e), noise error %.3e of its amplitude; %d of %d streams with a sine "
          "allowance that says nothing: %s" % (label, worst_sine, worst_tol, worst_noise, len(vacuous), B, sorted(set(vacuous))))
    # the sine check is empty only where single precision cannot hold the phase at all (test_front_ref.py pins that on the CPU): the alternating tracks
    assert set(vacuous) <= {"alt1", "alt7"}, vacuous
    return f0, ids, bufs


@pytest.mark.parametrize("T,upp", NSF_SHAPES)
@pytest.mark.parametrize("B", [1, 4, 64])
def test_nsf_source(front, B, T, upp):
    combos = [((1.0, 0.0), (1, 1)), ((2.5, 0.01), (40, 35)), ((2.5, 0.01), (1, 1)), ((1.0, 0.0), (40, 35))]
    for lin, ratio in (combos if B < 64 else combos[:2]):
        nsf_check(front, T, upp, B, lin, ratio, "T %d upp %d B %d lin %s ratio %s" % (T, upp, B, lin, ratio))


def test_nsf_streams_chunks_and_graph(front):
    T, upp, sr = 35, 400, 40000
    f0 = np.zeros((3, T), np.float32)                                         # unvoiced: the output is the noise alone
    a = nsf_run(front, f0, upp, sr, (1.0, 0.0), (1, 1), [(5, 9), (6, 9), (5, 10)])
    assert a[0] == 0
    out = a[1][1][index(a[3][1], 3, 0, 1, T * upp)].reshape(3, -1)
    assert not np.array_equal(out[0], out[1]), "two stream ids drew the same noise"
    assert not np.array_equal(out[0], out[2]), "chunk and chunk + 1 drew the same noise"
    f0 = np.stack([nsf_track(k, T, sr) for k in ("glide", "alt7", "c440")])
    a = nsf_run(front, f0, upp, sr, (2.5, 0.01), (40, 35), [(5, 9), (6, 9), (5, 10)])
    b = nsf_run(front, f0, upp, sr, (2.5, 0.01), (40, 35), [(5, 9), (6, 9), (5, 10)], graph=1)
    assert a[0] == 0 and b[0] == 0 and same_bits(a[1][1], b[1][1]), "eager and graph launch differ"


def test_nsf_refuses_more_than_512_frames(front):
    f0 = np.zeros((1, 513), np.float32)
    assert nsf_run(front, f0, 480, 48000, (1.0, 0.0), (1, 1), [(0, 0)])[0] == RVC_SHAPE
