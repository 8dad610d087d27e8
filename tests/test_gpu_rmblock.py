"""One ConvBlockRes of RMVPE at a time -- rm_block_kernel (obs_rvc_amd/csrc/rmblock.hip.h: one launch per block on the shallow levels) and the unfused path of
add_res_block (c1 + shortcut as one launch and c2, or one launch per convolution; avgpool2_kernel) -- through rvc_debug_rm_block, which queues a block as
build_rmvpe queues it, against the float64 definition of tests/rmblock_ref.py.  Every run
  * fills each allocation (input, output or concat buffer, pooled tensor) with a sentinel, the image halos with zeros as the plan's arena leaves them, the lower
    half of a concat buffer with data of its own;
  * checks the values per stream: max |gpu - ref| / rms(ref) < TOL = 2e-5, the convolution tests' tolerance (tests/test_gpu_tiles.py), accepted because single
    precision alone stays below a quarter of it on exactly these inputs (tests/test_rmblock_ref.py, measured on the CPU: 1.8e-6 at most);
  * checks the pooled second result to the same bound against the pooled reference;
  * checks that nothing else was written: the input, the zero halos of the output and of the pooled tensor, the guards, the lower half of a concat buffer and the
    other streams' padding come back bit for bit;
  * checks which kernel ran (rvc_debug_last_kernel) against the rule restated in rmblock_ref.expected_kernel, so that the suite cannot pass by running everything
    unfused -- and runs the case again with RVC_RM_FUSE = 0 (pooling cases also with 3: fused, no pooling folded in): both against the reference and against
    each other (< 2 TOL).
Cases (rmblock_ref.FAMILIES): the model's shapes at 1 - 4 streams; tile edges (8x16 exactly one 16-channel tile, 9x17, 13x37, 5x7, 2x2, 1x1, 1x40, 40x1); pooling
edges (a half-outside last column tile, a tile width that keeps the pooling launch); channel counts the model does not use (48 -> 16 at 58 KB of LDS, 64 -> 16
declined, 64 output channels never fused, 128 -> 64 on a one-row image for the unfused path's tap pruning -- the 16 / 32-channel 1x40 cases do not reach it: the
planner keeps a host copy of the weights for pruning only from K = 1024 on); five streams forced; a graph replayed three times.  Data: Gaussian, all-zero input
(the border ring differs from the constant interior only through the zero padding of y1: the sharpest check of the kernel's `inside`), one constant per channel
scaled per stream.

First GPU run (MI355X), worst max |gpu - ref| / rms(ref) per family -- rm_block_kernel / pair / plain: model 1.71e-6 / 6.7e-7 / 7.4e-7, edges 1.71e-6 / 7.0e-7 /
6.4e-7, pool 1.40e-6 / 5.2e-7 / 5.3e-7, channels 1.27e-6 / 6.8e-7 / 9.7e-7, streams5 1.63e-6 / - / 6.7e-7; pooled second output 1.44e-6 from the block, 5.4e-7 from
the pooling launch; fused against unfused 1.82e-6.  Every case ran the kernel the rule predicts; nothing was written outside the interiors; the graph replays equal
the eager runs bit for bit.  The whole module: 9 s.
"""
import ctypes as C

import numpy as np
import pytest

import rmblock_ref as R
from common import set_opt
from debug_abi import Handle, RmBlockSpec, index, ptr, same_bits, stray
from test_gpu_tiles import TOL

pytestmark = pytest.mark.gpu

assert TOL == R.TOL
SENT_X, SENT_Y, SENT_P = np.float32(-7777.25), np.float32(5555.5), np.float32(3333.75)
MEASURED = {}                      # worst figures of this run, printed by every test before it asserts
_REF = {}                          # (label, streams, kind) -> (data, out, pooled): computed once, shared by the runs under every hook


def _note(key, value):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(value))


def _ref(case, streams, kind):
    key = (case.label, streams, kind)
    if key not in _REF:
        for k in [k for k in _REF if k[0] != case.label]:
            del _REF[k]            # (one case at a time)
        d = R.data_for(case, streams, kind)
        _REF[key] = (d,) + R.reference(case, d)
    return _REF[key]


def _padded(g, B):
    """every float of the padded images [B][C][H + 2][W + 2] of an allocation of geometry g"""
    return index(g, B, 0, g[2], g[3] + 2, H=g[7] + 2) - g[4] - 1


class Block(Handle):
    def run(self, case, streams, kind, graph=0, reps=1):
        """-> (kernel name, problems, out [B][cout][H][W], pooled or None, the whole y and p allocations)"""
        d, ref, pref = _ref(case, streams, kind)
        B, co = streams, case.cout
        s = RmBlockSpec(streams=B, cin=case.cin, cout=co, H=case.H, W=case.W, pool_in=case.pool_in, pool_out=case.pool_out, y_in_cat=case.cat, next=case.next,
                        rm_fuse=case.rm_fuse, graph=graph, reps=reps)
        geo = (C.c_longlong * 24)()
        assert self.L.rvc_debug_rm_block(self.h, C.byref(s), *([None] * 9), geo) == 0, self.last_error()
        gx, gy, gp = list(geo[0:8]), list(geo[8:16]), list(geo[16:24])
        assert (gx[2], gx[7], gx[3]) == (case.cin,) + d["x"].shape[2:] and (gy[2], gy[7], gy[3]) == (co * (2 if case.cat else 1), case.H, case.W)
        x = np.full(gx[0], SENT_X, np.float32)
        x[_padded(gx, B)] = 0.0
        x[index(gx, B, 0, case.cin, gx[3], H=gx[7])] = d["x"]
        y = np.full(gy[0], SENT_Y, np.float32)
        y[_padded(gy, B)] = 0.0
        yidx = index(gy, B, co if case.cat else 0, co, case.W, H=case.H)
        y[yidx] = SENT_Y
        if case.cat:               # the lower half: what the decoder's transposed convolution will have written there
            y[index(gy, B, 0, co, case.W, H=case.H)] = R.rng_for(case.label + "/lower").uniform(-1, 1, (B, co, case.H, case.W)).astype(np.float32)
        p, pidx = None, None
        if case.pool_out:
            assert (gp[2], gp[7], gp[3]) == (co, case.H // 2, case.W // 2)
            p = np.full(gp[0], SENT_P, np.float32)
            p[_padded(gp, B)] = 0.0
            pidx = index(gp, B, 0, co, gp[3], H=gp[7])
            p[pidx] = SENT_P
        x0, y0, p0 = x.copy(), y.copy(), None if p is None else p.copy()
        rc = self.L.rvc_debug_rm_block(self.h, C.byref(s), ptr(d["w1"]), ptr(d["b1"]), ptr(d["w2"]), ptr(d["b2"]), ptr(d["wsc"]), ptr(d["bsc"]), ptr(x), ptr(y), ptr(p), geo)
        if rc != 0:
            return "?", ["rvc_debug_rm_block failed (%d): %s" % (rc, self.last_error())], None, None, None, None
        name = self.last_kernel()
        bad = []
        if not same_bits(x, x0):
            bad.append("input tensor changed at %d positions" % int(np.count_nonzero(x.view(np.uint32) != x0.view(np.uint32))))
        pos = stray(y, y0, yidx)
        if pos.size:
            o = int(pos[0]) - (gy[1] - gy[4] - 1)          # from the padded origin of stream 0, channel 0
            where = "in the front guard" if o < 0 else "stream %d, channel %d, padded row %d, padded column %d" % (o // gy[5], o % gy[5] // gy[6], o % gy[6] // gy[4], o % gy[4])
            bad.append("%d floats written outside the output's interior (first: %s; interior rows 1..%d, columns 1..%d)" % (pos.size, where, case.H, case.W))
        if p is not None:
            pos = stray(p, p0, pidx)
            if pos.size:
                bad.append("%d floats written outside the pooled tensor's interior (first at offset %d from element 0; ld %d, cs %d, bs %d)" %
                           (pos.size, int(pos[0]) - gp[1], gp[4], gp[6], gp[5]))
        out, pooled = y[yidx], None if p is None else p[pidx]
        for what, got, want in (("output", out, ref), ("pooled output", pooled, pref)):
            if got is None:
                continue
            for b in range(B):
                rms = float(np.sqrt(np.mean(want[b] * want[b])))
                err = np.abs(got[b].astype(np.float64) - want[b])
                e = float(np.max(err)) / rms if np.all(np.isfinite(got[b])) else np.inf
                _note("%s %s" % (name.split("_")[0].split("+")[0], what), e)
                if not e < TOL:
                    wi = np.unravel_index(int(np.argmax(err)), err.shape)
                    bad.append("%s, stream %d: max err / rms %.3e at (channel, row, column) %s (gpu %.6g, ref %.6g); %d pixels above the bound" %
                               (what, b, e, wi, got[b][wi], want[b][wi], int(np.count_nonzero(err / rms >= TOL))))
        return name, bad, out, pooled, y, p


@pytest.fixture(scope="module")
def blk():
    b = Block()
    try:
        yield b
    finally:
        set_opt("RVC_RM_FUSE", None)
        b.close()
        print("\nmeasured: " + ", ".join("%s %.3e" % kv for kv in sorted(MEASURED.items())))


def _check(blk, case):
    fails, worst = [], {}
    for streams, kind in R.runs_of(case):
        _, ref, pref = _ref(case, streams, kind)
        outs = {}
        for hook in case.hooks:
            set_opt("RVC_RM_FUSE", hook)
            try:
                name, bad, out, pooled, _, _ = blk.run(case, streams, kind)
            finally:
                set_opt("RVC_RM_FUSE", None)
            want = R.expected_kernel(case.cin, case.cout, case.H, case.W, streams, case.sc, bool(case.rm_fuse), hook, bool(case.pool_in), bool(case.pool_out), bool(case.cat))
            tag = "%s @ %d streams, %s, RVC_RM_FUSE=%s [%s]" % (case.label, streams, kind, hook, name)
            if name != want:
                bad.append("ran %s, the rule says %s" % (name, want))
            fails += ["%s: %s" % (tag, b_) for b_ in bad]
            if out is not None:
                outs[hook] = (out, pooled)
                for got, want_ in ((out, ref), (pooled, pref)):
                    if got is not None:
                        e = max(float(np.max(np.abs(got[b].astype(np.float64) - want_[b]))) / float(np.sqrt(np.mean(want_[b] * want_[b]))) for b in range(streams))
                        worst[name] = max(worst.get(name, 0.0), e)
        # the fused and the unfused result against each other
        hs = list(outs)
        for h in hs[1:]:
            for got, other, want_ in ((outs[hs[0]][0], outs[h][0], ref), (outs[hs[0]][1], outs[h][1], pref)):
                if got is None:
                    continue
                for b in range(streams):
                    e = float(np.max(np.abs(got[b].astype(np.float64) - other[b]))) / float(np.sqrt(np.mean(want_[b] * want_[b])))
                    _note("fused vs unfused", e)
                    if not e < 2 * TOL:
                        fails.append("%s @ %d streams, %s: RVC_RM_FUSE=%s and =%s differ by %.3e of rms in stream %d" % (case.label, streams, kind, hs[0], h, e, b))
    print("\n%s: worst max err / rms %s" % (case.label, ", ".join("%s %.3e" % kv for kv in sorted(worst.items()))))
    return fails


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.label)
def test_block(blk, case):
    fails = _check(blk, case)
    assert not fails, "\n  " + "\n  ".join(fails[:40])


@pytest.mark.parametrize("label", ["m_16_16", "m_32_32_poolout_cat", "m_64_32", "e_13x37_32_16"])
def test_graph_replayed_three_times_equals_the_eager_run(blk, label):
    # captured once with the warming workgroup in the launch (next = 1), replayed three times: bit for bit the eager result, halos and guards included
    case = next(c for c in R.CASES if c.label == label)
    assert case.next == 1
    streams = case.streams[-1]
    name_e, bad_e, _, _, y_e, p_e = blk.run(case, streams, "gauss")
    name_g, bad_g, _, _, y_g, p_g = blk.run(case, streams, "gauss", graph=1, reps=3)
    assert not bad_e and not bad_g, (bad_e, bad_g)
    assert name_e == name_g and name_e.startswith("rmb_"), (name_e, name_g)
    assert same_bits(y_e, y_g) and (p_e is None or same_bits(p_e, p_g))
