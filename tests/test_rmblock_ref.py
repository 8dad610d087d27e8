"""tests/rmblock_ref.py (the fp64 reference, kernel rule and cases of tests/test_gpu_rmblock.py) checked on the CPU:
  * the block and the pooling agree with torch.float64 (conv2d with padding 1, relu, avg_pool2d) to 1e-12 at every shape of the GPU suite, tests/test_layer_ref.py's
    bound;
  * oracle/ exposes RMVPE only as a whole network (ora_pitch / the rm.* taps), no single block: the definition is compared instead with tests/torch_ref._cbr, the
    block of the torch network that tests/test_oracle_vs_torch.py pins the oracle's RMVPE to;
  * the all-zero input: the interior of the result is one constant per channel -- the value a block padded with ReLU(b1) would have everywhere -- and the border
    ring differs from it by thousands of tolerances, so a kernel with the wrong padding rule for y1 cannot pass;
  * the rule restated in rmblock_ref.fused_tile gives the tiles, LDS sizes and refusals the issue of this suite names;
  * single precision alone: the chain restated in torch float32 on exactly the GPU suite's inputs stays below a quarter of the GPU tolerance (TOL / 4 = 5e-6), the
    condition on which 2e-5 is accepted there.  Measured worst max |fp32 - fp64| / rms(fp64) over every case, stream count and data kind (printed by the
    test): model 1.57e-6 (64 -> 32, Gaussian), edges 1.39e-6, pool 1.35e-6, channels 1.78e-6 (128 -> 64, Gaussian), streams5 9.9e-7 -- 0.36 of the allowance at most."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rmblock_ref as R

TOL64 = 1e-12


def _t64(a):
    return None if a is None else torch.from_numpy(np.asarray(a, np.float64))


def _torch64(case, d):
    x = _t64(d["x"])
    if case.pool_in:
        x = F.avg_pool2d(x, 2, 2)
    y = F.relu(F.conv2d(x, _t64(d["w1"]), _t64(d["b1"]), padding=1))
    y = F.relu(F.conv2d(y, _t64(d["w2"]), _t64(d["b2"]), padding=1))
    y = y + (x if d["wsc"] is None else F.conv2d(x, _t64(d["wsc"])[:, :, None, None], _t64(d["bsc"])))
    return y.numpy(), (F.avg_pool2d(y, 2, 2).numpy() if case.pool_out else None)


@pytest.mark.parametrize("fam", list(R.FAMILIES))
def test_definition_matches_torch_float64_at_every_gpu_shape(fam):
    for case in R.FAMILIES[fam]:
        for kind in ("gauss", "zero"):
            d = R.data_for(case, case.streams[-1], kind)
            out, pooled = R.reference(case, d)
            tout, tpooled = _torch64(case, d)
            assert out.shape == tout.shape == (case.streams[-1], case.cout, case.H, case.W)
            assert np.max(np.abs(out - tout)) < TOL64, case.label
            if case.pool_out:
                assert pooled.shape == tpooled.shape == (case.streams[-1], case.cout, case.H // 2, case.W // 2)
                assert np.max(np.abs(pooled - tpooled)) < TOL64, case.label


def test_avgpool_drops_an_odd_last_row_and_column_as_torch_does():
    x = np.random.default_rng(3).uniform(-1, 1, (2, 3, 7, 9))
    assert np.max(np.abs(R.avgpool2(x) - F.avg_pool2d(torch.from_numpy(x), 2, 2).numpy())) < TOL64


def test_definition_matches_the_torch_network_the_oracle_is_pinned_to():
    import torch_ref
    for label in ("m_32_16", "m_16_16", "e_13x37_16_32"):
        case = next(c for c in R.CASES if c.label == label)
        d = R.data_for(case, 2, "gauss")
        t = {"c1.w": d["w1"], "c1.b": d["b1"], "c2.w": d["w2"], "c2.b": d["b2"]}
        if case.sc:
            t.update({"sc.w": d["wsc"], "sc.b": d["bsc"]})
        with torch.no_grad():
            got = torch_ref._cbr(t, "", torch.from_numpy(d["x"])).numpy()
        ref, _ = R.reference(case, d)
        assert np.max(np.abs(got - ref)) / np.sqrt(np.mean(ref * ref)) < R.TOL / 4, label


@pytest.mark.parametrize("label", ["m_16_16", "m_32_16", "e_5x7_32_32", "e_9x17_16_32"])
def test_zero_input_shows_the_padding_rule_of_y1(label):
    case = next(c for c in R.CASES if c.label == label)
    d = R.data_for(case, 1, "zero")
    ref, _ = R.reference(case, d)
    # what a block that pads y1 with ReLU(b1) (the value y1 has everywhere inside) computes: one constant per channel, border included
    y1 = np.maximum(d["b1"].astype(np.float64), 0.0)
    wrong = np.maximum(np.einsum("ocij,c->o", d["w2"].astype(np.float64), y1) + d["b2"], 0.0) + (0.0 if d["bsc"] is None else d["bsc"].astype(np.float64))
    rms = np.sqrt(np.mean(ref * ref))
    assert rms > 0.1
    assert np.max(np.abs(ref[0, :, 1:-1, 1:-1] - wrong[:, None, None])) < TOL64                    # the interior: constant, and the same under both rules
    ring = ref[0].copy()
    ring[:, 1:-1, 1:-1] = wrong[:, None, None]
    dev = np.abs(ring - wrong[:, None, None])
    assert np.max(dev) / rms > 1000 * R.TOL                                                       # the border: visible
    corners = dev[:, [0, 0, -1, -1], [0, -1, 0, -1]]
    assert np.all(np.max(corners, axis=0) / rms > 100 * R.TOL)                                    # ... at each of the four corners


def test_rule_restated_gives_the_tiles_and_refusals_the_suite_relies_on():
    ft, ek = R.fused_tile, R.expected_kernel
    assert ft(16, 16, 32, 128, False)[:5] == (1, 3, 2, 8, 16) and ft(32, 32, 16, 64, False)[:5] == (2, 2, 1, 4, 8)
    assert ft(16, 16, 5, 7, False)[3:5] == (5, 7) and ft(16, 32, 5, 7, True)[3:5] == (4, 7) and ft(16, 16, 1, 40, False)[3:5] == (1, 16)
    assert ft(48, 16, 9, 17, True)[5] == 59392 and ft(64, 16, 9, 17, True) is None and ft(64, 32, 16, 32, True)[5] == 38912       # LDS: 58 KB, 73 KB, 38 KB
    assert ft(32, 64, 9, 17, True) is None and ft(128, 64, 9, 17, True) is None
    assert ft(16, 16, 9, 17, False, rm_fuse=False) is None and ft(16, 16, 9, 17, False, rm_fuse=False, hook=2) and ft(16, 16, 9, 17, False, hook=0) is None
    assert ft(32, 32, 12, 24, False, pool_out=True) and ft(32, 32, 6, 4, False, pool_out=True) is None and ft(32, 32, 6, 4, False)
    assert ft(16, 16, 8, 16, False, pool_out=True) is None and ft(16, 16, 10, 8, False, pool_out=True) and ft(32, 32, 5, 8, False, pool_out=True) is None
    assert ek(16, 32, 16, 32, 1, True, pool_in=True) == "rmb_2_2_1+pool_in" and ek(16, 32, 16, 32, 1, True, pool_in=True, hook=3) == "rmb_2_2_1"
    assert ek(32, 32, 16, 32, 4, False, pool_out=True, y_in_cat=True) == "rmb_2_2_1+pool_out" and ek(32, 32, 6, 4, 2, False, pool_out=True) == "rmb_2_2_1"
    assert ek(64, 16, 9, 17, 2, True) == "pair" and ek(128, 64, 9, 17, 5, True) == "plain" and ek(16, 16, 9, 17, 1, False, hook=0) == "plain"
    assert ek(16, 32, 9, 17, 3, True, hook=0, y_in_cat=True) == "plain" and ek(16, 32, 9, 17, 1, True, hook=0, y_in_cat=True) == "pair"
    labels = [c.label for c in R.CASES]
    assert len(set(labels)) == len(labels)


@pytest.mark.parametrize("fam", list(R.FAMILIES))
def test_single_precision_alone_stays_below_a_quarter_of_the_gpu_tolerance(fam):
    worst, where = 0.0, None
    for case in R.FAMILIES[fam]:
        for streams, kind in R.runs_of(case):
            d = R.data_for(case, streams, kind)
            ref, pref = R.reference(case, d)
            got, pgot = R.block_f32(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], d["wsc"], d["bsc"], pool_in=bool(case.pool_in))
            pairs = [(got, ref)] + ([(pgot, pref)] if case.pool_out else [])
            for g, r in pairs:
                for b in range(streams):
                    rms = np.sqrt(np.mean(r[b] * r[b]))
                    assert rms > 1e-3, (case.label, streams, kind)
                    e = float(np.max(np.abs(g[b] - r[b]))) / rms
                    if e > worst:
                        worst, where = e, (case.label, streams, kind)
    print("\nfp32 restatement vs fp64, family %s: worst %.3e of rms at %s (allowance %.1e)" % (fam, worst, where, R.TOL / 4))
    assert worst < R.TOL / 4, (worst, where)
