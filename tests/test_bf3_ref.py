"""CPU checks of tests/bf3_ref.py, the restatement of the split-bf16 GEMM that tests/test_gpu_bf3.py holds the device to:
  * the split itself against torch.bfloat16;
  * per GPU case: split_cost (what the three-term product alone costs against the fp64 definition), BOUND = 2 x split_cost + TOL, and that BOUND discriminates --
    each of the three broken variants (a term of the product missing) deviates from fp64 by at least 10 x BOUND on the very inputs the GPU test uses;
  * the index restatement of the weight panels and of the staged activation tile: A and B pair the same k, every value has one place."""
import numpy as np
import pytest
import torch

import bf3_ref as B3
from test_gpu_bf3 import bf3_must_run, conv_tile_takes, launch_shape


def test_split_is_torch_bfloat16_round_to_nearest_even():
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.uniform(-2, 2, 200000), rng.standard_normal(200000) * 1e-6, rng.standard_normal(200000) * 1e6,
                        [0.0, -0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e38]]).astype(np.float32)       # (1 + 2^-8, 1 + 3 * 2^-8: ties, to even both ways)
    t = torch.from_numpy(v)
    hi = t.to(torch.bfloat16).to(torch.float32)
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)
    mine_hi, mine_lo = B3.split(v)
    assert np.array_equal(mine_hi.view(np.uint32), hi.numpy().view(np.uint32))
    assert np.array_equal(mine_lo.view(np.uint32), lo.numpy().view(np.uint32))
    assert not np.any(mine_hi.view(np.uint32) & 0xFFFF) and not np.any(mine_lo.view(np.uint32) & 0xFFFF)
    # what the split keeps: 16 significant bits -- v - hi - lo is below 2^-17 |v| (half a unit of lo's last place, lo < 2^-8 |v|)
    nz = np.abs(v) > 1e-30
    rest = np.abs(v.astype(np.float64) - mine_hi - mine_lo)[nz] / np.abs(v.astype(np.float64))[nz]
    assert rest.max() <= 2.0 ** -17, rest.max()


@pytest.mark.parametrize("case", B3.ELIGIBLE, ids=lambda c: c.name)
def test_bound_discriminates(case):
    """split_cost and BOUND of the case; every broken variant is at least 10 x BOUND away from fp64, the full product within split_cost of it by definition"""
    for streams in case.streams:
        assert bf3_must_run(case, streams), (case.name, streams, launch_shape(case, streams))
        c = B3.cost(case, streams)
        print("%-24s @ %2d streams: split_cost %.3e  BOUND %.3e  broken / BOUND: %s" %
              (case.name, streams, c.split_cost, c.bound, "  ".join("%s %.1f" % (k, v / c.bound) for k, v in c.broken.items())))
        assert 0.0 < c.split_cost < c.bound
        for k, v in c.broken.items():
            assert v >= 10.0 * c.bound, (case.name, streams, k, v, c.bound)


@pytest.mark.parametrize("case", B3.INELIGIBLE, ids=lambda c: c.name)
def test_ineligible_cases_fail_the_rule_as_restated(case):
    for streams in case.streams:
        assert not bf3_must_run(case, streams), (case.name, streams)
    assert conv_tile_takes(case, case.streams[0]) == (case.name == "tile_first")


def test_the_rules_edge_is_250_workgroups():
    by = {c.name: c for c in B3.ELIGIBLE + B3.INELIGIBLE}
    a, b = launch_shape(by["lin_m128_edge250"], 1), launch_shape(by["edge249"], 1)
    assert a["wgs"] == 250 and b["wgs"] == 249 and a["N"] - b["N"] == 1 and b["N"] % 128 == 0
    assert {k: v for k, v in a.items() if k not in ("N", "wgs")} == {k: v for k, v in b.items() if k not in ("N", "wgs")}
    # every other ineligible case has its 250 workgroups: it is ONE other condition that keeps it off the kernel
    for c in B3.INELIGIBLE:
        if c.name != "edge249":
            assert launch_shape(c, c.streams[0])["wgs"] >= 250, c.name


@pytest.mark.parametrize("M,nchunks", [(128, 2), (700, 3), (160, 49), (33, 5)])
def test_panel_layout_pairs_the_same_k(M, nchunks):
    """A pure index test.  W[m][k] -> fragment-major fp32 panel -> bf3_pack_kernel's split panel -> what wload hands the MFMA as (row, k); the staged
    activation tile -> what kstep hands it as (column, k).  Both operands must give value i of lane the same k, a lane's row / column must be lane & 31 of its
    block, the packer must fill the panel exactly once and no two staged values may share LDS bytes."""
    K = nchunks * 16
    mt16, nblk = (M + 15) // 16, (M + 31) // 32
    # the fragment-major panel holds ids: m * K + k (rows M .. 16 * mt16 - 1 are the uploader's zero padding: id -1)
    frag = np.full(mt16 * nchunks * 256, -2, np.int64)
    m, k = np.meshgrid(np.arange(mt16 * 16), np.arange(K), indexing="ij")
    fi = B3.fragment_index(m, k, nchunks)
    assert np.array_equal(np.sort(fi.ravel()), np.arange(frag.size))                  # a bijection
    frag[fi] = np.where(m < M, m * K + k, -1)
    # the packer: element e, value i
    total = nblk * nchunks * 128
    assert total * 16 == B3.panel_bytes(M, nchunks)
    e, i = np.meshgrid(np.arange(total), np.arange(8), indexing="ij")
    src, half = B3.pack_source(e, i, M, nchunks)
    panel = np.where(src >= 0, frag[np.maximum(src, 0)], -1)                          # [e][i]: the id both halves of (m, k) carry
    # the kernel's reads: block, chunk, half, lane -> element; the MFMA's A operand takes (row lane & 31, k = a_k)
    seen = np.zeros(total, bool)
    for blk in range(nblk):
        for c in range(nchunks):
            for h in (0, 1):
                lane = np.arange(64)
                byte = B3.a_byte(blk, c, h, lane, nchunks)
                assert np.all(byte % 16 == 0) and byte.max() + 16 <= B3.panel_bytes(M, nchunks)
                el = byte // 16
                assert not seen[el].any()
                seen[el] = True
                assert np.all(half[el, 0] == h)
                ids = panel[el]                                                       # [lane][i]
                row = blk * 32 + (lane & 31)
                kk = B3.a_k(c, lane[:, None], np.arange(8)[None, :])
                want = np.where((row < M)[:, None], row[:, None] * K + kk, -1)
                assert np.array_equal(ids, want), (blk, c, h)
    assert seen.all()
    # the activation tile: 256 staging threads write, four waves read; per chunk
    for c in range(nchunks):
        owner = np.full(B3.HALF, -1, np.int64)                                        # byte -> k staged there (one half; hi and lo are written alike)
        colof = np.full(B3.HALF, -1, np.int64)
        for tid in range(256):
            for ii in range(8):
                off, kk = B3.stage_write(tid, c, ii)
                assert off + 2 <= B3.HALF and owner[off] == -1 and owner[off + 1] == -1
                owner[off] = owner[off + 1] = kk
                colof[off] = colof[off + 1] = tid % B3.BN
        cols = set()
        for wn in (0, 1):
            for nt in (0, 1):
                for lane in range(64):
                    for ii in range(8):
                        off, col = B3.b_read(wn, nt, lane, ii)
                        assert owner[off] == owner[off + 1] == B3.a_k(c, lane, ii), (c, wn, nt, lane, ii)       # B's k = A's k
                        assert colof[off] == col
                        cols.add(col)
        assert cols == set(range(B3.BN))
    assert B3.LDS_TILE_BYTES == 2 * 2 * 128 * 48
