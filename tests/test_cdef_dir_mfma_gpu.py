"""GPU parity of the luma strength search's batched direction pass (svt-av1_amd/csrc/cdef.hip, find_dir_batch16): a wave finds the directions of its sixteen
blocks b = wave + 4n of a filter block with seven v_mfma_i32_16x16x64_i8 -- 0/1 line matrices built from kDirBinPix times the blocks' samples as signed bytes.
What can go wrong there and nowhere else: an entry of the line matrices, the lane maps of the three operands, the packing of the samples (rows 2g, 2g + 1 of
block n in lane (n, g); `>> coeff_shift`, `^ 0x80`), the weights per result register, the sums across lane groups (the tile that directions 2 and 6 share),
batches with absent or skipped blocks.  Every case compares dir, var and both distortion tables with the oracle, like tests/test_cdef_gpu.py, on 8-bit planes
and on 16-bit planes."""
import numpy as np
import pytest

import cdef_common as cc
import test_cdef_dir0_gpu as td0

pytestmark = pytest.mark.gpu

FORMATS = td0.FORMATS                                                                       # (8, u8), (8, u16), (10, u16)
FORMATS_2 = [pytest.param(8, np.uint8, id="u8-8"), pytest.param(10, np.uint16, id="u16-10")]
DAMPING = (4,)                                                                              # the direction pass does not depend on it


@pytest.mark.parametrize("bd,dtype", FORMATS)
@pytest.mark.parametrize("size", [(208, 144), (200, 136)])
def test_direction_chart(hip, orc, bd, dtype, size):
    """every direction, the exact 1/7, 2/6 and 3/5 cost ties, var == 0 blocks, an all-skip and a one-live-block filter block (tests/test_cdef_chart_cpu.py
    counts them for this seed)"""
    assert cc.CHART_SEED == 7
    src, rec, skip8 = cc.make_chart_frame(size[0], size[1], bd, 7, dtype)
    td0.compare(hip, orc, src, rec, skip8, bd, dampings=DAMPING)


def impulse_frame(bd, dtype, on, seed):
    """One 64 x 64 filter block of mid-grey (128 << cs: a zero byte in the matrix product) in which block k has only sample k set: to the maximum (`on`) or
    to 0.  The eight costs of block k are then a^2 times the weight of the line sample k lies on in each direction (a = 127 or -128), so a sample that the
    matrices put on another line, or a block, a row pair or a result register that lands in another lane, changes that block's var."""
    cs, mx = bd - 8, (1 << bd) - 1
    rng = np.random.default_rng([seed, bd, on])
    luma = np.full((64, 64), 128 << cs, np.int64)
    for k in range(64):
        luma[8 * (k >> 3) + (k >> 3), 8 * (k & 7) + (k & 7)] = mx if on else 0
    rec = [luma] + [rng.integers(100 << cs, 156 << cs, (32, 32)) for _ in range(2)]
    src = [np.clip(p + (rng.integers(-9, 10, p.shape) << cs), 0, mx) for p in rec]
    as_planes = lambda ps: [np.ascontiguousarray(p.astype(dtype)) for p in ps]
    return as_planes(src), as_planes(rec), np.zeros((8, 8), np.uint8)


@pytest.mark.parametrize("bd,dtype", FORMATS_2)
@pytest.mark.parametrize("on", [True, False], ids=["max", "zero"])
def test_impulse_per_sample(hip, orc, bd, dtype, on):
    src, rec, skip8 = impulse_frame(bd, dtype, on, seed=21)
    # the expectation stated with numpy (cdef_common.find_dir_costs), so that the frame is what the docstring says: block k's best cost is a^2 * 840 / (the
    # shortest line through sample k), and the 64 blocks do not all agree
    blocks = cc.luma_blocks(rec[0].astype(np.int64)).reshape(64, 8, 8)
    cost, best, var = cc.find_dir_costs(blocks, bd - 8)
    a2 = (127 if on else 128) ** 2
    lines = cc.chart_lines()
    for k in range(64):
        w_k = [cc.CHART_WEIGHTS[d][lines[d][k >> 3, k & 7]] for d in range(8)]
        assert list(cost[k]) == [a2 * w for w in w_k] and best[k] == int(np.argmax(w_k)), k
    assert len(set(zip(best.tolist(), var.tolist()))) >= 6
    o_dir, o_var = cc.orc_find_dir_frame(orc, rec[0], bd)
    assert np.array_equal(o_dir.reshape(-1), best) and np.array_equal(o_var.reshape(-1), var)
    td0.compare(hip, orc, src, rec, skip8, bd, dampings=DAMPING)


@pytest.mark.parametrize("bd,dtype", FORMATS)
def test_absent_blocks_72(hip, orc, bd, dtype):
    """72 x 72: the second filter-block column and row are one block wide / high (nbx / nby = 1), so a wave's batch there holds 15 or 16 absent blocks"""
    src, rec, skip8 = cc.make_chart_frame(72, 72, bd, 7, dtype)
    td0.compare(hip, orc, src, rec, skip8, bd, dampings=DAMPING)


@pytest.mark.parametrize("bd,dtype", FORMATS_2)
def test_skip_holes(hip, orc, bd, dtype):
    """128 x 128 noise with a random half of the blocks skipped: batches with holes; a skipped block reports direction 0 / variance 0 (tcg.expected_dirs)"""
    mx = (1 << bd) - 1
    rng = np.random.default_rng([31, bd])
    rec = [np.ascontiguousarray(rng.integers(0, mx + 1, (128 >> (p > 0), 128 >> (p > 0))).astype(dtype)) for p in range(3)]
    src = [np.ascontiguousarray(np.clip(p.astype(np.int64) + (rng.integers(-9, 10, p.shape) << (bd - 8)), 0, mx).astype(dtype)) for p in rec]
    skip8 = np.zeros(256, np.uint8)
    skip8[rng.permutation(256)[:128]] = 1
    skip8 = np.ascontiguousarray(skip8.reshape(16, 16))
    for fbr in range(2):
        for fbc in range(2):
            n = int(skip8[8 * fbr:8 * fbr + 8, 8 * fbc:8 * fbc + 8].sum())
            assert 0 < n < 64
    td0.compare(hip, orc, src, rec, skip8, bd, dampings=DAMPING)


@pytest.mark.parametrize("bd,dtype", FORMATS_2)
@pytest.mark.parametrize("d", range(8))
def test_saturated_stripes(hip, orc, bd, dtype, d):
    """0 / max stripes, three lines wide, along direction d (one line wide, directions 0 and 4 are the same checkerboard; three, the stripes fall differently
    into neighbouring blocks): whole lines of -128 bytes, among them lines of eight samples (a line sum of -1024, the largest magnitude there is), next to whole
    lines of 127"""
    mx = (1 << bd) - 1
    rng = np.random.default_rng([41, bd, d])
    rec = [np.ascontiguousarray(((td0.direction_lines(72 >> (p > 0), 72 >> (p > 0), d) // 3 % 2) * mx).astype(dtype)) for p in range(3)]
    src = [np.ascontiguousarray(np.clip(p.astype(np.int64) + (rng.integers(-40, 41, p.shape) << (bd - 8)), 0, mx).astype(dtype)) for p in rec]
    skip8 = np.zeros((9, 9), np.uint8)
    x = (cc.luma_blocks(rec[0][:64, :64].astype(np.int64)).reshape(64, 64) >> (bd - 8)) - 128
    on_line = cc.chart_lines()[d].reshape(64, 1) == np.arange(15)
    assert x.min() == -128 and x.max() == 127 and (x @ on_line).min() == -1024
    o_dir, _ = cc.orc_find_dir_frame(orc, rec[0], bd)
    assert (o_dir == d).mean() >= 0.9, np.bincount(o_dir.reshape(-1), minlength=8)
    td0.compare(hip, orc, src, rec, skip8, bd, dampings=DAMPING)
