"""GPU parity of the CDEF strength search's direction shortcuts (svt-av1_amd/csrc/cdef.hip): primary index 0 filters along direction 0, and the search
does not compute that variant again where it equals the block's own -- a block of direction 0 (all terms), of direction 4 (the secondary sums) -- in luma per
block, in chroma only when every live 4x4 block of a pass agrees.  Frames of one direction each, frames that mix directions inside a chroma pass, and the
direction chart; both distortion tables and the dir / var outputs against the oracle, 8-bit planes and 16-bit planes at depths 8 and 10."""
import numpy as np
import pytest

import cdef_common as cc
import test_cdef_gpu as tcg

pytestmark = pytest.mark.gpu

FORMATS = [pytest.param(8, np.uint8, id="u8-8"), pytest.param(8, np.uint16, id="u16-8"), pytest.param(10, np.uint16, id="u16-10")]
DAMPINGS = (3, 6)


def direction_lines(ph, pw, d):
    """line index of sample (y, x) along direction d, continued over the whole plane (cdef_common.chart_lines per block), >= 0"""
    I, J = np.mgrid[0:ph, 0:pw]
    return (I + J, I + J // 2, I, pw // 2 + I - J // 2, pw + I - J, ph // 2 - I // 2 + J, J, I // 2 + J)[d]


def one_direction_frame(w, h, bd, dtype, d, seed):
    """(src, rec, skip8): every plane holds full-range levels that are constant along direction d (one random level per line) under +-2 LSB of noise"""
    cs, mx = bd - 8, (1 << bd) - 1
    rng = np.random.default_rng([seed, d, bd])
    src, rec = [], []
    for pli in range(3):
        pw, ph = (w, h) if pli == 0 else (w // 2, h // 2)
        lines = direction_lines(ph, pw, d)
        clean = rng.integers(0, mx + 1, int(lines.max()) + 1)[lines]
        rec.append(np.ascontiguousarray(np.clip(clean + (rng.integers(-2, 3, (ph, pw)) << cs), 0, mx).astype(dtype)))
        src.append(np.ascontiguousarray(np.clip(clean + (rng.integers(-2, 3, (ph, pw)) << cs), 0, mx).astype(dtype)))
    skip8 = (rng.random((h // 8, w // 8)) < 0.25).astype(np.uint8)
    skip8[0, 0] = skip8[-1, -1] = 0
    return src, rec, skip8


def compare(hip, orc, src, rec, skip8, bd, dampings=DAMPINGS):
    e_dir, e_var = tcg.expected_dirs(orc, rec[0], bd, skip8)
    for damping in dampings:
        exp = cc.orc_search(orc, rec, src, bd, skip8, damping)
        got, g_dir, g_var = tcg.gpu_search_dirs(hip, rec, src, bd, skip8, damping)
        assert np.array_equal(got[0], exp[0]), ("Y", bd, damping, np.argwhere(got[0] != exp[0])[:5])
        assert np.array_equal(got[1], exp[1]), ("UV", bd, damping, np.argwhere(got[1] != exp[1])[:5])
        assert np.array_equal(g_dir, e_dir), ("dir", bd, damping, np.argwhere(g_dir != e_dir)[:5])
        assert np.array_equal(g_var, e_var), ("var", bd, damping, np.argwhere(g_var != e_var)[:5])
        assert exp[0].any() and exp[1].any()


@pytest.mark.parametrize("bd,dtype", FORMATS)
@pytest.mark.parametrize("d", range(8))
def test_one_direction_frame(hip, orc, bd, dtype, d):
    """72 x 72: 2 x 2 filter blocks, the last ones one block wide.  Directions 0 and 4 take the new paths, the others pin the general one."""
    src, rec, skip8 = one_direction_frame(72, 72, bd, dtype, d, seed=11)
    o_dir, _ = cc.orc_find_dir_frame(orc, rec[0], bd)
    live = skip8 == 0
    assert (o_dir[live] == d).sum() >= 0.9 * live.sum(), (d, np.bincount(o_dir[live], minlength=8))
    compare(hip, orc, src, rec, skip8, bd)


# the four luma blocks of one chroma pass (a 4 x 16 strip of 4x4 blocks), one row of 8x8 blocks each: direction per block, -1 = skipped
MIXED_ROWS = [(0, 0, 0, 0), (0, 3, 0, 3), (0, 0, 0, 5), (0, -1, 0, -1), (4, 4, 4, 4), (4, 4, 1, 4), (4, -1, 4, 4), (0, 4, 0, 4), (-1, 0, 6, -1)]


def mixed_frame(bd, dtype, seed):
    """72 x 72: block row r holds MIXED_ROWS[r] twice (the second half shifted by one block) and its first entry in the ninth column"""
    cs, mx = bd - 8, (1 << bd) - 1
    rng = np.random.default_rng([seed, bd])
    want = np.array([list(r) + list(r[1:] + r[:1]) + [r[0]] for r in MIXED_ROWS])
    src, rec = [], []
    for pli in range(3):
        n = 8 >> (pli != 0)
        p = np.zeros((9 * n, 9 * n), np.int64)
        for by in range(9):
            for bx in range(9):
                cell = cc.chart_cell(("lvl", max(int(want[by, bx]), 0)), bd, rng)
                p[n * by:n * by + n, n * bx:n * bx + n] = cell if pli == 0 else cell[::2, ::2]
        rec.append(np.ascontiguousarray(p.astype(dtype)))
        src.append(np.ascontiguousarray(np.clip(p + (rng.integers(-9, 10, p.shape) << cs), 0, mx).astype(dtype)))
    return src, rec, np.ascontiguousarray((want < 0).astype(np.uint8)), want


@pytest.mark.parametrize("bd,dtype", FORMATS)
def test_mixed_chroma_passes(hip, orc, bd, dtype):
    """Chroma passes whose four blocks are all of direction 0 / all of direction 4 (shortcut), with skipped blocks among them (still the shortcut), and with
    one or two blocks of another direction (the wave-uniform test must be false: the whole pass runs as before)."""
    src, rec, skip8, want = mixed_frame(bd, dtype, seed=13)
    o_dir, _ = cc.orc_find_dir_frame(orc, rec[0], bd)
    live = skip8 == 0
    assert (o_dir[live] == want[live]).sum() >= 0.9 * live.sum()
    kinds = set()
    for by in range(9):                       # what the passes of the first filter-block column hold, by the oracle's directions
        for half in range(2):
            ds = [int(o_dir[by, 4 * half + q]) for q in range(4) if live[by, 4 * half + q]]
            kinds.add((len(ds) == 4, tuple(sorted(set(ds)))))
    for need in ((True, (0,)), (False, (0,)), (True, (4,)), (False, (4,)), (True, (0, 4)), (True, (0, 3)), (True, (0, 5)), (True, (1, 4))):
        assert need in kinds, (need, sorted(kinds))
    compare(hip, orc, src, rec, skip8, bd)


@pytest.mark.parametrize("bd,dtype", FORMATS)
def test_chart_frame(hip, orc, bd, dtype):
    """cdef_common.make_chart_frame at 200 x 136: every direction, flat blocks (direction 0, var 0), ties, saturated samples, partial filter blocks."""
    src, rec, skip8 = cc.make_chart_frame(200, 136, bd, cc.CHART_SEED, dtype)
    compare(hip, orc, src, rec, skip8, bd, dampings=(3, 5))
