"""CPU side of the mode-decision precompute pins (tests/test_md_pre_gpu.py): builds every case of md_common — each builder asserts on the way that the oracle's table equals a
plain numpy statement (int64) of the same operation on every slot — and asserts that the cases contain what the GPU tests say they cover.  Needs no GPU."""
import numpy as np
import pytest

import md_common as M


def test_numpy_grid_is_the_oracles_probe(orc):
    """numpy_grid against orc_md_subpel_probe position by position, every bank, on one block of noise: the independent statement of the banks the reference pins do not reach"""
    rng = np.random.default_rng(1)
    src, ref = M.Plane((0, 0, 64, 64), np.uint8, rng).freeze(), M.Plane((-24, -24, 88, 88), np.uint8, rng, shift=1).freeze()
    taps = M.interp_taps(orc)
    assert taps.shape == (6, 16, 8) and (taps.sum(2) == 128).all() and (taps[:, 0, 3] == 128).all()
    assert (taps[2][4::4, [0, 7]] != 0).all() and (taps[[0, 1, 3, 4, 5]][:, 4::4][:, :, [0, 7]] == 0).all()      # only the sharp kernels reach taps 0 and 7 at the grid's phases
    assert (np.abs(taps[:, 4::4]) < 128).all()                                                                    # the non-zero phases fit the kernels' int8 taps
    for bank in range(6):
        for (x, y, s, mx, my) in ((8, 16, 8, -3, 5), (16, 32, 16, 7, -6), (0, 0, 64, 2, 1)):
            c = M.Case(src=src, refs=[ref], pus=[(x, y, s, s)], mv=M.mv_words([[[mx]]], [[[my]]]), pic_w=64, pic_h=64, bank=bank)
            assert np.array_equal(M.oracle_grid_table(orc, c)[0, 0, 0], M.numpy_grid(src, ref, x, y, s, mx, my, bank, taps))


@pytest.mark.parametrize("bits", [8, 16])
def test_widths_case(orc, bits):
    c = M.widths_case(orc, bits)
    pus = c.pus
    assert len(pus) <= 128 and {p[2] for p in pus} == set(range(4, 65, 4))
    for w in range(4, 65, 4):
        rows = 64 // (w // 4)
        hs = {p[3] for p in pus if p[2] == w}
        assert hs == {min(v, 64) for v in (1, rows, rows + 1, 2 * rows + 1, 4 * rows, 4 * rows + 1, 64)}
        # exactly the widths of the table leave lanes past the last whole row of a step, and the list reaches the height from which that shows
        assert (64 % (w // 4) != 0) == (w in M.FIRST_WRONG_H)
        if w in M.FIRST_WRONG_H: assert M.FIRST_WRONG_H[w] == rows + 1 and max(hs) >= M.FIRST_WRONG_H[w]
    assert c.n_sb == 2 and len(c.refs) == 2 and int(c.refs[1].view(-24, -24, 176, 112).min()) == c.max == (255 if bits == 8 else 1023)
    assert (c.src.view(64, 0, 64, 64) == 0).all() and c.src.view(0, 0, 64, 64).any()
    assert (c.exp_sad[0] > 0).all()


@pytest.mark.parametrize("bits,grid", [(8, False), (16, False), (8, True)])
def test_edges_case(orc, bits, grid):
    c = M.edges_case(orc, bits, grid)
    done = (c.exp_grid[..., 0, 1] if grid else c.exp_sad) != M.NOT_COMPUTED
    extent = (lambda w, h: M.grid_extent(w)) if grid else M.sad_extent
    for sb, p, x, y, w, h in c.slots():
        lx, ty, rx, by = extent(w, h)
        for r in range(2):
            side, past = M.edge_slot(sb, p, r)
            mx, my = M.mv_xy(c.mv[sb, p, r])
            x_min, y_min, x_max, y_max = c.refs[r].box
            gap = {"left": x + mx + lx - x_min, "top": y + my + ty - y_min, "right": x_max - (x + mx + rx), "bottom": y_max - (y + my + by)}
            assert gap[side] == -past and all(v > 0 for s_, v in gap.items() if s_ != side) and bool(done[sb, p, r]) == (not past)
    for p in range(len(c.pus)):
        for side in range(4):
            assert sorted(bool(v) for v in done[side, p, :2]) == [False, True]
    assert len({r.box for r in c.refs}) == 3 and all(r.buf.shape[1] >= r.box[2] - r.box[0] + 2 * M.MARGIN for r in c.refs)
    if grid:
        assert (c.exp_grid[~done] == M.NOT_COMPUTED).all() and (c.exp_grid[done] != M.NOT_COMPUTED).any(-1).all() and c.exp_half.shape[-2:] == (9, 2)
    else:
        for q, (c0, c1) in enumerate(M.EDGE_PAIRS):
            assert np.array_equal(c.exp_avg[:, :, q] != M.NOT_COMPUTED, done[:, :, min(c0, c1)])
        assert {c0 for c0, _ in M.EDGE_PAIRS} == {c1 for _, c1 in M.EDGE_PAIRS} == {0, 1, 2}


@pytest.mark.parametrize("bits,shift", M.UNALIGNED)
def test_unaligned_case(orc, bits, shift):
    c = M.unaligned_case(orc, bits, shift)
    size = bits // 8
    assert c.src.stride == 203 and c.src.align() == (shift * size) & 3 != 0
    assert {c.src.align(x, y) for _, _, x, y, _, _ in c.slots()} == ({0, 1, 2, 3} if bits == 8 else {0, 2})
    assert all(r.stride % 2 == 1 and r.off % 2 == 1 for r in c.refs)
    # at least 16 readable bytes after the last row of the source, and the boxes well inside their buffers
    assert c.src.buf.size - (c.src.off + (c.pic_h - 1) * c.src.stride + c.pic_w) >= 16
    assert hasattr(c, "exp_grid") == (bits == 8)
    if bits == 8: assert (c.exp_grid[..., 0, 1] != M.NOT_COMPUTED).sum() > 250


@pytest.mark.parametrize("bank", range(6))
def test_banks_case(orc, bank):
    c = M.banks_case(orc, bank)
    assert set(np.unique(c.refs[0].view(-48, -48, 224, 160))) == {0, 255} == set(np.unique(c.refs[1].view(-48, -48, 224, 160)))
    for s in (8, 16, 32, 64):   # an edge of reference 1 runs through a PU of every size, both ways
        assert any(0 < int(c.refs[1].view(x + M.mv_xy(c.mv[sb, p, 1])[0], y + M.mv_xy(c.mv[sb, p, 1])[1], w, w).sum()) < 255 * w * w for sb, p, x, y, w, _ in c.slots() if w == s)
    if bank in (0, 2):
        assert M.banks_case_sensitive(orc, c) == {8, 16, 32, 64}
    if bank == 2:
        assert c.clips == dict(h_lo=True, h_hi=True, v_lo=True, v_hi=True)


@pytest.mark.parametrize("kind", M.CLOSED_KINDS)
def test_closed_forms(orc, kind):
    assert {p[2] for p in M.CLOSED_PUS} == {8, 16, 32, 64} and 64 * 64 * 65025 < 1 << 32
    for bank in range(6):
        c = M.closed_case(orc, kind, bank)
        assert (c.mv == 0).all()
        g = c.exp_grid[0, :, 0]
        if kind in ("max_on_0", "0_on_max"):
            assert [int(v) for v in g[:, :, 1].max(1)] == [s * s * 65025 for _, _, s, _ in M.CLOSED_PUS] and (g[:, :, 0] == 0).all()
        elif kind == "same": assert (g[:, 24] == 0).all()
        else: assert (g == 0).all() and int(c.src.view(0, 0, 64, 64).min()) == int(c.refs[0].view(-24, -24, 112, 112).max()) == 100


@pytest.mark.parametrize("name", M.GRID_LISTS)
def test_grid_list_case(orc, name):
    c = M.grid_list_case(orc, name)
    small = [p for p in c.pus if p[2] <= 16 and p[3] <= 16]          # the launcher's split: one wave / four waves
    large = [p for p in c.pus if p not in small]
    if name == "small_only": assert c.pus == [(0, 0, 8, 8)] and not large
    elif name == "large_only": assert c.pus == [(0, 0, 64, 64)] and not small
    else:
        assert {(0, 0, 4, 4), (8, 8, 12, 12)} < set(small) and {(0, 0, 16, 32), (0, 0, 32, 16)} < set(large)
        assert {p[2] for p in c.pus if p not in M.GRID_DECLINED} == {8, 16, 32, 64} and c.pus != sorted(c.pus) and c.pus != sorted(c.pus, reverse=True)
    for p, pu in enumerate(c.pus):
        assert (c.exp_grid[:, p] == M.NOT_COMPUTED).all() == (pu in M.GRID_DECLINED)
        assert (c.exp_half[:, p] == M.NOT_COMPUTED).all() == (pu in M.GRID_DECLINED)
    assert M.SENTINEL != M.NOT_COMPUTED and not (c.exp_grid == M.SENTINEL).any()
