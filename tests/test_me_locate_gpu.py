"""GPU parity of the integer search's locate step: the 8x8 / 16x16 PUs fold a unit of 8 candidates to (minimum SAD, unit) and the position inside the
winning unit is found afterwards (svt-av1_amd/csrc/me_fullpel.hip), so every case here makes the reference's "first minimum in raster order" depend on
where inside a unit, in which unit, row, wave, tile or strip the minimum lies.  Kernel = oracle everywhere, plus the planted winner stated in closed form."""
import numpy as np
import pytest

import me_common as mc

pytestmark = pytest.mark.gpu

PAD = mc.synth.PAD
WAVES = (1, 2, 4)


def pu_rect(pu):
    """(x, y, size) of an 8x8 (21..84) or 16x16 (5..20) PU inside the superblock: z-order of the 16x16 blocks, raster inside one"""
    z = (pu - 21) >> 2 if pu >= 21 else pu - 5
    X, Y = ((z >> 2) & 1) * 2 + (z & 1), (z >> 3) * 2 + ((z >> 1) & 1)
    if pu < 21:
        return 16 * X, 16 * Y, 16
    q = (pu - 21) & 3
    return 8 * (2 * X + (q & 1)), 8 * (2 * Y + (q >> 1)), 8


def noise_planes(w, h, seed):
    """full-range noise: no accidental ties, every unplanted SAD far above a planted one"""
    rng = np.random.default_rng(seed)
    cur = rng.integers(0, 256, (h, w), dtype=np.uint8)
    refp = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return mc.synth.pad_plane(cur), mc.synth.pad_plane(refp)


def one_window(orc, w, h, sb_index, window):
    allw = mc.windows(orc, w, h, window[0], window[1])
    d = allw[sb_index]
    assert (d.width, d.height) == tuple(window)        # the clamp left the whole window
    return (mc.OrcSbSearch * 1)(d)


def plant_period(cur_p, ref_p, d, pu, cy, cxa, cxb, rng):
    """Candidates (cxa, cy) and (cxb, cy) of `pu` tie and nothing between them does: the reference rows of the block are given the horizontal period
    cxb - cxa over exactly the columns those two candidates read, and the source block is made the block at candidate cxa with one sample changed by 1."""
    ox, oy, n = pu_rect(pu)
    p = cxb - cxa
    pat = rng.integers(0, 256, (n, p), dtype=np.uint8)
    row = np.tile(pat, (1, (n + p + p - 1) // p + 1))[:, :n + p]
    y0, x0 = PAD + d.sb_y + d.y_origin + cy + oy, PAD + d.sb_x + d.x_origin + cxa + ox
    ref_p[y0:y0 + n, x0:x0 + n + p] = row
    blk = row[:, :n].copy()
    blk[0, 0] ^= 1
    cur_p[PAD + d.sb_y + oy:PAD + d.sb_y + oy + n, PAD + d.sb_x + ox:PAD + d.sb_x + ox + n] = blk


def plant_copies(cur_p, ref_p, d, pu, cands):
    """every candidate of `cands` reads the source block with one sample changed by 1 (the blocks the candidates read must not overlap)"""
    ox, oy, n = pu_rect(pu)
    ys, xs = PAD + d.sb_y + oy, PAD + d.sb_x + ox
    blk = cur_p[ys:ys + n, xs:xs + n].copy()
    for cx, cy in cands:
        ref_p[ys + d.y_origin + cy:ys + d.y_origin + cy + n, xs + d.x_origin + cx:xs + d.x_origin + cx + n] = blk
    cur_p[ys, xs] ^= 1


def check(hip, orc, cur_p, ref_p, sbs, sub, expect, waves=WAVES):
    """expect: {pu: (cx, cy)} of record 0, the planted first minimum (SAD 1, SUB: 2)"""
    stride = cur_p.shape[1]
    o_sad, o_mv = mc.oracle_frame(orc, cur_p, ref_p, stride, PAD, sbs, sub)
    d = sbs[0]
    for pu, (cx, cy) in expect.items():     # the construction itself, against the oracle
        assert o_sad[0, pu] == (2 if sub else 1) and o_mv[0, pu] == mc.mv_word(d.x_origin + cx, d.y_origin + cy), (pu, hex(o_mv[0, pu]))
    try:
        for wv in waves:
            hip.check(hip.L.svt_hip_me_set_waves_per_sb(hip.h, wv))
            g_sad, g_mv = mc.hip_frame(hip, cur_p, ref_p, stride, PAD, sbs, sub)
            assert np.array_equal(g_sad, o_sad), (wv, [(i, pu, hex(g_sad[i, pu]), hex(o_sad[i, pu])) for i, pu in np.argwhere(g_sad != o_sad)[:6]])
            assert np.array_equal(g_mv, o_mv), (wv, [(i, pu, hex(g_mv[i, pu]), hex(o_mv[i, pu])) for i, pu in np.argwhere(g_mv != o_mv)[:6]])
    finally:
        hip.check(hip.L.svt_hip_me_set_waves_per_sb(hip.h, 4))      # the context's default
    return o_sad, o_mv


@pytest.mark.parametrize("sub", [0, 1])
def test_flat_content_first_candidate_wins(hip, orc, sub):
    """One superblock, flat source and reference, window 64 x 64: every SAD ties, candidate 0 must win for all 85 PUs."""
    w = h = 192
    cur_p = np.full((h + 2 * PAD, w + 2 * PAD), 77, np.uint8)
    ref_p = np.full_like(cur_p, 80)
    sbs = one_window(orc, w, h, 4, (64, 64))
    _, o_mv = check(hip, orc, cur_p, ref_p, sbs, sub, {})
    assert (o_mv[0] == mc.mv_word(sbs[0].x_origin, sbs[0].y_origin)).all()


@pytest.mark.parametrize("sub", [0, 1])
def test_ties_inside_one_unit(hip, orc, sub):
    """The minimum at positions 3 and 6 of the same unit (reference rows of horizontal period 3): position 3 must win.  Two 8x8 and two 16x16 PUs, in
    units of different rows and columns; also positions 0 and 7 (the unit's ends)."""
    w = h = 192
    cur_p, ref_p = noise_planes(w, h, 41)
    sbs = one_window(orc, w, h, 4, (64, 64))
    d, rng = sbs[0], np.random.default_rng(42)
    plant_period(cur_p, ref_p, d, 21, 5, 8 * 2 + 3, 8 * 2 + 6, rng)      # 8x8 PU (0, 0)
    plant_period(cur_p, ref_p, d, 84, 40, 8 * 7 + 3, 8 * 7 + 6, rng)     # 8x8 PU (56, 56), last unit of its row
    plant_period(cur_p, ref_p, d, 47, 63, 8 * 4 + 0, 8 * 4 + 7, rng)     # 8x8 PU, last candidate row, both ends of a unit
    plant_period(cur_p, ref_p, d, 8, 17, 3, 6, rng)                      # 16x16 PU (16, 16), first unit of its row
    plant_period(cur_p, ref_p, d, 17, 33, 8 * 5 + 3, 8 * 5 + 6, rng)     # 16x16 PU (32, 32)
    check(hip, orc, cur_p, ref_p, sbs, sub, {21: (19, 5), 84: (59, 40), 47: (32, 63), 8: (3, 17), 17: (43, 33)})


@pytest.mark.parametrize("sub", [0, 1])
def test_ties_across_units(hip, orc, sub):
    """The minimum at the last position of one unit and the first of the next (period 1), in two candidate rows, and in units that different waves own (at 4 / 2
    waves a wave takes 8 / 16 candidate rows of this window in turn), and in two units of the same lane (256 units apart)."""
    w = h = 192
    cur_p, ref_p = noise_planes(w, h, 43)
    sbs = one_window(orc, w, h, 4, (64, 64))
    d, rng = sbs[0], np.random.default_rng(44)
    plant_period(cur_p, ref_p, d, 21, 9, 8 * 3 + 7, 8 * 4, rng)           # 8x8 PU (0, 0): units 3 | 4 of candidate row 9
    plant_period(cur_p, ref_p, d, 20, 2, 8 * 6 + 7, 8 * 7, rng)           # 16x16 PU (48, 48): units 6 | 7 of candidate row 2
    plant_copies(cur_p, ref_p, d, 33, [(60, 10), (1, 11)])                # 8x8: end of row 10 | start of row 11
    plant_copies(cur_p, ref_p, d, 10, [(40, 31), (4, 32)])                # 16x16 PU (48, 0): rows 31 | 32 = waves 3 | 0 (4 waves), 1 | 0 (2 waves)
    plant_copies(cur_p, ref_p, d, 60, [(20, 3), (44, 12), (20, 35)])      # 8x8: waves 0 | 1 | the first's lane again (unit + 256)
    plant_copies(cur_p, ref_p, d, 13, [(50, 23), (3, 55)])                # 16x16 PU (0, 32): far apart, the later candidate in a smaller column
    check(hip, orc, cur_p, ref_p, sbs, sub, {21: (31, 9), 20: (55, 2), 33: (60, 10), 10: (40, 31), 60: (20, 3), 13: (50, 23)})


@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("window", [(8, 1), (72, 40), (136, 70)])
def test_window_sizes(hip, orc, sub, window):
    """8 x 1: a single unit.  72 x 40: two tiles, the second 8 wide -- the winner lies in the first tile, whose window is no longer staged when it is located,
    and ties with a candidate of the second tile in the same row.  136 x 70: 3 x 2 tiles, ragged in both directions."""
    w = h = 320
    cur_p, ref_p = noise_planes(w, h, 45 + window[0])
    sbs = one_window(orc, w, h, 12, window)
    d, rng = sbs[0], np.random.default_rng(46)
    if window == (8, 1):
        plant_period(cur_p, ref_p, d, 21, 0, 3, 6, rng)
        plant_period(cur_p, ref_p, d, 20, 0, 3, 6, rng)
        expect = {21: (3, 0), 20: (3, 0)}
    elif window == (72, 40):
        plant_copies(cur_p, ref_p, d, 21, [(5, 2), (66, 2)])
        plant_copies(cur_p, ref_p, d, 20, [(13, 39), (71, 39)])
        plant_period(cur_p, ref_p, d, 80, 20, 64 + 3, 64 + 6, rng)       # inside the narrow tile
        expect = {21: (5, 2), 20: (13, 39), 80: (67, 20)}
    else:
        plant_copies(cur_p, ref_p, d, 21, [(70, 65), (130, 65), (2, 66)])
        plant_copies(cur_p, ref_p, d, 20, [(135, 63), (0, 64)])          # last candidate of the first tile row | first of the second
        plant_period(cur_p, ref_p, d, 80, 69, 128 + 3, 128 + 6, rng)
        expect = {21: (70, 65), 20: (135, 63), 80: (131, 69)}
    check(hip, orc, cur_p, ref_p, sbs, sub, expect)


@pytest.mark.parametrize("sub", [0, 1])
def test_strip_boundary_tie(hip, orc, sub):
    """264 x 256 = 67 584 candidates: the strip-walking instance, strips of 248 and 8 candidate rows.  Exact ties between the last row of the first strip and
    the first of the second (the earlier strip must win), ties inside a unit in either strip, and a winner in the second strip alone."""
    w = h = 448
    cur_p, ref_p = noise_planes(w, h, 47)
    sbs = one_window(orc, w, h, 3 * 7 + 3, (264, 256))
    d, rng = sbs[0], np.random.default_rng(48)
    assert d.width * d.height > 65536 and 65536 // d.width == 248
    plant_copies(cur_p, ref_p, d, 21, [(100, 247), (10, 248)])
    plant_copies(cur_p, ref_p, d, 20, [(200, 247), (40, 248), (41, 255)])
    plant_period(cur_p, ref_p, d, 80, 100, 8 * 20 + 3, 8 * 20 + 6, rng)
    plant_period(cur_p, ref_p, d, 8, 250, 8 * 9 + 3, 8 * 9 + 6, rng)
    plant_copies(cur_p, ref_p, d, 50, [(263, 255)])
    check(hip, orc, cur_p, ref_p, sbs, sub, {21: (100, 247), 20: (200, 247), 80: (163, 100), 8: (75, 250), 50: (263, 255)}, waves=(4,))


@pytest.mark.parametrize("sub", [0, 1])
def test_corner_superblocks_clamped_windows(hip, orc, sub):
    """2 x 2 superblocks = the whole picture, search centres pushed outwards: every window is clamped at a picture corner and the located units lie on
    the window's outermost rows and columns, so the locate step's global reads run along the edge of the padded plane.  Flat bands make ties common."""
    w = h = 128
    cur, refp = mc.synth.make_luma_pair(w, h, seed=49)
    cur[40:100, 30:120] = 90
    refp[:, :50] = 90
    refp[90:, :] = 90
    cur_p, ref_p = mc.synth.pad_plane(cur), mc.synth.pad_plane(refp)
    centers = [(-90, -90), (90, -90), (-90, 90), (90, 90)]
    for sa in ((64, 64), (136, 70)):
        sbs = mc.windows(orc, w, h, sa[0], sa[1], centers)
        assert any((s.width, s.height) != sa for s in sbs)
        # the best candidate of a superblock's outermost PUs at the window's far corner: the block the last candidate reads
        for s, (ox, oy) in zip(sbs, ((0, 0), (56, 0), (0, 56), (56, 56))):
            if s.width >= 8:
                ys, xs = PAD + s.sb_y + oy, PAD + s.sb_x + ox
                cx, cy = s.x_origin + s.width - 1, s.y_origin + s.height - 1
                ref_p[ys + cy:ys + cy + 8, xs + cx:xs + cx + 8] = cur_p[ys:ys + 8, xs:xs + 8]
        check(hip, orc, cur_p, ref_p, sbs, sub, {})
