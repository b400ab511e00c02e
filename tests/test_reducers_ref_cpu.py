"""CPU side of the saturated / full-scale pins of the pixel reducers (block SSE lists, plane SSE, block SAD / variance, the 85-PU integer search, the 16-bit
windowed search): the oracle equals every closed form the GPU tests assert, on exactly the inputs they build (the same helper functions of dlf_common /
me_common), and the inputs contain what the GPU tests say they cover.  Needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import dlf_common as dc
import me_common as mc


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_block_sse_lists(bd):
    c = dc.sse_case(bd)          # asserts oracle == numpy on every list and that every pair lies inside the planes
    T = dc.SSE_LIST_THRESHOLD
    assert int(c["a"].max()) == int(c["b"].max()) == c["max"] == (1 << bd) - 1
    # the small-block list: just above the threshold, a last workgroup of three pairs, every width x height present
    small = c["small"]
    assert len(small) == T + 3 and len(small) % 4 == 3 and len(small[:T]) <= T < len(small[:T + 1])
    assert {(p[4], p[5]) for p in small} == {(w, h) for w in dc.SSE_SMALL_W for h in dc.SSE_SMALL_H}
    assert all(int(v) > 0 for v in c["exp_small"][-3:])            # a dropped last workgroup cannot pass as zeros
    # the rectangles: rows form alone, list form when embedded
    rects, exp = c["rects"], c["exp_rects"]
    assert len(rects) <= T and len(c["long"]) > T and len(c["long"]) % 4 != 0
    assert c["long"][c["rects_at"]:c["rects_at"] + len(rects)] == rects
    assert {(p[4], p[5]) for p in rects} >= {(384, 392), (320, 257), (70, 300), (1, 300), (65, 33), (384, 41)}
    assert sum(p[5] > 256 for p in rects) >= 4 and sum(p[4] > 64 for p in rects) >= 4 and any(p[5] % 8 for p in rects)
    assert any(p[0] % 2 for p in rects) and any(p[2] % 2 for p in rects)                       # odd columns on either side
    assert len({(p[0], p[1]) for p in rects}) == len(rects) and c["a"].shape[1] != c["b"].shape[1]
    assert max(p[4] * p[5] for p in rects) >= 150000
    assert int((exp == 0).sum()) == 1 and int(exp[rects.index(dc.SSE_RECT_IDENTICAL)]) == 0     # exactly one pair reads 0
    sat = 384 * 392 * c["max"] ** 2
    assert sat > 1 << 32 and int(exp[rects.index(dc.SSE_RECT_SATURATED)]) == sat
    assert int((exp > 1 << 32).sum()) >= 1
    # a second trip of the rows form matters: rows 256.. of the tall rectangles carry part of the sum
    for p, e in zip(rects, exp):
        if p[5] > 256 and p != dc.SSE_RECT_IDENTICAL:
            assert int(dc.numpy_sse(c["a"], c["b"], [p[:5] + (256,)])[0]) < int(e)


def test_plane_sse_and_block_variance_closed_forms():
    orc = dc.oracle()
    orc.orc_plane_sse.restype = C.c_uint64
    for mx in (255, 1023, 4095):
        for (w, h) in dc.PLANE_SSE_SATURATED_SIZES:
            a, b, closed = dc.saturated_planes(mx, w, h)
            got = orc.orc_plane_sse(a.itemsize, C.c_void_p(a.ctypes.data + (2 * a.shape[1] + 3) * a.itemsize), a.shape[1],
                                    C.c_void_p(b.ctypes.data + (1 * b.shape[1] + 5) * b.itemsize), b.shape[1], w, h)
            assert got == closed == w * h * mx * mx
    assert 8 * 4 * 1023 ** 2 > 1 << 24 and 8 * 4 * 4095 ** 2 < 1 << 32     # what a lane of plane_sse_kernel holds: above 24 bits, inside its u32
    assert dc.PLANE_SSE_SATURATED_SIZES[1][0] > 1024 and all(h % 8 for _, h in dc.PLANE_SSE_SATURATED_SIZES)
    orc.orc_nxm_sad.restype = C.c_uint32; orc.orc_sad_16b.restype = C.c_uint32
    orc.orc_variance.restype = C.c_uint32; orc.orc_variance_hbd10.restype = C.c_uint32
    for bd in (8, 10):
        ra, rb, (ax, ay, bx, by, w, h), closed = dc.saturated_block_pair(bd)
        a = np.zeros((256, 320), np.uint8 if bd == 8 else np.uint16); b = np.ones((256, 352), a.dtype)
        a[ra] = (1 << bd) - 1; b[rb] = 0
        assert (a[ay:ay + h, ax:ax + w] == (1 << bd) - 1).all() and (b[by:by + h, bx:bx + w] == 0).all() and (w, h) == (128, 128)
        pa = C.c_void_p(a.ctypes.data + (ay * 320 + ax) * a.itemsize); pb = C.c_void_p(b.ctypes.data + (by * 352 + bx) * b.itemsize)
        s = C.c_uint32(0)
        if bd == 8:
            got = (orc.orc_nxm_sad(pa, 320, pb, 352, h, w), orc.orc_variance(pa, 320, pb, 352, w, h, C.byref(s)), None)
        else:
            got = (orc.orc_sad_16b(pa, 320, pb, 352, h, w), orc.orc_variance_hbd10(pa, 320, pb, 352, w, h, C.byref(s)), None)
        assert (got[0], got[1], s.value) == closed
    assert dc.saturated_block_pair(8)[3] == (255 * 16384, 0, 255 ** 2 * 16384) and dc.saturated_block_pair(10)[3] == (1023 * 16384, 0, (1023 ** 2 * 16384 + 8) >> 4)


@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("window,strip", [(w, False) for w in mc.SATURATED_WINDOWS] + [(mc.SATURATED_STRIP_WINDOW, True)])
def test_me_saturated_closed_forms(orc, window, strip, sub):
    assert (window[0] * window[1] > 65536) == strip
    for pol in (0, 1):
        for variant in range(3):
            cur_p, ref_p, stride, sbs, (c_sad, c_mv), closed_for = mc.saturated_case(orc, window, variant, pol, sub, strip)
            lo, hi = (0, 255) if pol == 0 else (255, 0)
            assert (cur_p == lo).all() and int((ref_p != hi).sum()) == (0, 4096, 1)[variant]
            o_sad, o_mv = mc.saturated_oracle(orc, window, variant, pol, sub, strip)
            d = sbs[0]
            last = mc.mv_word(d.x_origin + d.width - 1, d.y_origin + d.height - 1)
            for i in closed_for:
                assert np.array_equal(o_sad[i], c_sad[i]) and np.array_equal(o_mv[i], c_mv[i]), (pol, variant, i)
            if variant == 0:
                assert closed_for == list(range(len(sbs))) and int(o_sad[0, 5]) == 0xFF00 and (o_sad == 255 * mc.PU_AREA).all()
                assert all((o_mv[i] == mc.mv_word(sbs[i].x_origin, sbs[i].y_origin)).all() for i in range(len(sbs)))
            elif variant == 1:
                assert o_sad[0, 0] == 0 and o_mv[0, 0] == last and (o_sad[0] < 255 * mc.PU_AREA).all()
            else:
                short = 2 if sub else 1
                assert closed_for == [0] and [int(o_sad[0, pu]) for pu in mc.PU_LAST] == [255 * (a - short) for a in (4096, 1024, 256, 64)]
                others = [pu for pu in range(85) if pu not in mc.PU_LAST]
                assert (o_mv[0, mc.PU_LAST] == last).all() and (o_mv[0, others] == mc.mv_word(d.x_origin, d.y_origin)).all()


@pytest.mark.parametrize("mx", [1023, 4095])
def test_hbd_windowed_search_closed_forms(orc, mx):
    assert all(mc.sad16_takes_lds_form(*s[:5]) for s in mc.SAD16_LDS_SHAPES) and not any(mc.sad16_takes_lds_form(*s[:5]) for s in mc.SAD16_GENERIC_SHAPES)
    assert {s[:2] for s in mc.SAD16_LDS_SHAPES} == {(16, 16), (32, 32), (48, 17), (64, 64)} and {s[2:4] for s in mc.SAD16_LDS_SHAPES} == {(8, 1), (64, 64), (24, 40)}
    assert {s[5] for s in mc.SAD16_LDS_SHAPES} == {0, 1} and mc.SAD16_SW % 2 == 0
    g = mc.SAD16_GENERIC_SHAPES
    assert any(s[4] == 2 for s in g) and {9, 5} <= {s[2] for s in g} and any(s[:2] == (8, 8) for s in g) and (64, 64, 72, 8, 1, 0) in g
    for pol in (0, 1):
        src, ref, S, closed = mc.saturated_sad16(mx, pol)
        assert all((j.src_x & 1) == s[5] for j, s in zip(S, [s for s in mc.SAD16_SHAPES for _ in range(3)]))
        e_sad, e_xy = mc.oracle_sad16(orc, src, ref, S)
        assert e_sad.tolist() == [c[0] for c in closed] and e_xy.tolist() == [[c[1], c[2]] for c in closed], pol
        at = {s: 3 * i for i, s in enumerate(mc.SAD16_SHAPES)}
        full = {1023: 0x3ff000, 4095: 0xfff000}[mx]
        assert e_sad[at[(64, 64, 64, 64, 1, 0)]] == full and e_sad[at[(64, 64, 16, 16, 2, 0)]] == {1023: 0x1ff800, 4095: 0x7ff800}[mx]
        assert e_sad[at[(16, 16, 64, 64, 1, 0)]] == {1023: 0x3ff00, 4095: 0xfff00}[mx] and int(e_sad.max()) == full < 0xffffff
        assert e_sad[at[(64, 64, 64, 64, 1, 1)] + 2] == full - mx
