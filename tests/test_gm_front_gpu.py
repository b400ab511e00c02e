"""GPU, bit for bit: FAST-9 corners, the 13x13 cross-correlation and the correspondence search of the global-motion front half against the reference's own exported
functions (svt_av1_fast_corner_detect, svt_av1_compute_cross_correlation_c, svt_av1_determine_correspondence).  Every comparison is exact; no tolerance anywhere.
tests/test_gm_front_ref_cpu.py shows that the inputs exercise what their names say.  The references are computed once per process and shared."""
import numpy as np
import pytest

import gm_front_common as f
import test_gm_front_abi as abi

pytestmark = pytest.mark.gpu
PICTURES = f.corner_pictures()


def embedded(plane, fill, top=5, left=3, right=34, bottom=4):
    """the plane at an odd offset and stride inside a larger buffer filled with `fill`"""
    h, w = plane.shape
    big = np.full((h + top + bottom, w + left + right), fill, np.uint8)
    v = big[top:top + h, left:left + w]
    v[:] = plane
    return v


# ------------------------------------------------------------------------------------------------ corners
@pytest.mark.parametrize("name", list(PICTURES))
def test_corners_one_plane(hip, ref, name):
    a = PICTURES[name]
    pts, cnt, kept = hip.gm_corners_batch([a])
    want = f.ref_corners(ref, a)
    assert (int(cnt[0]), int(kept[0])) == (len(want), f.ref_kept(ref, a))
    assert np.array_equal(pts[0], want)


def test_corners_three_planes_of_two_sizes(hip, ref):
    planes = [PICTURES["tex_96x80"], PICTURES["noise_352x288"], PICTURES["noise_90x50"], PICTURES["tex_96x80"]]
    for sel in ([0, 1, 3], [1, 2, 0]):
        ps = [planes[i] for i in sel]
        pts, cnt, kept = hip.gm_corners_batch(ps)
        for a, p, c, k in zip(ps, pts, cnt, kept):
            want = f.ref_corners(ref, a)
            assert (int(c), int(k)) == (len(want), f.ref_kept(ref, a)) and np.array_equal(p, want)


def test_corners_nine_planes(hip, ref):
    ps = [f.tex(60 + i, 40 + 3 * i, 30 + 5 * (i % 4), passes=1) for i in range(9)]
    pts, cnt, _ = hip.gm_corners_batch(ps)
    assert sum(int(c) for c in cnt) >= 100
    for a, p in zip(ps, pts):
        assert np.array_equal(p, f.ref_corners(ref, a))


@pytest.mark.parametrize("max_points", [1, 100, 4096])
def test_corners_truncation_in_raster_order(hip, ref, max_points):
    a = PICTURES["noise_352x288"]
    pts, cnt, kept = hip.gm_corners_batch([a, PICTURES["spikes"]], max_points=max_points)
    assert int(kept[0]) == f.ref_kept(ref, a) > 2 * 4096 and int(cnt[0]) == max_points
    assert np.array_equal(pts[0], f.ref_corners(ref, a, max_points))
    assert np.array_equal(pts[1], f.ref_corners(ref, PICTURES["spikes"], max_points)) and int(kept[1]) == 13


def test_corners_embedded_plane_reads_nothing_outside(hip, ref):
    for name in ("tex_100x76_p1", "tiny_8x8"):
        a = PICTURES[name]
        want = f.ref_corners(ref, a)
        for fill in (0x00, 0xFF, 0x5A):
            pts, cnt, _ = hip.gm_corners_batch([embedded(a, fill), a])
            assert np.array_equal(pts[0], want) and np.array_equal(pts[1], want), (name, fill)


def test_corners_two_calls_back_to_back_reuse_nothing(hip, ref):
    """a second call on other pictures does not see the first call's scores"""
    hip.gm_corners_batch([PICTURES["noise_352x288"]])
    pts, cnt, kept = hip.gm_corners_batch([PICTURES["flat"], PICTURES["blocks"]])
    assert list(cnt) == [0, 0] and list(kept) == [0, 0]


# ------------------------------------------------------------------------------------------------ cross-correlation
@pytest.mark.parametrize("name", list(f.correlation_inputs()))
def test_cross_correlation_bit_patterns(hip, ref, name):
    a, b, pairs = f.correlation_inputs()[name]
    want = f.correlation_reference(ref, name)
    got = hip.gm_cross_correlation_batch(a, b, pairs)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64)), np.flatnonzero(got[ok].view(np.uint64) != want[ok].view(np.uint64))[:8]


def test_cross_correlation_strided_planes_and_no_pairs(hip, ref):
    a, b, pairs = f.correlation_inputs()["texture"]
    pairs = pairs[-500:]
    want = f.correlation_reference(ref, "texture")[-500:]
    for fill in (0x00, 0xFF):
        got = hip.gm_cross_correlation_batch(embedded(a, fill), embedded(b, 255 - fill, top=2, left=11, right=6), pairs)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert hip.gm_cross_correlation_batch(a, b, np.zeros((0, 4), np.int32)).shape == (0,)


def test_cross_correlation_pair_outside_gives_zero(hip):
    """the documented convention: a pair either of whose windows leaves the plane is not read and gets 0.0"""
    a, b, _ = f.correlation_inputs()["texture"]
    h, w = a.shape
    pairs = np.array([(5, 40, 40, 40), (40, 5, 40, 40), (40, 40, w - 6, 40), (40, 40, 40, h - 6), (-1, -1, 40, 40), (40, 40, 1 << 30, 40), (40, 40, 40, -(1 << 31))],
                     np.int64).astype(np.int32)
    got = hip.gm_cross_correlation_batch(embedded(a, 0xFF), embedded(b, 0xFF), pairs)
    assert np.array_equal(got.view(np.uint64), np.zeros(len(pairs), np.uint64))


# ------------------------------------------------------------------------------------------------ correspondences
@pytest.mark.parametrize("name", f.CASES)
def test_correspondences(hip, ref, name):
    s, r, sp, rp = f.case(ref, name)
    got = hip.gm_correspondences_batch(s, [r], sp, [rp])
    assert np.array_equal(got[0], f.case_reference(ref, name))


def test_correspondences_small_list_capacity(hip, ref):
    """max_points is the capacity of the lists, not 4096: layouts follow it"""
    s, r, sp, rp = f.case(ref, "rot_96x80")
    cap = max(len(sp), len(rp))
    got = hip.gm_correspondences_batch(s, [r, s], sp, [rp, sp], max_points=cap)
    assert np.array_equal(got[0], f.case_reference(ref, "rot_96x80")) and np.array_equal(got[1], f.ref_correspondences(ref, s, sp, s, sp))


def test_correspondences_two_references_of_different_strides(hip, ref):
    s, r1, sp, rp1 = f.case(ref, "shifted_96x80")
    r2 = f.tex(21, 96, 80, dx=2, dy=-1)
    rp2 = f.ref_corners(ref, r2)
    want = [f.case_reference(ref, "shifted_96x80"), f.ref_correspondences(ref, s, sp, r2, rp2)]
    assert len(want[1]) >= 50 and not np.array_equal(want[0], want[1])
    for fill in (0x00, 0xFF):
        got = hip.gm_correspondences_batch(embedded(s, fill, top=1, left=7, right=2), [embedded(r1, 255 - fill), embedded(r2, fill, top=9, left=1, right=50), r1], sp, [rp1, rp2, rp2])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[2], f.ref_correspondences(ref, s, sp, r1, rp2))


def test_correspondences_eight_references(hip, ref):
    s = f.tex(21, 96, 80)
    sp = f.ref_corners(ref, s)
    refs = [f.tex(21, 96, 80, dx=(i % 3) - 1, dy=(i // 3) - 1) for i in range(8)]
    rps = [f.ref_corners(ref, r) for r in refs]
    got = hip.gm_correspondences_batch(s, refs, sp, rps)
    for g_, r, rp in zip(got, refs, rps):
        assert np.array_equal(g_, f.ref_correspondences(ref, s, sp, r, rp))


# ------------------------------------------------------------------------------------------------ chain
@pytest.mark.parametrize("name", ["rot_96x80", "rot_352x288"])
def test_chain_corners_feed_correspondences_on_the_device(hip, ref, name):
    """the lists and counts never leave the device between the two calls"""
    s, r, sp, rp = f.case(ref, name)       # sp, rp: the reference's svt_av1_fast_corner_detect of the two planes
    got = hip.gm_correspondences_batch(s, [r, s])
    assert np.array_equal(got[0], f.case_reference(ref, name))
    assert np.array_equal(got[1], f.ref_correspondences(ref, s, sp, s, sp))


def test_chain_truncated_lists(hip, ref):
    s, r = f.noise(24, 352, 288), f.noise(26, 352, 288)
    sp, rp = f.ref_corners(ref, s, 300), f.ref_corners(ref, r, 300)
    got = hip.gm_correspondences_batch(s, [r, s], max_points=300)
    assert np.array_equal(got[0], f.ref_correspondences(ref, s, sp, r, rp))
    want_self = f.ref_correspondences(ref, s, sp, s, sp)
    assert len(want_self) >= 50 and np.array_equal(got[1], want_self)


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_with_a_live_context(hip, pkg):
    L = pkg.lib()
    d = hip.empty(1 << 16)
    try:
        for c in abi.CORNERS_BAD:
            assert abi.call_corners(pkg, L, hip.h, d.value, **c) == abi.BAD_ARG, c
        for c in abi.CORR_BAD:
            assert abi.call_correlation(L, hip.h, d.value, **c) == abi.BAD_ARG, c
        for c in abi.MATCH_BAD:
            assert abi.call_match(pkg, L, hip.h, d.value, **c) == abi.BAD_ARG, c
        assert b"bad argument" in L.svt_hip_last_error(hip.h)
    finally:
        hip.free(d)
