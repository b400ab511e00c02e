"""CPU, reference only: the inputs of tests/test_gm_front_gpu.py deserve their names, so that the GPU tests cannot pass vacuously.  The pictures have the corners
the tests rely on (many, more than the truncation keeps, score 254, neighbours that remove each other, none); the closed form of the FAST-9 score the kernel uses
equals svt_aom_fast9_detect + svt_aom_fast9_score; the correspondence cases give correspondences where they should and none where they should not, resolve exact
ties by index and move points in both passes of improve_correspondence; the correlation inputs contain NaNs and exact ties."""
import numpy as np
import pytest

import gm_front_common as f

PICTURES = f.corner_pictures()


@pytest.mark.parametrize("name", list(PICTURES))
def test_closed_form_score_equals_the_reference(ref, name):
    a = PICTURES[name]
    xy, sc = f.ref_raw_corners(ref, a)
    cf = f.closed_form_scores(a)
    ys, xs = np.nonzero(cf)          # raster order, like the reference's list
    assert np.array_equal(np.stack([xs, ys], 1).astype(np.int32).reshape(-1, 2), xy)
    assert np.array_equal(cf[ys, xs], sc)


def test_pictures_have_the_corners_the_tests_rely_on(ref):
    raw = {n: f.ref_raw_corners(ref, a) for n, a in PICTURES.items()}
    kept = {n: f.ref_kept(ref, a) for n, a in PICTURES.items()}
    for n in ("tex_96x80", "tex_100x76_p1", "noise_90x50"):
        assert kept[n] >= 100 and len(raw[n][0]) > 2 * kept[n], n           # the suppression removes most
    assert kept["noise_352x288"] > 2 * f.MAX_CORNERS and len(f.ref_corners(ref, PICTURES["noise_352x288"])) == f.MAX_CORNERS
    for n in ("spikes", "spikes_inverse", "tiny_8x8_spike"):
        assert raw[n][1].max() == 254 and kept[n] == len(raw[n][0]) >= 1, n  # the largest score there is; isolated corners all stay
    pts = f.ref_corners(ref, PICTURES["spikes"])
    assert [3, 3] in pts.tolist() and [40 - 4, 31 - 4] in pts.tolist()      # the first and last pixel that can be a corner
    xy, sc = raw["blocks"]
    assert len(xy) == 7 and set(sc.tolist()) == {199} and kept["blocks"] == 0   # equal neighbours remove each other
    assert len(raw["flat"][0]) == 0 and kept["flat"] == 0
    assert len(raw["tiny_8x8"][0]) >= 1 and all(3 <= v <= 4 for v in raw["tiny_8x8"][0].ravel())


def test_truncation_keeps_the_top_rows(ref):
    a = PICTURES["noise_352x288"]
    full = f.ref_corners(ref, a, a.size)
    for m in (1, 100, f.MAX_CORNERS):
        assert np.array_equal(f.ref_corners(ref, a, m), full[:m])
    assert full[f.MAX_CORNERS - 1][1] < a.shape[0] // 2


@pytest.mark.parametrize("name", f.CASES)
def test_correspondence_cases(ref, name):
    s, r, sp, rp = f.case(ref, name)
    out = f.case_reference(ref, name)
    assert len(out) <= len(sp)
    if name in ("shifted_96x80", "rot_96x80", "rot_352x288", "identical", "same_corner_twice", "periodic_ties", "periodic_ties_raster"):
        assert len(sp) >= 100 and len(rp) >= 100 and len(out) >= 50
    if name in ("nothing_near", "flat_pair", "flat_reference", "empty_source", "empty_reference", "empty_both"):
        assert len(out) == 0
    if name in ("borders", "random_points"):
        assert 0 < len(out) < len(sp)
    if name == "shifted_96x80":
        assert (np.abs((out[:, 2:] - out[:, :2]) - np.array([3, -2])).max(1) == 0).sum() >= 50   # the shift is found
    if name == "identical":
        assert np.array_equal(out[:, :2], out[:, 2:])
    if name == "nothing_near":
        assert len(sp) >= 50 and len(rp) >= 50
    if name == "borders":
        h, w = s.shape
        for pts in (sp, rp):
            x, y = pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64)
            assert (x < 0).any() and (y < 0).any() and (x >= w).any() and (y >= h).any()
            for v, n in ((x, w), (y, h)):
                assert {5, 6, n - 7, n - 6} <= set(v.tolist())


def test_several_candidates_per_corner_at_352x288(ref):
    s, r, sp, rp = f.case(ref, "rot_352x288")
    assert max(s.shape) >> 4 == 22 and max(f.case(ref, "rot_96x80")[0].shape) >> 4 == 6
    d2 = ((sp[:200, None, :].astype(np.int64) - rp[None, :, :]) ** 2).sum(2)
    assert np.median((d2 <= 22 * 22).sum(1)) >= 3


def test_improve_correspondence_moves_points_in_both_passes(ref):
    """a reference point that is no reference corner was moved by the first pass, a source point that is no source corner by the second"""
    for name in ("rot_96x80", "rot_352x288"):
        s, r, sp, rp = f.case(ref, name)
        out = f.case_reference(ref, name).tolist()
        sset, rset = {tuple(p) for p in sp.tolist()}, {tuple(p) for p in rp.tolist()}
        assert sum(tuple(o[2:]) not in rset for o in out) >= 1 and sum(tuple(o[:2]) not in sset for o in out) >= 1


def test_exact_ties_are_won_by_the_lowest_index(ref):
    """patches a period apart are identical, so their correlations tie bit for bit and the order of the reference list alone decides the winner: the same points
    in the opposite order give other correspondences, and in either order the match is often not the identical point"""
    a, b = f.case_reference(ref, "periodic_ties"), f.case_reference(ref, "periodic_ties_raster")
    assert len(a) == len(b) >= 50 and np.array_equal(a[:, :2], b[:, :2])
    assert (a[:, 2:] != b[:, 2:]).any(1).sum() >= 20
    for out in (a, b):
        d = out[:, 2:] - out[:, :2]
        assert (d != 0).any(1).sum() >= 20 and set(np.unique(d).tolist()) <= {-8, 0, 8}
    s, r, sp, rp = f.case(ref, "same_corner_twice")
    assert rp[0].tolist() == rp[41].tolist() and rp[-1].tolist() == rp[6].tolist()


def test_correlation_inputs_contain_nans_and_ties(ref):
    v = {n: f.correlation_reference(ref, n) for n in f.correlation_inputs()}
    assert len(v["texture"]) >= 20000 and not np.isnan(v["texture"]).any() and (v["texture"] > 0).any() and (v["texture"] < 0).any()
    assert 50 <= np.isnan(v["flat_second"]).sum() <= len(v["flat_second"]) - 50
    assert np.isnan(v["zero_against_255"]).all() and np.isnan(v["against_255_zero"]).all()
    # a checker against itself: 84 or 85 of the 169 samples are 255, either way the largest variance there is, 255^2 * 84 * 85 (x 169); cov = +-var
    var = 255 * 255 * 84 * 85
    assert set(v["checker"].tolist()) == {var / np.sqrt(float(var)), -var / np.sqrt(float(var))}
    assert len(set(v["periodic"].view(np.uint64).tolist())) == 1 and v["periodic"][0] > 0   # twelve different pairs, one bit pattern
