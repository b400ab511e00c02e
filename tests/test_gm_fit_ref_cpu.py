"""CPU, reference only: the named correspondence lists of tests/gm_fit_common.py deserve their names, so that no test of the device's model fit passes vacuously.
Every figure below is the reference's own result on these lists."""
import gm_fit_common as fc

T, R, A = fc.TRANSLATION, fc.ROTZOOM, fc.AFFINE


def test_fourteen_points_are_refused(ref):
    for name in ("rz_14", "af_14"):
        for t in fc.TYPES:
            r = fc.ref_fit(ref, name, t)
            assert (r["ret"], r["num_inliers"], r["params"]) == (1, 0, fc.bits(fc.IDENTITY_PARAMS))


def test_rotzoom_lists_keep_most_points(ref):
    assert [fc.ref_fit(ref, n, R)["num_inliers"] for n in ("rz_300", "rz_2500", "rz_4096")] == [223, 1643, 3224]
    assert [fc.ref_fit(ref, n, A)["num_inliers"] for n in ("af_300", "af_2500", "af_4096")] == [197, 1759, 2064]
    assert fc.ref_fit(ref, "tr_300", T)["num_inliers"] == 223
    assert fc.ref_fit(ref, "rz_4096", R)["npoints"] == 4096


def test_degenerate_lists(ref):
    c = [fc.ref_fit(ref, "collinear_100", t) for t in fc.TYPES]
    assert [(r["ret"], r["num_inliers"]) for r in c] == [(0, 0), (1, 0), (1, 0)]
    assert all(fc.ref_fit(ref, "single_100", t)["ret"] == 1 for t in fc.TYPES)
    assert all(fc.ref_fit(ref, n, t)["ret"] == 1 for n in ("empty", "count_negative") for t in fc.TYPES)
    two = fc.lists()["two_rows"]["corr"]
    assert set(two[:120, 1]) == {140, 141} and fc.ref_fit(ref, "two_rows", R)["num_inliers"] == 120


def test_all_outliers(ref):
    t, r, a = (fc.ref_fit(ref, "outliers_300", k) for k in fc.TYPES)
    assert (t["ret"], t["num_inliers"], r["ret"], r["num_inliers"]) == (0, 0, 0, 0)
    assert (a["ret"], a["num_inliers"], a["num_inliers_kept"]) == (0, 3, 0)          # three points fit their own affine model exactly; the rule drops it
    assert max(abs(v - w) for v, w in zip(a["params_f"], fc.IDENTITY_PARAMS)) > 100   # far from identity, inside what the conversion defines
    assert max(abs(v) for v in a["params_f"]) * 65536 < 2 ** 31


def test_a_motion_of_fewer_than_three_inliers_keeps_identity_parameters(ref):
    r = fc.ref_fit(ref, "rz_15", T)
    assert (r["ret"], r["num_inliers"], r["num_inliers_kept"], r["params"], r["wmtype"]) == (0, 2, 2, fc.bits(fc.IDENTITY_PARAMS), 0)


def test_identity_list_gives_minus_zero_and_an_identity_model(ref):
    r = fc.ref_fit(ref, "identity_100", R)
    assert r["num_inliers"] == 100 and r["wmtype"] == 0 and r["num_inliers_kept"] == 100
    assert r["params"][4] == fc.bits([-0.0])[0] != fc.bits([0.0])[0] and r["params"][3] == fc.bits([0.0])[0]


def test_the_rule_drops_motions_and_counts_are_clamped(ref):
    assert [(fc.ref_fit(ref, n, T)["num_inliers"], fc.ref_fit(ref, n, T)["num_inliers_kept"]) for n in ("rz_300", "rz_4096")] == [(13, 0), (179, 0)]
    ls = fc.lists()
    assert (ls["count_over_capacity"]["count"], ls["count_over_capacity"]["n"], ls["count_negative"]["n"]) == (1000, 64, 0)
    assert ls["small_capacity"]["capacity"] == 200 and ls["small_capacity"]["n"] == 150
    assert fc.ref_fit(ref, "count_over_capacity", R)["num_inliers"] == 52


def test_two_thirds_of_the_runs_recompute_a_model(ref):
    recomputed = sum(fc.ref_fit(ref, n, t)["num_inliers"] >= 3 for n, t in fc.CASES)
    assert 3 * recomputed >= 2 * len(fc.CASES), (recomputed, len(fc.CASES))
    # every parameter stays inside what the conversion to integers defines
    assert max(abs(v) for n, t in fc.CASES for v in fc.ref_fit(ref, n, t)["params_f"]) * 65536 < 2 ** 31
