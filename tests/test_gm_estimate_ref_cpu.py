"""CPU, reference only: the picture pairs of tests/gm_estimate_common.py take the branches of compute_global_motion their names promise, so that the device test
of the picture call covers each of them."""
import gm_estimate_common as ec


def test_rotzoom_accepted(ref):
    for n in ("rot_96x80", "rot_352x288"):
        w = ec.reference(ref, n)
        assert w["wmtype"] == 2 and w["records"][0]["wmtype"] == 2 and w["wmmat"] == w["records"][0]["wmmat"]


def test_identical_planes(ref):
    w = ec.reference(ref, "identical_96x80")
    assert w["ref_frame_error"] == 0 and w["wmtype"] == 0 and w["records"][0]["num_inliers_kept"] > 100 and w["records"][0]["fit_wmtype"] == 0


def test_unrelated_noise_and_flat(ref):
    for n in ("noise_96x80", "noise_352x288", "flat_96x80"):
        w = ec.reference(ref, n)
        assert w["wmtype"] == 0 and all(r["num_inliers_kept"] == 0 for r in w["records"]), n
    assert ec.reference(ref, "noise_352x288")["ref_frame_error"] > 0 and ec.reference(ref, "flat_96x80")["ref_frame_error"] == 0


def test_translation_result(ref):
    w = ec.reference(ref, "shifted_96x80")
    assert w["wmtype"] == 1 and w["wmmat"][:2] == [3 * ec.ONE, -2 * ec.ONE]


def test_sheared_pairs_reject_rotzoom_and_accept_affine(ref):
    for n in ("shear_96x80", "shear_352x288"):
        w = ec.reference(ref, n)
        assert w["records"][0]["wmtype"] == 2 and w["wmtype"] == 3 and w["wmmat"] == w["records"][1]["wmmat"], n
        assert ec.reference(ref, n, rotzoom_model_only=1)["wmtype"] == 0
    w = ec.reference(ref, "squeeze_352x288")   # here the MIN_INLIER_PROB rule drops the ROTZOOM motion before any refinement
    assert w["records"][0]["num_inliers_kept"] == 0 and w["records"][0]["fit_wmtype"] == 2 and w["wmtype"] == 3
