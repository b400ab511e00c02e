"""GPU: svt_hip_gm_estimate_picture_dev, compute_global_motion of a picture in one call, against the composition of the reference's functions in its order
(gm_fit_common.ref_estimate): the final model and every per-model record, for 1, 2 and 8 references of different strides, rotzoom_model_only on and off, twice on
one scratch, and against the three existing calls with the reference's RANSAC on the host between them."""
import ctypes as C

import numpy as np
import pytest

import gm_common as g
import gm_estimate_common as ec
import gm_fit_common as fc
import test_gm_fit_abi as abi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ec.SMALL + ec.LARGE)
def test_one_reference(hip, ref, name):
    s, r = ec.pair(name)
    out = hip.gm_estimate_picture(s, [r])
    assert not ec.same_estimate(out[0], ec.reference(ref, name))


@pytest.mark.parametrize("rz_only", [0, 1])
def test_eight_references_of_different_strides(hip, ref, rz_only):
    """one source (the texture of seed 21) against eight planes in one call: its shifted copy, itself, and the other pairs' pictures, which are unrelated to this
    source -- the reference decides what each gives; two of three planes sit in wider buffers of their own stride"""
    src = ec.pair("identical_96x80")[0]
    others = [ec.pair("shifted_96x80")[1], src, ec.pair("rot_96x80")[1], ec.pair("noise_96x80")[1], ec.pair("flat_96x80")[1], ec.pair("shear_96x80")[1],
              ec.pair("shifted_96x80")[1], ec.pair("rot_96x80")[0]]
    refs = [ec.strided(r, 5 + 4 * i, 7 * i) if i % 3 else r for i, r in enumerate(others)]
    out = hip.gm_estimate_picture(src, refs, rotzoom_model_only=rz_only, allow_high_precision_mv=rz_only)
    types = set()
    for i, r in enumerate(others):
        want = fc.ref_estimate(ref, src, np.ascontiguousarray(r), rz_only, rz_only)
        assert not ec.same_estimate(out[i], want), i
        types.add(want["wmtype"])
    assert {0, 1} <= types


def test_two_references_at_cif_twice_on_one_scratch(hip, ref):
    s, r = ec.pair("shear_352x288")
    refs = [ec.strided(r, 32, 200), ec.pair("rot_352x288")[1]]
    out = hip.gm_estimate_picture(s, refs, repeat=2)
    assert not ec.same_estimate(out[0], ec.reference(ref, "shear_352x288"))
    assert not ec.same_estimate(out[1], fc.ref_estimate(ref, s, refs[1], 0, 0))


def test_rotzoom_model_only(hip, ref):
    for name in ("shear_96x80", "rot_96x80"):
        s, r = ec.pair(name)
        out = hip.gm_estimate_picture(s, [r], rotzoom_model_only=1)
        assert out[0].n_models == 1 and not ec.same_estimate(out[0], ec.reference(ref, name, rotzoom_model_only=1))


def test_the_single_call_equals_the_three_calls_with_ransac_on_the_host(hip, ref, pkg):
    """the parent's way: correspondences from the device, the reference's fit and conversion on the host, jobs uploaded to the refinement, frame error, the decision"""
    for name in ("rot_96x80", "shear_96x80", "shifted_96x80"):
        s, r = ec.pair(name)
        corr = hip.gm_correspondences_batch(s, [r])[0]
        records = []
        for t in (fc.ROTZOOM, fc.AFFINE):
            fit = fc.ref_fit_points(ref, corr, t)
            rec = dict(num_inliers_kept=fit["num_inliers_kept"], fit_wmtype=fit["wmtype"], wmmat=fit["wmmat"], wmtype=-1, best_error=-1)
            if fit["num_inliers_kept"] and fit["wmtype"]:
                job = pkg.GmJob(ref=0, wmtype=fit["wmtype"], wmmat=(C.c_int32 * 8)(*fit["wmmat"]), n_refinements=5, best_frame_error=g.INT64_MAX)
                res, _ = hip.gm_refine_picture(s, [r], (pkg.GmJob * 1)(job))
                rec.update(wmmat=list(res[0].wmmat), wmtype=res[0].wmtype, best_error=res[0].best_error)
            records.append(rec)
        ferr = int(hip.gm_frame_error_batch(s, [r])[0])
        want = dict(records=records, ref_frame_error=ferr)
        want["wmmat"], want["wmtype"] = fc.ref_decide(ref, records, ferr, 0, 0)
        out = hip.gm_estimate_picture(s, [r])
        assert not ec.same_estimate(out[0], want), name
        assert want["wmtype"] == ec.reference(ref, name)["wmtype"]


def test_bad_arguments_with_a_live_context(hip, pkg):
    L = pkg.lib()
    d = hip.empty(1 << 16)
    try:
        for c in abi.EST_BAD:
            assert abi.call_estimate(pkg, L, hip.h, d.value, **c) == abi.BAD_ARG, c
            assert b"svt_hip_gm_estimate_picture_dev: bad argument" in L.svt_hip_last_error(hip.h)
    finally:
        hip.free(d)
