"""CPU: svt_hip_gm_decide_host (the model loop of compute_global_motion, EbGlobalMotionEstimation.c:303-399) and the restated gm_get_params_cost against the
reference's own functions.  The expected side composes svt_get_shear_params, gm_get_params_cost and svt_av1_is_enough_erroradvantage in the loop's order
(gm_fit_common.ref_decide); every branch of the loop has a record set that takes it, and the test says which branch it took."""
import ctypes as C

import numpy as np
import pytest

import gm_common as g
import gm_fit_common as fc

ONE = g.ONE
ID = list(fc.DEFAULT_WM)


def test_params_cost_against_the_reference(pkg, ref):
    L = pkg.lib()
    rng = np.random.default_rng(5)
    n = 0
    for spread in (2, 64, 1000, 8192):
        for _ in range(700):
            m = [int(v) for v in rng.integers(-spread, spread + 1, 8)]
            m[0], m[1] = int(rng.integers(-(1 << 22), 1 << 22)), int(rng.integers(-(1 << 22), 1 << 22))
            if spread == 2:
                m[0] >>= 8; m[1] >>= 8
            m[2] += ONE; m[5] += ONE; m[6] = m[7] = 0
            for wmtype in (0, 1, 2, 3):
                mm = list(m)
                g.force_wmtype(mm, wmtype)
                for hp in (0, 1):
                    assert L.svt_hip_gm_params_cost_host((C.c_int32 * 8)(*mm), wmtype, hp) == fc.ref_params_cost(ref, mm, wmtype, hp), (mm, wmtype, hp)
                    n += 1
    assert n >= 4000


def _rec(kept, fit_type, wmmat=ID, wmtype=-1, err=-1):
    return dict(num_inliers_kept=kept, fit_wmtype=fit_type, wmmat=list(wmmat), wmtype=wmtype, best_error=err)


RZ = [3 * ONE, -2 * ONE, ONE + 600, 500, -500, ONE + 600, 0, 0]
AFF = [2 * ONE + 1024, ONE, ONE + 400, 300, -200, ONE - 350, 0, 0]
SHEAR_BAD = [0, 0, ONE + 20000, 30000, -30000, ONE + 20000, 0, 0]
AFF_BIG = [100 * ONE + 5120, -90 * ONE - 3072, ONE + 4000, 3000, 3000, ONE - 3500, 0, 0]
TRN = [5 * ONE + 3000, -3 * ONE - 9000, ONE, 0, 0, ONE, 0, 0]
NONE = _rec(0, 0)
# name -> (records, ref_frame_error, rotzoom_model_only, what the loop must return: None = the identity, else which record's type)
CASES = {
    "rotzoom_accepted": ([_rec(200, 2, RZ, 2, 300000), _rec(180, 3, AFF, 3, 100)], 1000000, 0, 2),
    "rotzoom_rejected_affine_accepted": ([_rec(200, 2, RZ, 2, 900000), _rec(180, 3, AFF, 3, 300000)], 1000000, 0, 3),
    "both_rejected_by_the_ratio": ([_rec(200, 2, RZ, 2, 900000), _rec(180, 3, AFF, 3, 700000)], 1000000, 0, None),
    "rejected_by_the_product": ([NONE, _rec(180, 3, AFF_BIG, 3, 640000)], 1000000, 0, None),      # 0.64 < 0.65, but 0.64 * the cost of six large parameters >= 20000
    "same_ratio_cheaper_model_accepted": ([_rec(200, 2, RZ, 2, 640000), NONE], 1000000, 0, 2),
    "invalid_shear": ([_rec(200, 2, SHEAR_BAD, 2, 10), _rec(180, 3, AFF, 3, 300000)], 1000000, 0, 3),
    "invalid_shear_only": ([_rec(200, 2, SHEAR_BAD, 2, 10), NONE], 1000000, 0, None),
    "translation_result": ([_rec(200, 2, TRN, 1, 200000), _rec(180, 3, AFF, 3, 100)], 1000000, 0, 1),
    "frame_error_zero_model_survives": ([_rec(200, 2, RZ, 2, 0), _rec(180, 3, AFF, 3, 0)], 0, 0, 3),
    "frame_error_zero_rotzoom_survives_an_empty_affine": ([_rec(200, 2, RZ, 2, 0), NONE], 0, 0, 2),
    "frame_error_zero_rotzoom_only": ([_rec(200, 2, RZ, 2, 0), NONE], 0, 1, 2),
    "rotzoom_model_only_stops": ([_rec(200, 2, RZ, 2, 900000), _rec(180, 3, AFF, 3, 300000)], 1000000, 1, None),
    "no_inliers": ([NONE, NONE], 1000000, 0, None),
    "identity_fit_not_refined": ([_rec(100, 0), _rec(100, 0)], 1000000, 0, None),
    "rule_dropped_rotzoom_affine_accepted": ([_rec(0, 2, RZ, 2, 1), _rec(180, 3, AFF, 3, 300000)], 1000000, 0, 3),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("allow_hp", [0, 1])
def test_decision_against_the_composed_reference(pkg, ref, name, allow_hp):
    records, ferr, rz_only, branch = CASES[name]
    want = fc.ref_decide(ref, records, ferr, rz_only, allow_hp)
    tab = (pkg.GmModelRecord * 2)()
    for i, r in enumerate(records):
        tab[i] = pkg.GmModelRecord(r["num_inliers_kept"], r["fit_wmtype"], (C.c_int32 * 8)(*r["wmmat"]), r["wmtype"], 0, r["best_error"])
    wmmat, wmtype = (C.c_int32 * 8)(), C.c_int32(-9)
    assert pkg.lib().svt_hip_gm_decide_host(tab, ferr, rz_only, allow_hp, wmmat, C.byref(wmtype)) == 0
    assert (list(wmmat), wmtype.value) == (want[0], want[1])
    # the case takes the branch its name says
    assert want[1] == (0 if branch is None else branch)
    if branch is None:
        assert want[0] == ID
    if name == "translation_result":   # rewritten to the translation-only precision, which depends on allow_high_precision_mv
        assert want[0][0] % (1 << (13 if allow_hp else 14)) == 0 and want[0][:2] != TRN[:2]
    if name == "invalid_shear":
        assert not g.ref_shear(ref, SHEAR_BAD[:6])[4]


def test_the_hp_flag_changes_a_translation(pkg, ref):
    records = CASES["translation_result"][0]
    assert fc.ref_decide(ref, records, 1000000, 0, 0)[0] != fc.ref_decide(ref, records, 1000000, 0, 1)[0]
