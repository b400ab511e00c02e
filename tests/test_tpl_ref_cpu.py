"""CPU: the reference composition of the TPL dispenser (tests/tpl_common.py: ref_dispenser).  It does not depend on the order in which independent
macroblocks are visited (which is what lets the device run them in parallel) and notices an order that breaks a dependency; rate_estimator's floating-point
expression is a bit length; the stored golden result is reproduced; and the generated inputs exercise what the device tests rely on -- asserted here on the
reference's result alone, before any device is involved."""
import math
import os

import numpy as np
import pytest

import intra_common as ic
import tpl_common as T
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "tpl_dispenser_200x136.npz")


def test_log1p_expression_is_a_bit_length():
    """(int)(log1p(level) / log(2.0)) + 1 == bit length of level + 1 for every level svt_av1_quantize_fp can produce at 16x16 (at most 32767 * 2^14 >> 16)."""
    for level in range(8192):
        assert int(math.log1p(level) / math.log(2.0)) + 1 == (level + 1).bit_length(), level


def test_golden_file_shape():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert g["cur"].shape == (136, 200) and g["stats"].shape == (9, 13) and g["stats"].dtype == T.STATS_DTYPE and g["recon"].shape == (136, 200)
    assert g["mv"].shape == (3, 9, 13) and g["mask"].shape == (9, 13) and g["qp"].shape == (7, 2)
    assert not g["stats_intra"]["is_inter"].any() and (g["stats_intra"]["rf_idx"] == -1).all()


@pytest.fixture(scope="module")
def small(ref):
    case = T.make_case(200, 136, T.case_seed(200, 136))
    om, oc = ic.ref_ois(ref, T.cur_plane(case), 200, 136)
    return case, om, oc


def test_golden_equals_a_fresh_composition(ref, small):
    case, om, oc = small
    gcase, g = T.load_golden(GOLDEN)
    assert (gcase["cur"] == case["cur"]).all() and (gcase["mv"] == case["mv"]).all() and (gcase["mask"] == case["mask"]).all()
    assert all((gcase["refs"][r][k] == case["refs"][r][k]).all() for r in range(3) for k in range(2))
    assert (g["ois_mode"] == om).all() and (g["ois_cost"] == oc).all() and (g["qp"] == T.qparams(ref, 140)).all()
    stats, rec = T.ref_dispenser(ref, gcase, g["ois_mode"], g["ois_cost"], g["qp"])
    assert T.stats_equal(stats, g["stats"]) and (rec == T.golden_recon(g, "recon", 200, 136)).all()
    stats, rec = T.ref_dispenser(ref, T.all_intra(gcase), g["ois_mode"], g["ois_cost"], g["qp"])
    assert T.stats_equal(stats, g["stats_intra"]) and (rec == T.golden_recon(g, "recon_intra", 200, 136)).all()


@pytest.mark.parametrize("qindex", T.QINDEXES)
def test_order_independence(ref, small, qindex):
    """z-order (the reference's), raster, x + 2y, and "every inter macroblock first, then the intra ones in x + 2y order" (the device's) agree; so they do on
    the all-intra picture, where reversed raster order does not: the comparison notices a broken order."""
    case, om, oc = small
    qp = T.qparams(ref, qindex)
    mbw, mbh = 13, 9
    z = T.ref_dispenser(ref, case, om, oc, qp, T.zorder(mbw, mbh))
    inter_first = sorted(T.raster(mbw, mbh), key=lambda p: (0 if z[0]["is_inter"][p[1], p[0]] else 1, p[0] + 2 * p[1]))
    for order in (T.raster(mbw, mbh), T.wavefront(mbw, mbh), inter_first):
        o = T.ref_dispenser(ref, case, om, oc, qp, order)
        assert T.stats_equal(o[0], z[0]) and (o[1] == z[1]).all()
    ai = T.all_intra(case)
    z = T.ref_dispenser(ref, ai, om, oc, qp, T.zorder(mbw, mbh))
    assert T.chain(z[0]) == mbw + 2 * mbh - 2
    for order in (T.raster(mbw, mbh), T.wavefront(mbw, mbh)):
        o = T.ref_dispenser(ref, ai, om, oc, qp, order)
        assert T.stats_equal(o[0], z[0]) and (o[1] == z[1]).all()
    o = T.ref_dispenser(ref, ai, om, oc, qp, T.raster(mbw, mbh)[::-1])
    assert not T.stats_equal(o[0], z[0]) or (o[1] != z[1]).any()


def test_generator_conditions(ref):
    """What the device tests need from the inputs, over the case set (200x136 and 352x288 at the three qindex values)."""
    sums = []
    for (w, h) in ((200, 136), (352, 288)):
        case = T.make_case(w, h, T.case_seed(w, h))
        om, oc = ic.ref_ois(ref, T.cur_plane(case), w, h)
        for q in T.QINDEXES:
            s = T.summary(case, T.ref_dispenser(ref, case, om, oc, T.qparams(ref, q))[0])
            print(w, h, q, s)
            sums.append(s)
    for s in sums:
        assert 0.5 <= s["inter_share"] <= 0.95, s
        assert s["dir_intra_share"] >= 0.05, s
        assert s["chain"] >= 3, s
    for k in ("inter_eob0", "inter_eobp", "intra_eob0", "intra_eobp", "leave"):
        assert any(s[k] > 0 for s in sums), k
    for r in range(3):
        assert any(s["wins"][r] > 0 for s in sums), r
