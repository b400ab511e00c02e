"""GPU: svt_hip_tpl_dispenser_picture_dev against the reference's tpl_mc_flow_dispenser composed from its own functions (tests/tpl_common.py: ref_dispenser):
every field of every macroblock's statistics and every sample of the padded reconstruction, bit for bit; a guard band around the destination stays untouched."""
import ctypes as C
import os

import numpy as np
import pytest

import intra_common as ic
import tpl_common as T
from conftest import ROOT
from test_tpl_abi import bad_argument_cases, call

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "tpl_dispenser_200x136.npz")

_cases = {}


def _case(L, w, h):
    """(case, ois_mode, ois_cost) of the seeded generator, the intra tables from the reference's open-loop search."""
    if (w, h) not in _cases:
        case = T.make_case(w, h, T.case_seed(w, h))
        _cases[(w, h)] = (case,) + ic.ref_ois(L, T.cur_plane(case), w, h)
    return _cases[(w, h)]


def _check(hip, pkg, L, case, om, oc, qindex, pad=T.PAD, extra_stride=0, offset=0, calls=1, **flags):
    qp = T.qparams(L, qindex)
    rs, rr = T.ref_dispenser(L, case, om, oc, qp, pad=pad, **flags)
    s = T.summary(case, rs)
    print(f"{case['w']}x{case['h']} q{qindex} {flags}: {s}")
    ds, dr, untouched = T.device_dispenser(hip, pkg, case, om, oc, qp, pad=pad, extra_stride=extra_stride, offset=offset, calls=calls, **flags)
    T.compare(ds, dr, rs, rr, pad)
    assert untouched, "samples outside (w + 2 pad) x (h + 2 pad) were written"
    return rs, s


def test_trailing_half_macroblocks(hip, pkg, ref):
    """200x136: the last macroblock column is 8 wide, the last row 8 high; both are processed as full blocks."""
    rs, _ = _check(hip, pkg, ref, *_case(ref, 200, 136), 140)
    assert rs.size == 117


@pytest.mark.parametrize("qindex", T.QINDEXES)
def test_cif(hip, pkg, ref, qindex):
    _check(hip, pkg, ref, *_case(ref, 352, 288), qindex)


def test_720p(hip, pkg, ref):
    _, s = _check(hip, pkg, ref, *_case(ref, 1280, 720), 140)
    assert 0.5 <= s["inter_share"] <= 0.95 and s["chain"] >= 3


def test_4k_ois_from_the_device(hip, pkg, ref):
    """3840x2160, the intra tables produced by svt_hip_intra_ois_picture_dev (which tests/test_intra_ois_gpu.py pins to the reference)."""
    case = T.make_case(3840, 2160, T.case_seed(3840, 2160))
    om, oc = ic.device_ois(hip, T.cur_plane(case), 3840, 2160)
    _, s = _check(hip, pkg, ref, case, om, oc, 140)
    assert 0.5 <= s["inter_share"] <= 0.95 and s["chain"] >= 3


def test_all_intra(hip, pkg, ref):
    """No slot in use: every macroblock is intra, the dependency chain is the whole picture (mb_cols + 2 mb_rows - 2 steps)."""
    case, om, oc = _case(ref, 352, 288)
    for q in (40, 230):
        rs, s = _check(hip, pkg, ref, T.all_intra(case), om, oc, q)
        assert s["inter_share"] == 0 and s["chain"] == 22 + 2 * 18 - 2 and (rs["rf_idx"] == -1).all()


@pytest.mark.parametrize("flags", [dict(use_ois=0), dict(add_residual=0), dict(rate=0), dict(best_ref_only=1), dict(use_ois=0, best_ref_only=1, rate=0)])
def test_switches(hip, pkg, ref, flags):
    case, om, oc = _case(ref, 352, 288)
    rs, s = _check(hip, pkg, ref, case, om, oc, 40, **flags)
    if flags.get("use_ois") == 0:
        assert (rs["mode"] == 0).all() and ((rs["is_inter"] != 0) == (case["mask"] != 0)).all()   # INT64_MAX intra cost: inter wins wherever a slot is valid
    if flags.get("rate") == 0:
        assert (rs["srcrf_rate"] == 1).all() and (rs["recrf_rate"] == 1).all()


def test_use_ois_0_without_tables(hip, pkg, ref):
    case, _, _ = _case(ref, 200, 136)
    _check(hip, pkg, ref, case, None, None, 140, use_ois=0)


def test_single_slot_in_list_1(hip, pkg, ref):
    case, om, oc = _case(ref, 352, 288)
    rs, _ = _check(hip, pkg, ref, T.move_slots(case, {1: 5}), om, oc, 140)
    assert set(np.unique(rs["rf_idx"]).tolist()) == {-1, 5}
    rs, _ = _check(hip, pkg, ref, T.move_slots(case, {0: 6, 1: 3, 2: 4}), om, oc, 40, best_ref_only=1)
    assert set(np.unique(rs["rf_idx"]).tolist()) == {-1, 3, 4, 6}


def test_offset_and_odd_stride_views(hip, pkg, ref):
    """Every plane inside a wider buffer: odd strides (different per plane), bases that are not a multiple of 2."""
    case, om, oc = _case(ref, 352, 288)
    _check(hip, pkg, ref, case, om, oc, 140, extra_stride=13, offset=5)
    _check(hip, pkg, ref, *_case(ref, 200, 136), 40, extra_stride=1, offset=3)


def test_two_calls_identical(hip, pkg, ref):
    _check(hip, pkg, ref, *_case(ref, 352, 288), 40, calls=2)


def test_clamp(hip, pkg, ref):
    """pad declared as 32 on planes that carry 96 samples, of which only 32 are border (noise beyond), the outermost macroblocks' vectors pointing outwards by
    33 .. 64 samples: the expected value is the composition with the block position kept inside [-32, w + 16] x [-32, h + 16].  A kernel that forgot the
    clamp still reads allocated memory: it fails by comparison, as the composition without the clamp does here."""
    case, om, oc = _case(ref, 352, 288)
    case = T.clamp_case(case, 32)
    free, _ = T.ref_dispenser(ref, case, om, oc, T.qparams(ref, 140))
    rs, _ = _check(hip, pkg, ref, case, om, oc, 140, pad=32)
    assert not T.stats_equal(rs, free), "no vector of the case needs the clamp"


def test_ois_mode_out_of_range_is_dc(hip, pkg, ref):
    case, om, oc = _case(ref, 200, 136)
    qp = T.qparams(ref, 140)
    wild = om.copy(); wild[::2, 1::3] = 200; wild[1::2, ::4] = 13
    dc = np.where(wild > 12, 0, wild).astype(om.dtype)
    rs, rr = T.ref_dispenser(ref, case, dc, oc, qp)
    ds, dr, untouched = T.device_dispenser(hip, pkg, case, wild, oc, qp)
    T.compare(ds, dr, rs, rr)
    assert untouched and ((rs["is_inter"] == 0) & (wild > 12)).any()


def test_golden_without_the_reference(hip, pkg):
    """The stored result of the 200x136 case (tests/golden/make_tpl_golden.py): holds where the reference library is absent."""
    case, g = T.load_golden(GOLDEN)
    ds, dr, untouched = T.device_dispenser(hip, pkg, case, g["ois_mode"], g["ois_cost"], g["qp"])
    T.compare(ds, dr, g["stats"], T.golden_recon(g, "recon", 200, 136))
    assert untouched
    ds, dr, untouched = T.device_dispenser(hip, pkg, T.all_intra(case), g["ois_mode"], g["ois_cost"], g["qp"])
    T.compare(ds, dr, g["stats_intra"], T.golden_recon(g, "recon_intra", 200, 136))
    assert untouched
    grid = pkg.tpl_stats_grid(ds, False)
    assert grid.shape == (18, 26) and (grid[5, 7] == ds[2, 3]) and pkg.tpl_stats_grid(ds, True).shape == (9, 13)


def test_bad_arguments_with_a_context(hip, pkg):
    """The host-visible bad arguments are refused with a live context too, before anything is launched (so the pointers need not be valid)."""
    L = pkg.lib()
    d = hip.empty(4096)
    try:
        ok, wrong = bad_argument_cases(pkg, d.value)
        for c in wrong:
            a = dict(ok); a.update(c)
            assert call(L, hip.h, a) == 2, c
        hip.check(L.svt_hip_sync(hip.h), "sync")
    finally:
        hip.free(d)
