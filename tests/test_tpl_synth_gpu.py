"""GPU: svt_hip_tpl_window_dev (and the two single-step entry points) against the Python restatement of the reference's tpl_mc_flow after the dispensers
(tests/tpl_synth_common.py) and against the host form svt_hip_tpl_window_host, bit for bit: every cell of every picture's grid, r0, both base sums, every
factor and every beta (doubles by bit pattern), with guard bands around every buffer the device writes.  The closed forms worked out by hand are checked on the
device's results as well."""
import ctypes as C
import os

import numpy as np
import pytest

import tpl_common as T
import tpl_synth_common as S
from conftest import ROOT
from test_tpl_synth_abi import bad_argument_cases, call
from test_tpl_synth_host import contention_sums

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "tpl_dispenser_200x136.npz")


def _check(hip, pkg, cases, n_max=4, steps=False, twice=False):
    """Every case (one geometry) on one set of device buffers, one after the other: the grids still hold the previous window (or the marker) when a call
    starts.  Returns the device results."""
    c0 = cases[0]
    D = S.DeviceWindow(hip, pkg, c0["w"], c0["h"], c0["cell_log2"], c0["sb_size"], n_max)
    results = []
    try:
        for case in cases:
            out, grids, peak = S.restate(case)
            assert peak < S.LIMIT
            host = S.host_window(pkg, case)
            S.same(host, (out, grids), case["name"] + " (host form)")
            for _ in range(2 if twice else 1):
                got = D.run(case)
                S.same(got, (out, grids), case["name"])
            if steps:
                S.same(D.run_in_steps(case), (out, grids), case["name"] + " (single steps)")
            print(f"{case['name']}: r0 {out['r0']!r} bases {out['intra_cost_base']} {out['mc_dep_cost_base']} non-zero cells {[int(g.any(axis=-1).sum()) for g in grids]}")
            results.append(got)
        return results
    finally:
        D.close()


@pytest.mark.parametrize("cell_log2", [3, 4])
def test_window_small(hip, pkg, cell_log2):
    """200 x 136, four pictures, at both cell sizes; rf_idx == -1 meaning the picture itself (POC 0 first), another picture (POC 0 second) and nothing."""
    cases = [S.small_window(cell_log2, pocs) for pocs in ((0, 8, 4, 2), (16, 0, 8, 4), (16, 32, 24, 20))]
    res = _check(hip, pkg, cases, steps=True)
    for case, (out, grids) in zip(cases, res):
        assert grids[2].any() and not case["pics"][2]["on"]          # the picture that is off still receives
        assert not grids[3].any()                                     # nothing references the last picture
        s = case["pics"][0]["stats"]
        assert (s["rf_idx"] == -1).any() and (s["recrf_dist"] < s["srcrf_dist"]).any()
    assert grids.shape[1:3] == ((18, 26) if cell_log2 == 3 else (9, 13))


def test_closed_forms(hip, pkg):
    """The chain, the single scatters and the truncation, stated as literals in tests/tpl_synth_common.py, on the device."""
    (got,) = _check(hip, pkg, [S.chain_case()])
    assert S.check_closed_forms("chain", got)
    cases = [S.single_case(mb, mv, **kw) for mb, mv, kw, _ in S.SINGLE]
    for case, got in zip(cases, _check(hip, pkg, cases, n_max=2)):
        assert S.check_closed_forms(case["name"], got)


def test_one_cell_contention(hip, pkg):
    """352 x 288: every source block of picture 1 adds into the same cell of picture 0 (16 x 16 cells: 396 adds on each of two addresses; 8 x 8 cells: 396 on
    each of eight), signs mixed.  Twice into grids that are not zero when the call starts."""
    c16, c8 = S.contention_case(), S.contention_case_8x8()
    (_, g16), = _check(hip, pkg, [c16], n_max=2, twice=True)
    assert tuple(g16[0, 8, 10]) == contention_sums(c16) and int((g16 != 0).sum()) == 2
    (_, g8), = _check(hip, pkg, [c8], n_max=2, twice=True)
    assert all(tuple(g8[0, r, c]) == contention_sums(c8) for r in (17, 18) for c in (21, 22)) and int((g8 != 0).sum()) == 8


def test_r0_kept_and_unit_factors(hip, pkg):
    """Picture 0 off with zero records: mc_dep_cost_base == 0, r0 == r0_in, factors 1.2, betas 1.0; then a window with real records on the same buffers."""
    first, second = S.r0_kept_cases()
    (out, grids), _ = _check(hip, pkg, [first, second])
    assert out["mc_dep_cost_base"] == 0 and out["r0"] == first["r0_in"] == 0.3125
    assert (out["factors"] == 1.2).all() and (out["beta"] == 1.0).all() and not grids.any()


def test_sb128_and_720p_rule(hip, pkg):
    """128 x 128 superblocks at both cell sizes; 720 x 728 is where the binding's rule (min(w, h) >= 720) picks 16 x 16 cells: 45 x 46 macroblocks with a
    trailing half row."""
    _check(hip, pkg, [S.small_window(3, (0, 8, 4, 2), seed=2, sb_size=128)])
    case = S.big_case()
    P = pkg.tpl_synth_params(case["w"], case["h"], case["base_rdmult"], r0_in=case["r0_in"], sb_size=128)
    assert P.cell_log2 == case["cell_log2"] == 4 and pkg.tpl_synth_params(712, 1280, 1).cell_log2 == 3
    (out, grids), = _check(hip, pkg, [case], n_max=3)
    assert out["beta"].shape == (6, 6) and out["factors"].shape == (46, 45) and grids.shape == (3, 46, 45, 2)
    D = S.DeviceWindow(hip, pkg, 720, 728, 4, 128, 3)
    try:
        S.same(D.run(case, params=P), (out, grids), "the binding's cell size")
    finally:
        D.close()


def test_after_the_dispenser(hip, pkg):
    """One 352 x 288 window of three pictures whose records are the ones svt_hip_tpl_dispenser_picture_dev left on the device: the window call reads them where
    they lie.  They are downloaded afterwards, for the restatement and the host form only."""
    w, h, pad = 352, 288, T.PAD
    L = pkg.lib()
    qp = T.device_qparams(pkg, np.load(GOLDEN)["qp"])
    # POCs 0, 8, 4: picture 1 references the first, picture 2 both others (slot 0, which wins most of the generator's ties, names picture 1)
    slot_pocs = [[999, 998, 997], [0, 999, 0], [8, 0, 999]]
    pocs = [0, 8, 4]
    D = S.DeviceWindow(hip, pkg, w, h, 3, 64, 3)
    held = []
    try:
        for i in range(3):
            case = T.make_case(w, h, T.case_seed(w, h) + i)
            up = lambda a: (held.append(hip.to_device(np.ascontiguousarray(a))), held[-1])[1]
            stride = case["cur"].shape[1]
            origin = lambda d: C.c_void_p(d.value + pad * stride + pad)
            d_cur = origin(up(case["cur"]))
            refs = (pkg.TplRef * 7)()
            for r in range(3):
                sp, rp = case["refs"][r]
                refs[r].d_src, refs[r].src_stride = origin(up(sp)).value, stride
                refs[r].d_rec, refs[r].rec_stride = (refs[r].d_src if rp is sp else origin(up(rp)).value), stride
            om, oc = hip.intra_ois_picture(d_cur, stride, w, h)
            P = pkg.TplParams()
            P.w, P.h, P.pad, P.q = w, h, pad, qp
            P.use_ois, P.add_residual, P.rate, P.best_ref_only = 1, 1, 1, 0
            d_recon = up(np.zeros_like(case["cur"]))
            d_scratch = hip.empty(L.svt_hip_tpl_dispenser_scratch_bytes(w, h)); held.append(d_scratch)
            hip.check(L.svt_hip_tpl_dispenser_picture_dev(hip.h, C.byref(P), d_cur, stride, refs, up(case["mv"]), up(case["mask"]), up(om), up(oc), origin(d_recon), stride,
                                                           D.d_stats[i], d_scratch), "tpl_dispenser_picture")
        shell = S.make_case("after_the_dispenser", w, h, 3, [S.pic(pocs[i], None, slot_pocs[i]) for i in range(3)])
        got = D.run(shell, upload=False)
        for i in range(3):
            shell["pics"][i]["stats"] = D.stats_to_host(i, (18, 22))
        s = shell["pics"][2]["stats"]
        assert (s["rf_idx"] == -1).any() and (s["rf_idx"] >= 0).any() and (s["is_inter"] != 0).any() and (s["is_inter"] == 0).any() and (s["mv_row"] != 0).any()
        out, grids, peak = S.restate(shell)
        assert peak < S.LIMIT
        S.same(got, (out, grids), "after the dispenser")
        S.same(S.host_window(pkg, shell), (out, grids), "after the dispenser (host form)")
        assert grids[0].any() and grids[1].any() and out["mc_dep_cost_base"] > out["intra_cost_base"] > 0
    finally:
        hip.check(L.svt_hip_sync(hip.h), "sync")
        hip.free(*held)
        D.close()


def test_bad_arguments_live_context(hip, pkg):
    """Code and text of every refusal with a live context, before anything is launched (so the pointers need not be valid)."""
    L = pkg.lib()
    names = dict(synth="svt_hip_tpl_synth_picture_dev", r0beta="svt_hip_tpl_r0beta_dev", window="svt_hip_tpl_window_dev")
    d = hip.empty(4096)
    try:
        ok, wrong = bad_argument_cases(pkg, d.value)
        for change, where, word in wrong:
            a = dict(ok); a.update(change)
            for which in where:
                if which == "host": continue
                assert call(L, hip.h, which, a) == 2, (which, change)
                text = L.svt_hip_last_error(hip.h).decode()
                assert text.startswith(names[which] + ": ") and word in text, (which, change, text)
        hip.check(L.svt_hip_sync(hip.h), "sync")
    finally:
        hip.free(d)
