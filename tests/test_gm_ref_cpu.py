"""CPU, reference only: the inputs of the global-motion GPU tests deserve their names.  (a) the Python restatement of the walk equals
svt_av1_refine_integerized_param on every shared walk; (b) the generated error table equals error_measure_lut; and the walks show what they are there to show:
(c) stale rows 4-5 of a ROTZOOM model change a result, (d) a walk that starts valid steps onto an invalid model and stays there with error 1, (e) a walk that
starts invalid, (f) a translation that reaches the +-4096 clamp, (g) a directional run longer than the speculation depth K, (h) best_frame_error below the
initial error."""
import ctypes as C

import numpy as np
import pytest

import gm_common as g


@pytest.mark.parametrize("name", g.WALK_NAMES)
def test_restatement_equals_the_reference(ref, name):
    (mat, wmtype, err), r = g.walk_reference(ref, name)
    assert (r["wmmat"], r["wmtype"], r["error"]) == (mat, wmtype, err)
    assert r["probes"] >= 1


def test_error_table_formula_equals_the_reference(ref):
    lut = (C.c_int * 512).in_dll(ref, "error_measure_lut")
    assert np.array_equal(np.array(lut[:], np.int64), g.error_table())


def test_early_exit_is_invisible(ref):
    for name in ("rotzoom_near", "affine_near", "frame_error_wins", "onto_invalid_affine"):
        wk = g.walk_by_name(name)
        src, rf = g.walk_planes(wk)
        full = g.restated_walk(ref, wk["start"], wk["wmtype"], rf, src, wk["n"], wk["bfe"], early_exit=False)
        assert full == g.walk_reference(ref, name)[1]


def test_stale_rows_change_a_rotzoom_walk(ref):
    differs = []
    for wk in g.WALKS:
        if wk["wmtype"] != g.ROTZOOM:
            continue
        src, rf = g.walk_planes(wk)
        fresh = g.restated_walk(ref, wk["start"], wk["wmtype"], rf, src, wk["n"], wk["bfe"], fresh_rows=True)
        stale = g.walk_reference(ref, wk["name"])[1]
        if (fresh["wmmat"], fresh["error"]) != (stale["wmmat"], stale["error"]):
            differs.append(wk["name"])
    assert "stale_rows_100" in differs


@pytest.mark.parametrize("name", ["onto_invalid_rotzoom", "onto_invalid_affine"])
def test_walk_steps_onto_an_invalid_model_and_stays(ref, name):
    wk = g.walk_by_name(name)
    start = list(wk["start"]) + [0, 0]
    g.force_wmtype(start, wk["wmtype"])
    assert g.ref_shear(ref, start[:6])[4] == 1
    (mat, _, err), r = g.walk_reference(ref, name)
    assert err == 1 and mat != start and r["invalid"] > 0


def test_walk_that_starts_invalid(ref):
    wk = g.walk_by_name("starts_invalid")
    start = list(wk["start"]) + [0, 0]
    assert g.ref_shear(ref, start[:6])[4] == 0
    (mat, _, err), r = g.walk_reference(ref, "starts_invalid")
    assert err == 1 and mat == start and r["invalid"] == r["probes"]


def test_translation_reaches_the_clamp(ref):
    (mat, wmtype, _), _ = g.walk_reference(ref, "translation_clamp")
    assert mat[0] == 4096 << 10 and wmtype == g.TRANSLATION
    assert g.add_param_offset(0, mat[0], 1) == mat[0]


def test_runs_on_both_sides_of_the_speculation_depth(ref):
    runs = {n: g.walk_reference(ref, n)[1]["longest_run"] for n in g.WALK_NAMES}
    assert max(runs.values()) > 2 * g.K + 2          # outlives the first batch and a whole continuation batch
    assert g.K + 1 in runs.values()                  # K accepted steps, the refusal in the next round
    assert any(0 < v <= g.K for v in runs.values())  # ends inside the speculated part


def test_best_frame_error_below_the_initial_error(ref):
    wk = g.walk_by_name("frame_error_wins")
    src, rf = g.walk_planes(wk)
    start = list(wk["start"]) + [0, 0]
    g.force_wmtype(start, wk["wmtype"])
    assert g.ref_warp_error(ref, g.make_wm(start, wk["wmtype"]), rf, src) > wk["bfe"]
    (mat, _, err), _ = g.walk_reference(ref, "frame_error_wins")
    assert err == wk["bfe"] and mat == start


def test_golden_file_is_what_the_generator_records(ref):
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_gm_golden as mk
    stored = np.load(os.path.join(ROOT, "tests", "golden", "gm_walks.npz"))
    now = mk.record(ref)
    assert sorted(stored.files) == sorted(now)
    for k in now:
        assert np.array_equal(stored[k], now[k]) and stored[k].dtype == now[k].dtype, k
    assert stored["src"].shape[0] <= 80 and stored["src"].shape[1] <= 96
