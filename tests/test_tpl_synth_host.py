"""CPU: svt_hip_tpl_window_host (svt-av1_amd/csrc/tpl_synth.h run serially) against the Python restatement of the reference (tests/tpl_synth_common.py) on
every window the GPU tests run -- all grids, r0, both base sums, factors and betas, doubles by bit pattern -- and both against the closed forms worked out by
hand.  tests/tpl_synth_host_test.cpp runs the same header stand-alone, plain and under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tpl_common as T
import tpl_synth_common as S
from conftest import ROOT

CASES = S.window_cases()
_restated = {}


def restated(i):
    """The restatement of case i, computed once and shared; the tests never change it."""
    if i not in _restated:
        out, grids, peak = S.restate(CASES[i])
        assert peak < S.LIMIT, f"{CASES[i]['name']}: a value reached 2^{peak.bit_length() - 1}: the restatement models no overflow"
        grids.setflags(write=False)
        _restated[i] = (out, grids)
    return _restated[i]


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{k}_{c['name']}" for k, c in enumerate(CASES)])
def test_host_form_matches_the_restatement(pkg, i):
    case = CASES[i]
    want = restated(i)
    got = S.host_window(pkg, case)
    S.same(got, want, case["name"])
    assert not np.isnan(want[0]["factors"]).any() and not np.isnan(want[0]["beta"]).any()   # a NaN's sign and payload are not the arithmetic under test
    S.check_closed_forms(case["name"], want)
    S.check_closed_forms(case["name"], got)


def test_closed_forms_are_among_the_cases(pkg):
    names = [c["name"] for c in CASES]
    closed = [n for i, n in enumerate(names) if S.check_closed_forms(n, restated(i))]
    assert closed == ["chain"] + [f"single{mb}{mv}" for mb, mv, _, _ in S.SINGLE]


def contention_sums(case):
    """What every macroblock's block 0 (area = the whole cell, nothing propagated: picture 1 receives nothing) adds up to, from the records alone."""
    s = case["pics"][1]["stats"]
    return int((s["recrf_rate"] - s["srcrf_rate"]).sum()), int((s["recrf_dist"] - s["srcrf_dist"]).sum())


def test_contention_sums(pkg):
    """The one-cell cases have a closed form too: the cell holds the plain sums of the records' differences, signs mixed."""
    c16, c8 = S.contention_case(), S.contention_case_8x8()
    for c in (c16, c8):
        s = c["pics"][1]["stats"]
        assert ((s["recrf_rate"] < s["srcrf_rate"]).any() and (s["recrf_rate"] > s["srcrf_rate"]).any() and (s["recrf_dist"] < s["srcrf_dist"]).any())
    _, grids = S.host_window(pkg, c16)
    want = np.zeros_like(grids); want[0, 8, 10] = contention_sums(c16)
    assert (grids == want).all()
    _, grids = S.host_window(pkg, c8)
    want = np.zeros_like(grids); want[0, 17:19, 21:23] = contention_sums(c8)   # area 64 of 64: every quarter adds the whole difference
    assert (grids == want).all()


def test_r0_kept_and_unit_factors(pkg):
    first, _ = S.r0_kept_cases()
    out, grids = S.host_window(pkg, first)
    assert out["mc_dep_cost_base"] == 0 and out["intra_cost_base"] == 0 and out["r0"] == first["r0_in"] == 0.3125
    assert (out["factors"] == 1.2).all() and (out["beta"] == 1.0).all() and not grids.any()


def test_rf_idx_minus_one_onto_itself(pkg):
    """The POC-0 rule with the window's first picture at POC 0: its records without a reference add into their own cells only (zero vector, whole area), and
    the vector fields of such a record are not read."""
    w, h = 40, 24
    s = S.blank_stats(w, h, srcrf_dist=3, recrf_dist=10, srcrf_rate=2, recrf_rate=7, rf_idx=-1)
    s["mv_row"], s["mv_col"] = 77, -300   # the reference never copies a vector into a record without a reference (:795-798)
    for cl in (3, 4):
        case = S.make_case("self", w, h, cl, [S.pic(0, s, [])])
        out, grids = S.host_window(pkg, case)
        S.same((out, grids), S.restate(case)[:2], "self")
        want = np.zeros_like(grids)
        if cl == 3: want[0, :3, :5] = (5, 7)
        else: want[0, :2, :3] = (5, 7)   # 16 x 16 cells: rows 0 and 16 < 24, columns 0, 16, 32 < 40
        assert (grids == want).all()


def test_out_of_range_rf_idx_and_zero_recrf(pkg):
    """What the header defines where the reference has no defined result: rf_idx outside -1 .. 6 scatters nothing, recrf_dist == 0 propagates nothing."""
    w, h = 64, 64
    s1 = S.blank_stats(w, h, srcrf_dist=5, recrf_dist=0, srcrf_rate=1, recrf_rate=1, rf_idx=0)
    s2 = S.blank_stats(w, h, srcrf_dist=1, recrf_dist=9, srcrf_rate=1, recrf_rate=1, rf_idx=0)
    s0 = S.blank_stats(w, h, srcrf_dist=1, recrf_dist=9, srcrf_rate=1, recrf_rate=4, rf_idx=7)
    s0[1, 2]["rf_idx"] = -128
    case = S.make_case("edges", w, h, 4, [S.pic(5, s0, []), S.pic(6, s1, [5]), S.pic(7, s2, [6])])
    out, grids = S.host_window(pkg, case)
    want = np.zeros_like(grids)
    want[1, :, :, 1] = 8          # from picture 2
    want[0, :, :, 1] = -5         # from picture 1: cur_dep_dist = -5, the propagated part of its 8 is 0 by definition
    assert (grids == want).all()
    S.same((out, grids), S.restate(case)[:2], "edges")


def _dump(pkg, case, want, path):
    out, grids = want
    with open(path, "wb") as f:
        f.write(np.array([case["w"], case["h"], case["cell_log2"], case["sb_size"], case["base_rdmult"], len(case["pics"])], np.int32).tobytes())
        f.write(np.float64(case["r0_in"]).tobytes())
        for p, rw in zip(case["pics"], S.case_ref_windows(pkg, case)):
            f.write(np.array([p["on"]] + rw, np.int32).tobytes())
            f.write(np.ascontiguousarray(p["stats"], T.STATS_DTYPE).tobytes())
        f.write(np.ascontiguousarray(grids).tobytes())
        hd = pkg.TplR0BetaHeader(out["r0"], out["intra_cost_base"], out["mc_dep_cost_base"])
        f.write(bytes(hd) + np.ascontiguousarray(out["factors"], np.float64).tobytes() + np.ascontiguousarray(out["beta"], np.float64).tobytes())


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_standalone_program(pkg, flags, tmp_path):
    """tpl_synth.h in a program of its own (no Python, nothing preloaded): the closed forms from stored numbers, then two dumped windows -- vectors that leave
    the picture on every side, both cell sizes -- against the restatement's grids and outputs."""
    exe = str(tmp_path / "tpl_synth_host_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", *flags, os.path.join(ROOT, "tests", "tpl_synth_host_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout + r.stderr)[-3000:]
    for i in (0, 3):
        assert CASES[i]["name"] in ("small3_poc0", "small4_poc0")
        path = str(tmp_path / f"case{i}.bin")
        _dump(pkg, CASES[i], restated(i), path)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout + r.stderr)[-3000:]
