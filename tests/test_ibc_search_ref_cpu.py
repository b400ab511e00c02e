"""CPU: the numpy restatement of the intra-block-copy full-pel search (tests/ibc_search_common.py) against the reference's recorded results, the conditions its
case lists exist for, and the library's host form against the restatement.

svt_av1_diamond_search_sad_c, svt_av1_refining_search_sad and svt_av1_get_mvpred_var take an IntraBcContext and full_pixel_diamond, exhuastive_mesh_search and
full_pixel_exhaustive are static, so they are pinned by tests/golden/ibc_full_search.npz, made the way ibc_hash.npz was: a throw-away C program outside the
repository, built against the reference with av1me.c included, ran on the 8-bit pictures and job lists of eleven of the cases here (every job that is searched: 500; the wide
strip is left out for its size) and recorded, per job: every diamond pass from step_param to 10 on its own (value, vector, num00 and the re-costed value), full_pixel_diamond, the refinement from
its vector, exhuastive_mesh_search for every scan of the walk, full_pixel_exhaustive, the final x->best_mv of svt_av1_full_pixel_search on a table built by the
reference's own generators and inserter, and av1_is_dv_valid of it.  The file keeps inputs and results only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ibc_hash_common as H
import ibc_search_common as S
from conftest import ROOT, ptr

GOLDEN = os.path.join(ROOT, "tests", "golden", "ibc_full_search.npz")
FORMATS = [(np.uint8, 8), (np.uint16, 8), (np.uint16, 10)]


def run_case(c, dtype=np.uint8, bd=8, jobs=None, mesh=None):
    """-> (plane, table, jc, cc, jobs, results, infos) of the restatement"""
    plane = H.as_format(c["pic"], dtype, bd)
    table = H.table(H.pyramid(plane))
    jc, cc = H.cost_tables(zero=c["zero"])
    p32 = plane.astype(np.int32)
    jobs = c["jobs"] if jobs is None else jobs
    infos = [{} for _ in jobs]
    want = [S.full_search(plane, bd, table, jc, cc, c["patterns"], j, info, mesh=mesh, p32=p32) for j, info in zip(jobs, infos)]
    return plane, table, jc, cc, jobs, want, infos


@pytest.fixture(scope="module")
def runs():
    """{case name: run_case at 8 bits}, made once"""
    return {c["name"]: (c,) + run_case(c) for c in S.cases()}


# ------------------------------------------------------------------------------------------------------------------ the recorded results
def test_restatement_equals_the_recorded_reference():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 100 * 1024
    names = [k[:-5] for k in g.files if k.endswith("_jobs")]
    jobs_seen, shapes, shifts = 0, set(), set()
    for n in names:
        pic, pats, zero = g[str(g[n + "_pic"])], [tuple(p) for p in g[n + "_patterns"].tolist()], bool(g[n + "_zero"])
        assert pic.dtype == np.uint8
        jc, cc = H.cost_tables(zero=zero)
        table, p32 = H.table(H.pyramid(pic)), pic.astype(np.int32)
        for row, ref in zip(g[n + "_jobs"].tolist(), g[n + "_ref"].tolist()):
            j, info = dict(zip(S.JOB_FIELDS, row[:len(S.JOB_FIELDS)])), {}
            r = S.full_search(pic, 8, table, jc, cc, pats, j, info, p32=p32)
            x = S.X(p32, 8, j, jc, cc)
            mine = [0] * len(ref)
            for p in range(S.MAX_MVSEARCH_STEPS - j["step_param"]):   # svt_av1_diamond_search_sad_c and svt_av1_get_mvpred_var, pass by pass
                sad, mv, num00 = S.diamond_search_sad(x, (j["mvp_row"], j["mvp_col"]), j["step_param"] + p, j["sad_per_bit"])
                mine[5 * p:5 * p + 5] = [sad, mv[0], mv[1], num00, S.get_mvpred_var(x, *mv)]
            mine[55:58] = [r["dia_var"], r["dia_row"], r["dia_col"]]   # full_pixel_diamond
            sad, mv, _ = S.refining_search_sad(x, (r["dia_row"], r["dia_col"]), j["sad_per_bit"], 8)
            mine[58:61] = [sad, mv[0], mv[1]]
            scans = info.get("mesh_passes", [])
            assert row[len(S.JOB_FIELDS):len(S.JOB_FIELDS) + 2] == [r["mesh_ran"], len(scans)]
            for i, (rng, step, centre, best, mv) in enumerate(scans):   # exhuastive_mesh_search, scan by scan, on the inputs the recorder was given
                assert row[len(S.JOB_FIELDS) + 2 + 4 * i:len(S.JOB_FIELDS) + 6 + 4 * i] == [rng, step, centre[0], centre[1]]
                mine[61 + 3 * i:64 + 3 * i] = [best, mv[0], mv[1]]
            if r["mesh_ran"]: mine[73:76] = [r["mesh_var"], r["mesh_row"], r["mesh_col"]]   # full_pixel_exhaustive
            mine[76:79] = [r["best_row"], r["best_col"], r["dv_valid"]]   # svt_av1_full_pixel_search's x->best_mv, av1_is_dv_valid
            assert mine == ref, (n, j, [i for i in range(len(ref)) if mine[i] != ref[i]])
            jobs_seen += 1
            shapes.add((j["block_w"], j["block_h"])); shifts.add(j["ibc_shift"])
    assert jobs_seen >= 300 and shifts == {0, 1} and shapes == set(S.SHAPES)
    assert {tuple(map(tuple, g[n + "_patterns"].tolist()))[:2] for n in names} >= {tuple(S.PATTERNS[k][:2]) for k in ("full", "two", "four", "invalid")}


def test_sad_of_every_shape_equals_the_reference(ref):
    rng = np.random.default_rng(3)
    for bw, bh in S.SHAPES:
        f = getattr(ref, "svt_aom_sad%dx%d_c" % (bw, bh)); f.restype = C.c_uint32
        for lo, hi in ((0, 256), (0, 2), (254, 256)):
            a, b = (np.ascontiguousarray(rng.integers(lo, hi, (bh + 2, bw + 5)).astype(np.uint8)) for _ in range(2))
            pic = np.concatenate([a, 255 - b if lo == 0 and hi == 2 else b])
            j = S.job(0, 0, bw, bh, (0, 5, 0, bh + 4), pic.shape[1], pic.shape[0])
            x = S.X(pic, 8, j, *H.cost_tables())
            for row, col in ((bh + 2, 0), (bh + 3, 4), (1, 3)):
                assert f(ptr(pic), pic.shape[1], ptr(pic[row:, col:]), pic.shape[1]) == x.sdf(row, col), (bw, bh, row, col)


# ------------------------------------------------------------------------------------------------------------------ the parallel scan
def test_first_strict_minimum_equals_the_two_stage_loop(runs):
    """the literal loop (sad < best, then sad + cost < best, four columns at a time) and the vectorised scan (argmin by total, then scan index, over the columns
    the shared rule says are examined) give the same value and vector, scan by scan, and visit the same vectors"""
    scans = 0
    for name in ("noise_four", "noise_deep", "tiled_zero", "planted_cols", "planted_thr", "text_four", "flat"):
        c, plane, table, jc, cc, jobs, want, infos = runs[name]
        for j, r, info in zip(jobs, want, infos):
            for rng, step, centre, best, mv in info.get("mesh_passes", []):
                x = S.X(plane, 8, j, jc, cc)
                f_ref = (j["ref_mv_row"] >> 3, j["ref_mv_col"] >> 3)
                v1, v2 = [], []
                a = S.exhuastive_mesh_search(x, f_ref, centre, rng, step, j["sad_per_bit"], v1)
                b = S.mesh_search_vectorised(x, f_ref, centre, rng, step, j["sad_per_bit"], v2)
                assert a == b == (best, mv) and v1 == v2, (name, j, rng, step, centre)
                scans += 1
    assert scans >= 100


# ------------------------------------------------------------------------------------------------------------------ what the case lists exist for
def test_the_case_lists_meet_their_conditions(runs):
    jobs = [(name, j, r, i) for name, (c, plane, table, jc, cc, js, want, infos) in runs.items() for j, r, i in zip(js, want, infos)]
    done = [t for t in jobs if t[2]["status"] == 0]
    assert {(j["block_w"], j["block_h"]) for _, j, _, _ in done} == set(S.SHAPES) and {j["ibc_shift"] for _, j, _, _ in done} == {0, 1}
    for s in range(3):
        assert sum(r["source"] == s for _, _, r, _ in done) >= 10, s
    assert sum(r["dv_valid"] for _, _, r, _ in done) >= 10 and sum(not r["dv_valid"] for _, _, r, _ in done) >= 10
    assert sum(r["mesh_ran"] for _, _, r, _ in done) >= 20
    assert sum(1 for _, j, r, _ in done if j["exhaustive_allowed"] and not r["mesh_ran"]) >= 20
    assert sum(1 for _, _, _, i in done if i["skipped"]) >= 10                       # a pass skipped through num00
    assert sum(1 for _, _, _, i in done if i["cleared"]) >= 10 and sum(1 for _, _, _, i in done if i["refined"]) >= 10
    assert sum(1 for _, _, _, i in done if i["refine_moved"]) >= 10 and sum(1 for _, _, _, i in done if i["refine_moved"] == 8) >= 1
    # an invalid first pattern: the mesh "ran" and returned INT_MAX
    inv = [r for n, _, r, _ in done if n == "text_invalid" and r["mesh_ran"]]
    assert len(inv) >= 5 and all(r["mesh_passes"] == 0 and r["mesh_var"] == S.INT_MAX and r["source"] != 1 for r in inv)
    # the threshold itself: var == thr does not run the mesh, thr + 1 does
    thr = [(r, i) for n, _, r, i in done if n == "planted_thr"]
    assert [(r["dia_var"] - i["thr"], r["mesh_ran"]) for r, i in thr[:2]] == [(0, 0), (1, 1)]
    # two equal best positions: the one row-major order meets first, which column-major order would meet second
    (r1, c1), (r2, c2) = S.TIE_COPIES
    assert r1 < r2 and c1 > c2 and thr[2][0]["mesh_ran"] and (thr[2][0]["mesh_row"], thr[2][0]["mesh_col"]) == (r1, c1) and thr[2][0]["source"] == 1
    # the last column of a step-1 scan: found only when the number of columns is a multiple of 4; the column before it always
    c, plane, table, jc, cc, js, want, infos = runs["planted_cols"]
    seen = set()
    for j, r, (n, back) in zip(js, want, S.planted_cols_layout()):
        assert j["col_max"] - j["col_min"] + 1 == n and r["mesh_ran"] and r["mesh_passes"] == 1
        copy = (-8, j["col_max"] - back)
        x = S.X(plane, 8, j, jc, cc)
        assert x.sdf(*copy) == 0 and (r["dia_row"], r["dia_col"]) != copy
        assert ((r["mesh_row"], r["mesh_col"]) == copy) == (back == 1 or n % 4 == 0), (n, back, r)
        seen.add((n % 4, back))
    assert seen == {(m, b) for m in range(4) for b in range(2)}
    # the range and each of the four limits bound a scan's window, each on its own side
    bound = set()
    for _, j, r, i in done:
        for rng, step, fc, best, mv in i.get("mesh_passes", []):
            for side, lim, sign in (("row_min", j["row_min"] - fc[0], -1), ("row_max", j["row_max"] - fc[0], 1), ("col_min", j["col_min"] - fc[1], -1),
                                    ("col_max", j["col_max"] - fc[1], 1)):
                bound.add((side, "limit" if sign * lim < rng else ("range" if sign * lim > rng else "both")))
    assert bound >= {(s, k) for s in ("row_min", "row_max", "col_min", "col_max") for k in ("limit", "range")}, bound
    # ... and on the wide strip a {256, 1} scan that the range bounds on both sides
    assert any(j["col_min"] - fc[1] < -256 and j["col_max"] - fc[1] > 256 for n, j, r, i in done if n == "strip" for rng, step, fc, best, mv in i.get("mesh_passes", []) if rng == 256)
    # progressive walks of 2, 3 and 4 scans in which every scan starts from another centre than the one before it (each scan but the last moved)
    for count in (2, 3, 4):
        assert sum(len(i.get("mesh_passes", [])) == count and all(p[4] != p[2] for p in i["mesh_passes"][:-1]) for _, _, _, i in done) >= 1, count
    # ties: a flat picture with real cost tables; all-zero cost tables
    assert sum(1 for n, _, r, _ in done if n == "flat") >= 10 and sum(1 for n, _, r, _ in done if n == "tiled_zero" and r["mesh_ran"]) >= 5
    # status 1, and -1 for each reason
    c, plane, table, jc, cc = runs["noise"][:5]
    good = next(j for j, r in zip(runs["noise"][5], runs["noise"][6]) if r["status"] == 0)
    assert [S.job_status(dict(good, **b), plane.shape[1], plane.shape[0], True) for b in S.BAD_JOBS] == [-1] * len(S.BAD_JOBS)
    assert [S.job_status(dict(good, **b), plane.shape[1], plane.shape[0], True) for b in S.EMPTY_JOBS] == [1] * len(S.EMPTY_JOBS)
    assert S.job_status(dict(good, use_hash=1), plane.shape[1], plane.shape[0], False) == -1 and S.job_status(dict(good, use_hash=0), plane.shape[1], plane.shape[0], False) == 0


def test_depth_10_decides_by_the_scaled_variance():
    """jobs at depth 10 whose value in the scaled form stays at or below the threshold while the unscaled variance of the same vector is above it"""
    c = next(c for c in S.cases() if c["name"] == "text_four")
    plane, table, jc, cc, jobs, want, infos = run_case(c, np.uint16, 10)
    hits = 0
    for j, r, i in zip(jobs, want, infos):
        if r["status"] or not j["exhaustive_allowed"] or r["mesh_ran"]: continue
        x = S.X(plane, 8, j, jc, cc)   # bd 8: the unscaled form
        hits += S.get_mvpred_var(x, r["dia_row"], r["dia_col"]) > i["thr"] >= r["dia_var"] > 0
    assert hits >= 3


# ------------------------------------------------------------------------------------------------------------------ the host form
@pytest.mark.parametrize("dtype,bd", FORMATS, ids=["u8", "u16_bd8", "u16_bd10"])
def test_host_form_equals_the_restatement(pkg, runs, dtype, bd):
    for name, (c, plane8, table8, jc, cc, _, want8, _) in runs.items():
        jobs = c["jobs"] + [dict(c["jobs"][0], **b) for b in S.BAD_JOBS + S.EMPTY_JOBS]
        if bd == 8 and dtype == np.uint8:
            plane, table = plane8, table8
            want = want8 + [S.full_search(plane, bd, table, jc, cc, c["patterns"], j) for j in jobs[len(c["jobs"]):]]
        else:
            plane, table, _, _, _, want, _ = run_case(c, dtype, bd, jobs)
        if bd == 8 and dtype == np.uint16:   # 8-bit samples in 16-bit words: other hashes, the same search
            strip = lambda r: dict(r, hash=dict(r["hash"], count=0, n_matched=0))
            assert [strip(r) for r in want[:len(c["jobs"])]] == [strip(r) for r in want8], name
        got = S.c_results(pkg.ibc_full_search_host(plane, table, jc, cc, c["patterns"], S.c_jobs(pkg, jobs), bd=bd), len(jobs))
        for i, (g, r) in enumerate(zip(got, want)):
            assert g == r, (name, i, jobs[i])
        # without a table: use_hash is a bad job; cleared, the hash stage does not apply
        sub = [dict(j, use_hash=u) for j in c["jobs"][::7] for u in (0, 1)]
        want = [S.full_search(plane, bd, None, jc, cc, c["patterns"], j) for j in sub]
        assert S.c_results(pkg.ibc_full_search_host(plane, None, jc, cc, c["patterns"], S.c_jobs(pkg, sub), bd=bd), len(sub)) == want, name


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_standalone_program(pkg, runs, flags, tmp_path):
    """csrc/ibc_search.h in a program of its own (no Python, nothing preloaded) over case files: its results, byte for byte, against what the library's host form
    gave here; every buffer it allocates has exactly the contracted size"""
    if flags:
        probe = tmp_path / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this compiler has no sanitizer runtime")
    exe = str(tmp_path / "ibc_search_host_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "ibc_search_host_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    todo = [(n, np.uint8, 8, True) for n in ("text_glyphs", "noise_open", "noise_deep", "planted_cols", "planted_thr", "ramp", "strip")]
    todo += [("text_four", np.uint16, 10, True), ("noise_four", np.uint16, 8, False)]
    for k, (name, dtype, bd, with_table) in enumerate(todo):
        c = runs[name][0]
        plane = np.ascontiguousarray(H.as_format(c["pic"], dtype, bd))
        h, w = plane.shape
        jc, cc = H.cost_tables(zero=c["zero"])
        jobs = c["jobs"] + [dict(c["jobs"][0], **b) for b in S.BAD_JOBS + S.EMPTY_JOBS]
        if not with_table: jobs = [dict(j, use_hash=0) for j in jobs]
        table = None
        if with_table:
            start, entries, info = pkg.ibc_hash_table_host(plane, bd=bd)
            table = (start, entries[:info[0]])
        tab = S.c_jobs(pkg, jobs)
        res = pkg.ibc_full_search_host(plane, table, jc, cc, c["patterns"], tab, bd=bd)
        path = str(tmp_path / ("run%d.bin" % k))
        with open(path, "wb") as f:
            f.write(np.array([plane.itemsize, bd, w, w, h, len(table[1]) if with_table else -1, len(jobs), 0], np.int32).tobytes())
            f.write(pkg.ibc_mesh_patterns(c["patterns"]).tobytes() + plane.tobytes() + jc.tobytes() + cc.tobytes() + bytes(tab)[:C.sizeof(pkg.IbcFullSearchJob) * len(jobs)])
            if with_table: f.write(table[0].tobytes() + table[1].tobytes())
            f.write(bytes(res)[:C.sizeof(pkg.IbcFullSearchResult) * len(jobs)])
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok "), (name, (r.stdout + r.stderr)[-3000:])
