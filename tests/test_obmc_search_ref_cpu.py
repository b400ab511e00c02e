"""CPU: the numpy restatement of OBMC in mode decision (tests/obmc_common.py) against the reference's recorded results and its exported leaves, the conditions the
case lists exist for, and a stand-alone sanitizer build of the library's host forms.

calc_target_weighted_pred, the two foreach_overlappable_nb_*, obmc_refining_search_sad, svt_av1_obmc_full_pixel_search and
svt_av1_find_best_obmc_sub_pixel_tree_up are static or take the encoder's contexts, so they are pinned by tests/golden/obmc_search.npz, made the way
ibc_full_search.npz and comp_search.npz were: a throw-away C program outside the repository, built against the reference with EbEncInterPrediction.c and av1me.c
included.  It filled only the structure fields those functions read (the mi grid's sb_type and ref_frame[0] around the block, up / left_available, n4_w, n4_h,
mi_rows, mi_cols, the source picture, blk_geom->bsize, the block origin; wsrc_buf, mask_buf, xdplane[0].pre[0], mv_limits, nmv_vec_cost, mv_cost_stack, errorperbit),
ran the C dispatch set-up and init_fn_ptr, and recorded: per target job of both target lists the wsrc and mask arrays calc_target_weighted_pred left (the
neighbour lists came from its own foreach_overlappable_nb_* on the sb_type / ref_frame grid, so they are pinned with them); per search job of both search lists
the vector and value of obmc_refining_search_sad and its number of moves (the smallest search_range at which it ends at the same vector), the vector and
return value of svt_av1_obmc_full_pixel_search, and the vector, return value, distortion and sse1 of svt_av1_find_best_obmc_sub_pixel_tree_up, with
svt_av1_mv_bit_cost of the final vector.  The file keeps the jobs, CRCs of the samples and the results only: the samples are made again here from their seeds."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import obmc_common as S
from conftest import ROOT, ptr

WHICH = ["small", "big"]


# ------------------------------------------------------------------------------------------------------------------ the recorded results
def test_restatement_equals_the_recorded_reference():
    g = np.load(S.GOLDEN)
    golden_dir = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(S.GOLDEN) <= max(os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir) if f != "obmc_search.npz")
    for which in WHICH:
        case, (wsrc, mask), _ = S.cached("target", which)
        search, want, _ = S.cached("search", which)
        assert g["inputs_%s_crc" % which].tolist() == S.input_crcs(which)
        assert g["target_%s_jobs" % which].tolist() == [S.flat_target_job(j) for j in case["jobs"]]
        assert g["search_%s_jobs" % which].tolist() == [[j[f] for f in S.JOB_FIELDS] for j in search["jobs"]]
        assert (g["target_%s_wsrc" % which] == wsrc).all() and (g["target_%s_mask" % which] == mask).all() and wsrc.size == case["wm_samples"] > 90000
        rows = g["search_%s" % which].tolist()
        assert len(rows) == len(want)
        for k, (row, mine) in enumerate(zip(rows, want)):
            assert row[0] == mine["status"], (which, k)   # 1: the recorder saw the narrowed limits empty too, and did not call the reference there
            if mine["status"] == 0:
                assert row == [S.to_int(mine[f]) for f in S.RESULT_FIELDS], (which, k, search["specs"][k])
    assert sum(len(S.cached("search", w)[1]) for w in WHICH) >= 300 and sum(len(S.cached("target", w)[0]["jobs"]) for w in WHICH) >= 200


# ------------------------------------------------------------------------------------------------------------------ the reference's exported leaves
def test_leaves_equal_the_reference_library(ref):
    rng = np.random.default_rng(9)
    ref.svt_av1_get_obmc_mask.restype = C.POINTER(C.c_uint8)
    for n, table in S.OBMC_MASK.items():
        assert ref.svt_av1_get_obmc_mask(n)[:n] == table
    plane = rng.integers(0, 256, (160, 176)).astype(np.uint8)
    for b in S.SIZES:
        bw, bh = S.BLOCK_W[b], S.BLOCK_H[b]
        sad_fn, var_fn = getattr(ref, "svt_aom_obmc_sad%dx%d_c" % (bw, bh)), getattr(ref, "svt_aom_obmc_variance%dx%d_c" % (bw, bh))
        sad_fn.restype = var_fn.restype = C.c_uint32
        for style in range(3):
            # the ranges calc_target_weighted_pred produces, and their extremes (a sum of differences of one sign: the sum * sum term at its largest)
            mask = rng.integers(0, 4097, (bh, bw)).astype(np.int32) if style < 2 else np.full((bh, bw), 4096, np.int32)
            wsrc = (rng.integers(0, 256 * 4096, (bh, bw)) if style == 0 else np.full((bh, bw), 255 * 4096) if style == 1 else np.zeros((bh, bw))).astype(np.int32)
            pre = plane[8:8 + bh, 16:16 + bw]
            at = plane[8:, 16:]
            assert sad_fn(ptr(at), plane.shape[1], ptr(wsrc), ptr(mask)) == S.obmc_sad(pre, wsrc, mask)
            sse = C.c_uint32()
            var = var_fn(ptr(at), plane.shape[1], ptr(wsrc), ptr(mask), C.byref(sse))
            assert (var, sse.value) == S.obmc_variance(pre, wsrc, mask), (b, style)
        for sx, sy in [(0, 0), (3, 0), (0, 5), (1, 7), (4, 4), (7, 1), (6, 2)] + ([(x, y) for x in range(8) for y in range(8)] if b == S.BSIZE_OF[16, 16] else []):
            out = np.zeros((bh, bw), np.uint8)
            src = plane[12:, 20:]   # room for the filter's -3 .. +4
            ref.svt_aom_upsampled_pred_c(None, None, 0, 0, None, ptr(out), bw, bh, sx, sy, ptr(src), plane.shape[1], 3)   # USE_8_TAPS
            assert (out == S.upsampled_pred(plane, 12, 20, bw, bh, sx, sy)).all(), (b, sx, sy)
    # saturating content: the horizontal pass clips before the vertical one filters
    hard = (rng.integers(0, 2, (64, 64)) * 255).astype(np.uint8)
    out = np.zeros((16, 16), np.uint8)
    for sx, sy in ((4, 4), (1, 3), (7, 7), (2, 0), (0, 6)):
        ref.svt_aom_upsampled_pred_c(None, None, 0, 0, None, ptr(out), 16, 16, sx, sy, ptr(hard[8:, 8:]), 64, 3)
        assert (out == S.upsampled_pred(hard, 8, 8, 16, 16, sx, sy)).all()
    jc, cc = S.cost_tables()
    jc32, cc32 = np.ascontiguousarray(jc, np.int32), np.ascontiguousarray(cc, np.int32)
    stack = (C.c_void_p * 2)(cc32.ctypes.data + 4 * S.MV_MAX, cc32.ctypes.data + 4 * (S.MV_VALS + S.MV_MAX))
    ref.svt_av1_mv_bit_cost.restype = C.c_int32
    for _ in range(300):
        r, c, rr, rc = (int(v) for v in rng.integers(-8000, 8001, 4))
        mv, rmv = (C.c_int16 * 2)(r, c), (C.c_int16 * 2)(rr, rc)
        assert ref.svt_av1_mv_bit_cost(mv, rmv, ptr(jc32), stack, 108) == S.mv_bit_cost(r, c, rr, rc, jc, cc), (r, c, rr, rc)


# ------------------------------------------------------------------------------------------------------------------ what the case lists contain
def test_target_lists_contain_what_they_exist_for():
    small, big = S.cached("target", "small")[0], S.cached("target", "big")[0]
    jobs = small["jobs"] + big["jobs"]
    assert {j["bsize"] for j in jobs} == set(S.SIZES) and len(S.SIZES) == 17
    assert {j["bsize"] for j in small["jobs"]} == set(S.SMALL_SIZES) and {j["bsize"] for j in big["jobs"]} == set(S.BIG_SIZES) and len(S.BIG_SIZES) == 3
    assert any(j["n_above"] == 0 for j in jobs) and any(j["n_left"] == 0 for j in jobs) and any(j["n_above"] == 0 and j["n_left"] == 0 for j in jobs)
    for side in ("above", "left"):
        assert {j["n_" + side] for j in jobs} == {0, 1, 2, 3, 4}
        # a gap: two segments of a side that do not touch
        assert any(j[side + "_rel"][i] + j[side + "_len"][i] < j[side + "_rel"][i + 1] for j in jobs for i in range(j["n_" + side] - 1))
    rows = list(zip(small["specs"] + big["specs"], jobs, small["segs"] + big["segs"]))
    # a 4-wide neighbour pair: the odd unit's flag decides for both
    assert any(a and 1 in a[0] and sa for _, _, (sa, sl, a, l) in rows) and any(l and 1 in l[0] and sl for _, _, (sa, sl, a, l) in rows)
    pair = S.neighbours([1, 1, 1, 1], [1, 0, 0, 1], 4, 6, 100)
    assert pair == [(2, 2)]   # units 0, 1: the odd one says no; units 2, 3: the odd one says yes, the segment starts at the even one
    # a list cut by nb_max: more overlappable neighbours along the edge than max_neighbor_obmc allows
    cut = 0
    for spec, j, (sa, sl, a, l) in rows:
        for segs, lay, n4, pos, end in ((sa, a, S.BLOCK_W[j["bsize"]] // 4, j["x"] // 4, spec["mi_cols"]), (sl, l, S.BLOCK_H[j["bsize"]] // 4, j["y"] // 4, spec["mi_rows"])):
            if lay and segs and segs[-1][0] + segs[-1][1] < min(n4, end - pos) and any(lay[1][segs[-1][0] + segs[-1][1]:min(n4, end - pos)]):
                assert len(segs) == S.MAX_NEIGHBOR_OBMC[n4.bit_length() - 1]
                cut += 1
    assert cut >= 4
    # the picture's last column / row inside the block: the segments end there
    assert any(s["mi_cols"] * 4 < j["x"] + S.BLOCK_W[j["bsize"]] and sa and (sa[-1][0]) * 4 + j["x"] < s["mi_cols"] * 4 for s, j, (sa, sl, a, l) in rows)
    assert any(s["mi_rows"] * 4 < j["y"] + S.BLOCK_H[j["bsize"]] and sl for s, j, (sa, sl, a, l) in rows)
    assert S.neighbours([2] * 8, [1] * 8, 8, 16, 19) == [(0, 2), (2, 2)]   # units 16 .. 18 of 19: the third neighbour starts inside the picture too, but nb_max = 3 ...
    assert S.neighbours([2] * 8, [1] * 8, 8, 16, 18) == [(0, 2)]
    # 128 wide: the overlap is capped at 32 rows / columns and a neighbour's step at 16 units
    for j, (sa, sl, a, l) in zip(big["jobs"], big["segs"]):
        assert all(n <= 16 for _, n in sa + sl)
    assert any(S.BLOCK_W[j["bsize"]] == 128 and j["n_above"] for j in big["jobs"]) and any(S.BLOCK_H[j["bsize"]] == 128 and j["n_left"] for j in big["jobs"])
    assert S.neighbours([32] * 32, [1] * 32, 32, 0, 100) == [(0, 16), (16, 16)]
    _, (wsrc, mask), _ = S.cached("target", "big")
    j = next(j for j in big["jobs"] if j["bsize"] == S.BSIZE_OF[128, 128] and j["n_above"] and j["n_left"])
    m = mask[j["wm_off"]:j["wm_off"] + 128 * 128].reshape(128, 128)
    assert (m[32:, 32:] == 4096).all() and (m[:32, :32] < 4096).any()


def test_search_lists_contain_what_they_exist_for():
    case, want, infos = S.cached("search", "small")
    big_case, big_want, _ = S.cached("search", "big")
    assert {j["bsize"] for j in case["jobs"]} == set(S.SMALL_SIZES) and {j["bsize"] for j in big_case["jobs"]} == set(S.BIG_SIZES)
    named = {S.BSIZE_OF[8, 8], S.BSIZE_OF[8, 32], S.BSIZE_OF[32, 8], S.BSIZE_OF[16, 16]}
    done = [(j, r, i) for j, r, i in zip(case["jobs"], want, infos) if r["status"] == 0]
    assert any(r["status"] == 1 for r in want) and all(r["status"] == 0 for r in big_want)
    for b in named:   # every condition on each of the four shapes
        mine = [(r, i) for j, r, i in done if j["bsize"] == b]
        # the refinement
        assert any(r["steps"] == 0 for r, _ in mine) and any(r["steps"] == 8 for r, _ in mine)
        assert {s for _, i in mine for s in i["sites"]} == {0, 1, 2, 3}
        assert any(i["excluded"] for _, i in mine) and any(i["clamped"] for _, i in mine)
        assert any(i["cost_rejects"] for _, i in mine)   # passed `sad < best`, failed with the cost added
        assert any(i["ties"] for _, i in mine)           # an equal value is not taken
        # the sub-pel tree
        assert {len(i["best_idx"]) for _, i in mine} == {2, 3}
        assert {v for _, i in mine for v in i["best_idx"]} == {-1, 0, 1, 2, 3, 4}
        assert {v for _, i in mine for v in i["third"]} == {True, False}
        assert any(i["out_axis"] for _, i in mine) and any(i["out_diag"] for _, i in mine) and any(i["out_second"] for _, i in mine)
        assert {v for _, i in mine for v in i["rewrites"]} == {"kr", "kc"}
    hp = {j["allow_hp"]: 0 for j, _, _ in done}
    assert set(hp) == {0, 1}
    # a probe that costs more than INT_MAX as an unsigned value: the unsigned / int mix decides there
    assert any(r["besterr"] > S.INT_MAX for r in want) or any(i["out_diag"] for i in infos if i)
    # every job's window lies inside the border the case gives it, derived from the limits; the tightest job needs all but a few samples of it
    for c in (case, big_case):
        for j in c["jobs"]:
            lim = S.search_range(S.block_limits(j, c["mi_rows"], c["mi_cols"]), j["ref_mv_row"], j["ref_mv_col"])
            if lim[0] <= lim[1] and lim[2] <= lim[3]:
                assert S.plane_covers(j, lim, c["width"], c["height"], c["pad_w"], c["pad_h"])
        need = max(max(S.BLOCK_W[j["bsize"]], S.BLOCK_H[j["bsize"]]) for j in c["jobs"]) + 9
        assert need <= c["pad_w"] < need + 8


# ------------------------------------------------------------------------------------------------------------------ the stand-alone program
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def case_file(pkg, path, which):
    """both stages of a search case for tests/obmc_search_host_test.cpp, the border cut to exactly what the largest block needs, with what the library's host forms
    make of it"""
    c, _, _ = S.cached("search", which)
    t = c["target"]
    need = max(max(S.BLOCK_W[j["bsize"]], S.BLOCK_H[j["bsize"]]) for j in c["jobs"]) + 9
    cut = c["pad_w"] - need
    padded = np.ascontiguousarray(c["padded"][cut:c["padded"].shape[0] - cut, cut:c["padded"].shape[1] - cut])
    picture = padded[need:need + c["height"], need:need + c["width"]]
    tj, sj = S.c_target_jobs(pkg, t["jobs"]), S.c_search_jobs(pkg, c["jobs"])
    wsrc, mask = pkg.obmc_target_host(t["plane"], t["nbr"], tj, t["wm_samples"])
    res = pkg.obmc_search_host(picture, need, need, c["mi_rows"], c["mi_cols"], wsrc, mask, c["jc"], c["cc"], sj)
    with open(path, "wb") as f:
        f.write(struct.pack("16i", t["plane"].shape[1], t["plane"].shape[1], t["plane"].shape[0], t["nbr"].size, t["wm_samples"], len(c["jobs"]), padded.shape[1],
                            c["width"], c["height"], need, need, c["mi_rows"], c["mi_cols"], 0, 0, 0))
        for part in (np.ascontiguousarray(t["plane"]), t["nbr"], bytes(tj), padded, np.ascontiguousarray(c["jc"], np.int32), np.ascontiguousarray(c["cc"], np.int32), bytes(sj),
                     wsrc, mask, bytes(res)):
            f.write(part if isinstance(part, bytes) else part.tobytes())
    return len(c["jobs"])


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_standalone_program(pkg, flags, tmp_path):
    """csrc/obmc_search.h in a program of its own (no Python, nothing preloaded) over both case lists: its arrays and results, byte for byte, against what the
    library's host forms gave here; every buffer it allocates has exactly the contracted size"""
    if flags:
        probe = tmp_path / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this compiler has no sanitizer runtime")
    exe = str(tmp_path / "obmc_search_host_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "obmc_search_host_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    for which in WHICH:
        path = str(tmp_path / (which + ".bin"))
        n = case_file(pkg, path, which)
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok %d jobs" % n), (which, r.returncode, r.stdout[-500:], r.stderr[-3000:])
