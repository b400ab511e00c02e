"""CPU: the numpy restatement of the masked-compound and inter-intra searches (tests/comp_search_common.py) against the reference's recorded results and its
exported leaves, the conditions the case lists exist for, and a stand-alone sanitizer build of the library's host form.

pick_wedge, pick_interinter_seg, pick_interintra_wedge and model_rd_with_curvfit are static or need the encoder's structures, so they are pinned by
tests/golden/comp_search.npz, made the way ibc_full_search.npz was: a throw-away C program outside the repository, built against the reference with
EbEncInterPrediction.c and EbModeDecision.c included.  It filled only the structure fields those functions read (base_q_idx, y_dequant_q3 of the depth in use,
hbd_mode_decision, full_lambda_md, the block origin, the source picture, wedge_idx_fac_bits and inter_intra_mode_fac_bits), ran the C dispatch set-up and
svt_av1_init_wedge_masks, and recorded, at 8 and at 10 bits: interp_rgrid_curv, interp_dgrid_curv and bsize_curvfit_model_cat_lookup as the running reference holds
them; model_rd_with_curvfit on 4459 points of (block size, sse, quantizer, lambda); and for the 219 + 310 + 219 jobs of job_specs("wedge" | "diffwtd" |
"interintra") every candidate's (sign, sse, rate, dist, rd) from the reference's own leaves, model and RDCOST, the outputs of pick_wedge and pick_interinter_seg, the
mode loop of inter_intra_search on combine_interintra[_highbd] and model_rd_for_sb_with_curvfit, and pick_interintra_wedge's index and return value.  The file keeps
the jobs' seeds and the results only: the samples are made again here from the seeds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import comp_search_common as S
from conftest import ROOT, ptr

FORMATS = [(np.uint8, 8), (np.uint16, 8), (np.uint16, 10)]
IDS = ["u8", "u16_bd8", "u16_bd10"]


@pytest.fixture(scope="module")
def grids():
    return S.golden_grids()


@pytest.fixture(scope="module")
def mixed(grids):
    """{(format index, "real" | "synthetic"): (case, restatement results, infos)} on the list the GPU test launches, made once"""
    out = {}
    for f, (dtype, bd) in enumerate(FORMATS):
        case = S.build_case(S.job_specs("mixed"), bd, dtype)
        for name, g in (("real", grids), ("synthetic", S.synthetic_grids(grids))):
            infos = [{} for _ in case["jobs"]]
            out[f, name] = (case, S.run_case(case, g, infos), infos)
    return out


# ------------------------------------------------------------------------------------------------------------------ the recorded results
def test_restatement_equals_the_recorded_reference(grids):
    g = np.load(S.GOLDEN)
    assert os.path.getsize(S.GOLDEN) <= max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f != "comp_search.npz")
    assert g["rate_grid"].shape == (4, 65) and g["dist_grid"].shape == (2, 65) and g["bsize_cat"].shape == (22,)
    for bd in (8, 10):
        m = g["model_%d" % bd].tolist()
        assert len(m) >= 4000
        for b, q, lam, sse, rate, dist in m:
            assert S.model_rd(grids, b, sse, S.BLOCK_W[b] * S.BLOCK_H[b], q, lam) == (rate, dist), (bd, b, q, lam, sse)
        specs = [S.spec(k, b, S.STYLES[st], seed, p, q, lam) for k, b, st, seed, p, q, lam in g["specs_%d" % bd].tolist()]
        assert specs == S.job_specs("wedge") + S.job_specs("diffwtd") + S.job_specs("interintra")
        assert all(sum(s["kind"] == k for s in specs) >= 200 for k in range(3))
        got = S.run_case(S.build_case(specs, bd, np.uint16), grids)
        for k, ((r, c), row) in enumerate(zip(got, g["ref_%d" % bd].tolist())):
            mine = [v for cand in c for v in cand]
            mine += {0: [r["wedge_index"], r["wedge_sign"], 0, 0], 1: [r["mask_type"], 0, 0, 0],
                     2: [r["interintra_mode"], r["interintra_wedge_index"], r["rd_wedge"], r["rd"]]}[specs[k]["kind"]]
            assert mine == row, (bd, k, specs[k], [i for i in range(len(row)) if mine[i] != row[i]])


# ------------------------------------------------------------------------------------------------------------------ the reference's exported leaves
def test_leaves_equal_the_reference_library(ref):
    rng = np.random.default_rng(5)
    ref.svt_av1_wedge_sse_from_residuals_c.restype = C.c_uint64
    ref.svt_aom_sum_squares_i16_c.restype = C.c_uint64
    ref.svt_av1_wedge_sign_from_residuals_c.restype = C.c_int8
    ref.svt_av1_wedge_sign_from_residuals_c.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64]
    for n in (64, 128, 1024, 16384):
        for lo, hi in ((-255, 256), (-1023, 1024), (1023, 1024), (-1023, -1022)):
            a, b = (rng.integers(lo, hi, n).astype(np.int16) for _ in range(2))
            m = rng.integers(0, 65, n).astype(np.uint8)
            a64, b64, m64 = a.astype(np.int64), b.astype(np.int64), m.astype(np.int64)
            assert ref.svt_av1_wedge_sse_from_residuals_c(ptr(a), ptr(b), ptr(m), n) == S.sse_from_residuals(a64, b64, m64)
            assert ref.svt_aom_sum_squares_i16_c(ptr(a), n) == S.sum_squares(a64)
            d = np.zeros(n, np.int16)
            ref.svt_av1_wedge_compute_delta_squares_c(ptr(d), ptr(a), ptr(b), n)
            assert (d == S.delta_squares(a64, b64)).all()
            for limit in (0, int((d.astype(np.int64) * m64).sum()), int((d.astype(np.int64) * m64).sum()) - 1, -(1 << 40)):
                assert ref.svt_av1_wedge_sign_from_residuals_c(ptr(d), ptr(m), n, limit) == S.sign_from_residuals(d.astype(np.int64), m64, limit)
    ref.log2f_32.restype = C.c_uint32
    for x in [1, 2, 3, 4, 7, 8, 255, 256, 65535, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 1] + rng.integers(1, 1 << 32, 200).tolist():
        assert ref.log2f_32(C.c_uint32(x)) == S.log2f_32(x), x


def test_masks_equal_the_reference_library(ref):
    ref.svt_av1_init_wedge_masks()
    ref.av1_get_contiguous_soft_mask.restype = C.POINTER(C.c_uint8)
    table = S.wedge_table()
    assert table.size == S.TABLE_BYTES
    seen = 0
    for b in range(22):
        if b not in S.WEDGE_SIZES:
            assert S.wedge_offset(b, 0, 0) == -1
            continue
        n = S.BLOCK_W[b] * S.BLOCK_H[b]
        for sign in (0, 1):
            for w in range(16):
                o = S.wedge_offset(b, sign, w)
                assert (np.ctypeslib.as_array(ref.av1_get_contiguous_soft_mask(w, sign, b), (n,)) == table[o:o + n]).all(), (b, sign, w)
                seen += 1
        # contiguous like the reference's buffer: a size's masks follow each other, sign 0 then sign 1
        first = C.addressof(ref.av1_get_contiguous_soft_mask(0, 0, b).contents)
        assert C.addressof(ref.av1_get_contiguous_soft_mask(5, 1, b).contents) - first == S.wedge_offset(b, 1, 5) - S.wedge_offset(b, 0, 0)
    assert seen == 9 * 2 * 16
    for b in range(22):
        bw, bh = S.BLOCK_W[b], S.BLOCK_H[b]
        for mode in range(4):
            m = np.zeros(bw * bh, np.uint8)
            ref.build_smooth_interintra_mask(ptr(m), bw, b, mode)
            assert (m == S.smooth_mask(mode, b)).all(), (b, mode)


def test_blends_and_diffwtd_masks_equal_the_reference_library(ref):
    rng = np.random.default_rng(6)
    for b in S.WEDGE_SIZES:
        bw, bh = S.BLOCK_W[b], S.BLOCK_H[b]
        for mode in range(4):
            inter8, intra8 = (rng.integers(0, 256, bw * bh).astype(np.uint8) for _ in range(2))
            out8 = np.zeros(bw * bh, np.uint8)
            ref.combine_interintra(mode, 0, 0, 0, b, b, ptr(out8), bw, ptr(inter8), bw, ptr(intra8), bw)
            assert (out8 == S.blend_a64(S.smooth_mask(mode, b), intra8.astype(np.int64), inter8.astype(np.int64))).all()
            inter, intra = (rng.integers(0, 1024, bw * bh).astype(np.uint16) for _ in range(2))
            out = np.zeros(bw * bh, np.uint16)
            ref.combine_interintra_highbd(mode, 0, 0, 0, b, b, ptr(out), bw, ptr(inter), bw, ptr(intra), bw, 10)
            assert (out == S.blend_a64(S.smooth_mask(mode, b), intra.astype(np.int64), inter.astype(np.int64))).all()
    for b in (3, 9, 15, 18, 21):
        bw, bh = S.BLOCK_W[b], S.BLOCK_H[b]
        for inv in (0, 1):
            a8, b8 = (rng.integers(0, 256, bw * bh).astype(np.uint8) for _ in range(2))
            m = np.zeros(bw * bh, np.uint8)
            ref.svt_av1_build_compound_diffwtd_mask_c(ptr(m), inv, ptr(a8), bw, ptr(b8), bw, bh, bw)
            assert (m == S.diffwtd_mask(a8.astype(np.int64), b8.astype(np.int64), 8, inv)).all()
            for bd in (8, 10):
                a, c = (rng.integers(0, 1 << bd, bw * bh).astype(np.uint16) for _ in range(2))
                ref.svt_av1_build_compound_diffwtd_mask_highbd_c(ptr(m), inv, ptr(a), bw, ptr(c), bw, bh, bw, bd)
                assert (m == S.diffwtd_mask(a.astype(np.int64), c.astype(np.int64), bd, inv)).all()


# ------------------------------------------------------------------------------------------------------------------ what the case lists exist for
def test_the_case_lists_meet_their_conditions(mixed):
    for f, (dtype, bd) in enumerate(FORMATS):
        case, got, infos = mixed[f, "real"]
        jobs = case["jobs"]
        assert len(jobs) <= 300
        by_kind = lambda k: [(j, r, c, i) for j, (r, c), i in zip(jobs, got, infos) if j["kind"] == k]
        assert {j["bsize"] for j, *_ in by_kind(0)} == {j["bsize"] for j, *_ in by_kind(2)} == set(S.WEDGE_SIZES)
        assert {(S.BLOCK_W[j["bsize"]], S.BLOCK_H[j["bsize"]]) for j, *_ in by_kind(1)} == {(8, 8), (8, 32), (64, 16), (16, 64), (64, 64), (128, 128)}
        assert sum(S.BLOCK_W[j["bsize"]] == 128 for j in jobs) == 1
        # ds saturated at both ends; the int16 clamp of the sse term at 10 bits and never at 8
        assert any(i.get("ds_hi") for i in infos) and any(i.get("ds_lo") for i in infos)
        assert any(i.get("clamp") for i in infos) == (bd == 10)
        # both signs; a tie between wedge indices resolved to index 0; sse == 0 with rate 0 and dist 0
        assert {r["wedge_sign"] for _, r, _, _ in by_kind(0)} == {0, 1}
        ties = [(r, c) for _, r, c, _ in by_kind(0) if len({x[2:] for x in c[:16]}) == 1 and c[0][2] > 0]
        assert ties and all(r["wedge_index"] == 0 for r, _ in ties)
        zeros = [(j, c) for j, _, c, _ in by_kind(0) + by_kind(1) + by_kind(2) if c[0][2] == 0]   # kind 2's rate is the mode's own rate alone
        assert {j["kind"] for j, _ in zeros} == {0, 1, 2} and all(c[0][3] == 0 and c[0][1] == (case["rates"][j["mode_rate"]] if j["kind"] == 2 else 0) for j, c in zeros)
        # the skip branch taken and not; both distortion categories; the logarithm's argument 0, 1 and (10 bits: a sample difference can exceed 255) >= 2^16
        assert set().union(*[i.get("skips", set()) for i in infos]) == {False, True}
        assert set().union(*[i.get("dcats", set()) for i in infos]) == {0, 1}
        args = set().union(*[i.get("log_args", set()) for i in infos])
        cols = set().union(*[i.get("cols", set()) for i in infos])
        assert {0, 1} <= args and (max(args) >= 1 << 16) == (bd == 10) and (62 in cols) == (bd == 10) and 31 in cols and cols <= set(range(31, 62, 2)) | {62}
        # rate_i == 0: never with the recorded grids (their columns from 31 on are positive), taken with the caller's grids cleared there
        assert not any(i.get("rate0") for i in infos) and any(i.get("rate0") for i in mixed[f, "synthetic"][2])
        assert mixed[f, "synthetic"][1] != got
        # every inter-intra mode and at least 12 of the 16 wedge indices win somewhere
        assert {r["interintra_mode"] for _, r, _, _ in by_kind(2)} == {0, 1, 2, 3}
        assert len({r["wedge_index"] for _, r, _, _ in by_kind(0)} | {r["interintra_wedge_index"] for _, r, _, _ in by_kind(2)}) >= 12
        assert {r["mask_type"] for _, r, _, _ in by_kind(1)} == {0, 1}
        # a block in each corner of a plane whose stride is no multiple of 64
        h, w = case["plane"].shape
        stride = case["plane"].strides[0] // case["plane"].itemsize
        assert stride % 64 and stride > w
        corners = {(j["x"] == 0, j["y"] == 0) for j in jobs if j["x"] in (0, w - S.BLOCK_W[j["bsize"]]) and j["y"] in (0, h - S.BLOCK_H[j["bsize"]])}
        assert len(corners) == 4
        assert all(S.job_ok(j, w, h, case["pool"].size, case["rates"].size) for j in jobs)


def test_depth_8_in_16_bit_words_is_depth_8(mixed):
    assert mixed[0, "real"][1] == mixed[1, "real"][1] and mixed[0, "real"][1] != mixed[2, "real"][1]


# ------------------------------------------------------------------------------------------------------------------ the stand-alone program
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_standalone_program(pkg, grids, mixed, flags, tmp_path):
    """csrc/comp_search.h in a program of its own (no Python, nothing preloaded) over case files: the table and every result and candidate record, byte for byte,
    against what the library's host form gave here; every buffer it allocates has exactly the contracted size"""
    if flags:
        probe = tmp_path / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this compiler has no sanitizer runtime")
    exe = str(tmp_path / "comp_search_host_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", *flags, os.path.join(ROOT, "tests", "comp_search_host_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    table = pkg.wedge_masks_host()
    for k, (f, name) in enumerate(((0, "real"), (2, "real"), (1, "synthetic"), (2, "synthetic"))):
        case = mixed[f, name][0]
        g = pkg.rd_curvfit_grids(grids if name == "real" else S.synthetic_grids(grids))
        plane = case["plane"]
        store = plane.base
        jobs = S.c_jobs(pkg, case["jobs"])
        n = len(case["jobs"])
        res, cand = pkg.compound_search_host(g, plane, case["pool"], case["rates"], jobs, bd=case["bd"])
        path = str(tmp_path / ("run%d.bin" % k))
        with open(path, "wb") as fh:
            fh.write(np.array([plane.itemsize, case["bd"], store.shape[1], plane.shape[1], plane.shape[0], case["pool"].size, case["rates"].size, n], np.int32).tobytes())
            fh.write(g[0].tobytes() + g[1].tobytes() + g[2].tobytes() + store.tobytes() + case["pool"].tobytes() + case["rates"].tobytes())
            fh.write(bytes(jobs)[:C.sizeof(pkg.CompSearchJob) * n] + table.tobytes() + bytes(res)[:C.sizeof(pkg.CompSearchResult) * n])
            fh.write(bytes(cand)[:C.sizeof(pkg.CompSearchCand) * S.MAX_CANDS * n])
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok %d jobs" % n), (f, name, (r.stdout + r.stderr)[-3000:])
