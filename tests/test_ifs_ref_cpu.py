"""CPU: the numpy restatement of the dual interpolation filter search (tests/ifs_common.py) against the reference's exported leaves on the very lists the GPU test
launches, the conditions those lists exist for, the library's host form, a stand-alone sanitizer build of it, and the refusals.

interpolation_filter_search itself takes the encoder's picture, context and candidate structures, so it is pinned by tests/golden/ifs_search.npz, made the way
obmc_search.npz was: a throw-away C program outside the repository, built against the reference with EbEncInterPrediction.c compiled in and one line added after each
`tmp_rd = RDCOST(...)` that notes the loop index and the value.  It filled only what the function and its callees read -- the sequence header's enable_dual_filter and
order hints, y_dequant_q3 of the depth in use, full_lambda_md, interpolation_search_level, the block's geometry and edges, zeroed neighbour arrays (no neighbour: both
contexts end in SWITCHABLE_FILTERS), switchable_interp_fac_bitss, the candidate's vectors, reference types and compound type, the source, the two reference pictures and
the prediction buffer -- ran the C dispatch set-up and called the function once per call, at 8 and at 10 bits, on 166 jobs of this file's list (every block of at most
512 samples, six of 1024, 64x64 with one and two references, 128x128) with the phases made even, as a luma vector in eighths of a sample makes them.  Recorded per call:
the block, the phases, both reference windows, the source block, the six rates, lambda, the quantizer, the branch, for COMPOUND_DISTANCE the offsets
svt_av1_dist_wtd_comp_weight_assign gave; and interp_filters, what was added to fast_luma_rate, ifs_is_regular_last and every (i, tmp_rd) in evaluation order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ifs_common as S
from conftest import ROOT, ptr
from percall_common import CONV, CONVH, ConvParams, FilterParams, as_proto

FORMATS = [(np.uint8, 8), (np.uint16, 8), (np.uint16, 10)]
IDS = ["u8", "u16_bd8", "u16_bd10"]
REF_TAPS = ["sub_pel_filters_8", "sub_pel_filters_8smooth", "sub_pel_filters_8sharp"]   # EIGHTTAP_REGULAR, EIGHTTAP_SMOOTH, MULTITAP_SHARP
SPDIST = C.CFUNCTYPE(C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32)
BRANCH = {(0, 0): "2d_copy", (1, 0): "x", (0, 1): "y", (1, 1): "2d"}   # convolve[subpel_x != 0][subpel_y != 0]


@pytest.fixture(scope="module")
def cases():
    """{format index: (case, restatement results, infos)} on the list the GPU test launches, made once"""
    out = {}
    for f, (dtype, bd) in enumerate(FORMATS):
        case = S.build_case(bd, dtype)
        infos = [{} for _ in case["jobs"]]
        out[f] = (case, S.run_case(case, infos), infos)
    return out


# ------------------------------------------------------------------------------------------------------------------ the recorded results
def test_restatement_equals_the_recorded_reference():
    assert os.path.getsize(S.GOLDEN) <= max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f != "ifs_search.npz")
    seen = set()
    for bd in (8, 10):
        calls = S.golden_calls(bd)
        assert len(calls) >= 150
        for k, (case, (filters, rate, last, evals)) in enumerate(calls):
            j = case["jobs"][0]
            res, cands, _ = S.run_job(case, j)
            assert (res[1], res[2]) == (filters, rate), (bd, k, j)
            assert last == (res[3] if j["order"] == 1 else 7), (bd, k, j)   # 7: the value put there before the call, left alone by the first branch
            if j["order"] == 0:
                # all nine ascending, then the second loop from the winner of the first: pairs seen before, the same values, and no change of the result
                again = list(range(res[0] + 3, 9, 3))
                assert [i for i, _ in evals] == list(range(9)) + again, (bd, k)
                assert all(cands[i][3] >= res[4] for i in again)
                seen.add(("second loop", len(again)))
            else:
                assert [i for i, _ in evals] == [i for i in range(8, -1, -1) if S.evaluated(j, i)], (bd, k)
            assert [rd for _, rd in evals] == [cands[i][3] for i, _ in evals], (bd, k, j)
            assert res[4] == min(rd for _, rd in evals)
            seen |= {("order", j["order"], j["dual"]), ("type", j["type"]), ("best", j["order"], res[0]), ("bsize", j["bsize"])}
            if j["order"] == 1 and len({rd for _, rd in evals}) < len(evals) and res[0] != min(i for i, rd in evals if rd == res[4]):
                seen.add("a tie that the descending walk gives to the higher index")
            if j["order"] == 0 and [rd for _, rd in evals[:9]].count(res[4]) > 1:
                seen.add("a tie that the ascending walk gives to the lower index")
    assert {("order", 0, 1), ("order", 1, 0), ("order", 1, 1), ("type", -1), ("type", 0), ("type", 1)} <= seen
    assert {("best", 0, i) for i in range(9)} <= seen and {("best", 1, i) for i in (0, 4, 8)} <= seen
    assert {("second loop", n) for n in (0, 1, 2)} <= seen and {("bsize", b) for b in (3, 6, 9, 12, 15)} <= seen
    assert "a tie that the descending walk gives to the higher index" in seen and "a tie that the ascending walk gives to the lower index" in seen


# ------------------------------------------------------------------------------------------------------------------ the reference's exported leaves
def _leaf_predict(ref, case, j, i):
    """the luma prediction of job j under pair i from the reference's own convolve functions"""
    bw, bh, bd = S.BLOCK_W[j["bsize"]], S.BLOCK_H[j["bsize"]], case["bd"]
    dtype, pb = case["src"].dtype, case["src"].itemsize
    fy, fx = S.FILTER_SETS[i]
    px = FilterParams(C.addressof(C.c_int16.in_dll(ref, REF_TAPS[fx])), 8, 16, fx)
    py = FilterParams(C.addressof(C.c_int16.in_dll(ref, REF_TAPS[fy])), 8, 16, fy)
    out, buf = np.zeros((bh, bw), dtype), np.zeros((bh, bw), np.uint16)
    nrefs = 1 if j["type"] < 0 else 2
    for r in range(nrefs):
        a = case["ref"][r]
        sx, sy = j["subpel%d_x" % r], j["subpel%d_y" % r]
        name = BRANCH[int(sx != 0), int(sy != 0)]
        if nrefs == 1:
            fn = as_proto(CONV, getattr(ref, "svt_av1_convolve_%s_sr_c" % name)) if pb == 1 else as_proto(CONVH, getattr(ref, "svt_av1_highbd_convolve_%s_sr_c" % name))
            cp = ConvParams(0, 0, None, 0, 3, 11, 0, 0, 0, 0, 0, 0)   # get_conv_params(0, 0, 0, bd)
        else:
            fn = as_proto(CONV, getattr(ref, "svt_av1_jnt_convolve_%s_c" % name)) if pb == 1 else as_proto(CONVH, getattr(ref, "svt_av1_highbd_jnt_convolve_%s_c" % name))
            cp = ConvParams(0, r, buf.ctypes.data, bw, 3, 7, 0, 1, j["type"], j["fwd_offset"], j["bck_offset"], j["type"])   # get_conv_params_no_round
        at = a.ctypes.data + ((j["ref%d_y" % r] + S.REACH_LO) * a.shape[1] + j["ref%d_x" % r] + S.REACH_LO) * pb
        fn(at, a.shape[1], out.ctypes.data, bw, bw, bh, C.byref(px), C.byref(py), sx, sy, C.byref(cp), *((bd,) if pb == 2 else ()))
    return out


@pytest.mark.parametrize("f", range(3), ids=IDS)
def test_restatement_equals_the_reference_leaves_on_the_lists(ref, cases, f):
    """every candidate of every job: the prediction from svt_av1_[highbd_]convolve_*_sr_c / svt_av1_[highbd_]jnt_convolve_*_c, the sse from
    svt_spatial_full_distortion_kernel_c / svt_full_distortion_kernel16_bits_c, rate and dist from model_rd_from_sse"""
    case, got, _ = cases[f]
    bd, src = case["bd"], case["src"]
    stride = src.strides[0] // src.itemsize
    dist_fn = as_proto(SPDIST, ref.svt_spatial_full_distortion_kernel_c if src.itemsize == 1 else ref.svt_full_distortion_kernel16_bits_c)
    ref.model_rd_from_sse.argtypes = [C.c_int, C.c_int16, C.c_uint8, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_uint8]
    ref.model_rd_from_sse.restype = None
    for k, (j, (res, cands, best_pred)) in enumerate(zip(case["jobs"], got)):
        bw, bh = S.BLOCK_W[j["bsize"]], S.BLOCK_H[j["bsize"]]
        for i, (fy, fx) in enumerate(S.FILTER_SETS):
            if not S.evaluated(j, i):
                assert cands[i] == (-1, 0, 0, 0)
                continue
            pred = _leaf_predict(ref, case, j, i)
            assert np.array_equal(pred, S.predict(case, j, i)), (k, j, i)
            sse = dist_fn(ptr(src), j["y"] * stride + j["x"], stride, ptr(pred), 0, bw, bw, bh)
            rate, dist = C.c_uint32(), C.c_uint64()
            ref.model_rd_from_sse(j["bsize"], j["quantizer"], bd, (sse + ((1 << (2 * (bd - 8))) >> 1)) >> (2 * (bd - 8)), C.byref(rate), C.byref(dist), 0)
            rs = j["rate_tab"][0][fy] + j["rate_tab"][1][fx]
            assert (rate.value + rs, sse, dist.value) == cands[i][:3], (k, j, i)
            assert cands[i][3] == S.rdcost(j["full_lambda"], rate.value + rs, dist.value)
            if i == res[0]:
                assert np.array_equal(pred, best_pred)


def test_model_equals_the_reference_on_every_segment_boundary(ref):
    ref.svt_av1_model_rd_from_var_lapndz.argtypes = [C.c_int64, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    ref.svt_av1_model_rd_from_var_lapndz.restype = None
    rng = np.random.default_rng(9)
    points = S.model_points() + [(int(rng.integers(1, 1 << int(rng.integers(1, 36)))), int(rng.integers(6, 15)), int(rng.integers(0, 4096))) for _ in range(3000)]
    for var, n_log2, qstep in points:
        rate, dist = C.c_int32(), C.c_int64()
        ref.svt_av1_model_rd_from_var_lapndz(var, n_log2, qstep, C.byref(rate), C.byref(dist))
        assert (rate.value, dist.value) == S.model_lapndz(var, n_log2, qstep), (var, n_log2, qstep)


def test_the_model_points_touch_every_segment_boundary():
    hit = {S.model_xsq(v, n, q)[0] for v, n, q in S.model_points() if v}
    assert ({x for x in S.XSQ_IQ_Q10} | {x - 1 for x in S.XSQ_IQ_Q10[1:]}) - {S.MAX_XSQ_Q10 + 1} <= hit and S.MAX_XSQ_Q10 in hit
    assert {S.model_xq(x)[0] for x in hit} == set(range(103))
    assert any(S.model_xsq(v, n, q)[1] for v, n, q in S.model_points() if v) and any(v == 0 for v, _, _ in S.model_points())


# ------------------------------------------------------------------------------------------------------------------ what the job list exists for
def test_the_job_list_meets_its_conditions(cases):
    for f, (dtype, bd) in enumerate(FORMATS):
        case, got, infos = cases[f]
        jobs = case["jobs"]
        assert 150 <= len(jobs) <= 400 and case["src"].shape == (S.H, S.W) and all(S.job_ok(j) for j in jobs)
        stride = case["src"].strides[0] // case["src"].itemsize
        assert stride % 64 and stride > S.W and all(a.shape == (S.H + 7, S.W + 7) for a in case["ref"])
        single = [(j, r, c, i) for j, (r, c, _), i in zip(jobs, got, infos) if j["type"] < 0]
        double = [(j, r, c, i) for j, (r, c, _), i in zip(jobs, got, infos) if j["type"] >= 0]
        # each of the 17 shapes, with one and with two references; the four branches for one reference and for each reference of two
        assert {j["bsize"] for j, *_ in single} == {j["bsize"] for j, *_ in double} == set(S.SIZES) and len(S.SIZES) == 17
        assert set().union(*[i["branches"] for i in infos]) == {(n, b) for n in (1, 2, 3) for b in range(4)}
        assert {j["type"] for j in jobs} == {-1, 0, 1}
        # each pair winning under order 0; each equal-filter pair under order 1 without dual filters, where no other pair is evaluated
        assert {r[0] for j, (r, _, _) in zip(jobs, got) if j["order"] == 0} == set(range(9))
        nodual = [(j, r, c) for j, (r, c, _) in zip(jobs, got) if j["order"] == 1 and not j["dual"]]
        assert {r[0] for _, r, _ in nodual} == {0, 4, 8} and all([x[0] >= 0 for x in c] == [i in (0, 4, 8) for i in range(9)] for _, _, c in nodual)
        assert {r[3] for j, (r, _, _) in zip(jobs, got) if j["order"] == 1} == {0, 1} and {r[3] for j, (r, _, _) in zip(jobs, got) if j["order"] == 0} == {-1}
        # the two orders on one job
        key = lambda j: tuple(sorted((k, str(v)) for k, v in j.items() if k not in ("order", "dst_x", "dst_y", "page")))
        twins = {}
        for j, (r, c, _) in zip(jobs, got):
            twins.setdefault(key(j), {})[j["order"]] = (j, r, c)
        twins = [t for t in twins.values() if len(t) == 2]
        assert any(t[0][1][0] != t[1][1][0] for t in twins)
        whole = [t for t in twins if not any(t[0][0]["subpel0_" + a] for a in "xy")]
        for t in whole:
            assert len({c[1] for c in t[0][2]}) == 1 and t[0][2][0][1] > 0   # all nine sse equal
        decided = [t for t in whole if len({c[0] for c in t[0][2]}) == 9]
        assert decided and all(t[0][1][0] == t[1][1][0] == min(range(9), key=lambda i: t[0][2][i][3]) for t in decided)
        equal = [t for t in whole if len({c[0] for c in t[0][2]}) == 1]
        assert equal and all((t[0][1][0], t[1][1][0]) == (0, 8) for t in equal)
        # sse == 0: rate is the two symbols alone, dist 0
        zeros = [(j, c) for j, (_, c, _) in zip(jobs, got) if c[0][1] == 0]
        assert {j["type"] for j, _ in zeros} == {-1, 0, 1} and all(c[0][2] == 0 and c[0][0] == j["rate_tab"][0][0] + j["rate_tab"][1][0] for j, c in zeros)
        # the clamp of the abscissa reached and not; the quantizer's ends; weights from at least three rows of quant_dist_lookup_table
        assert set().union(*[i.get("clamp", set()) for i in infos]) == {False, True}
        assert {1, 32767} <= {j["quantizer"] for j in jobs}
        assert len({tuple(sorted((j["fwd_offset"], j["bck_offset"]))) for j in jobs if j["type"] == 1} & {tuple(sorted(w)) for w in S.QUANT_DIST}) >= 3
        # the whole border at each picture edge, with both phases so that every sample of the window is read; the shapes that need strips among them
        for edge in (lambda j, bw, bh: j["ref0_x"] == 0, lambda j, bw, bh: j["ref0_y"] == 0, lambda j, bw, bh: j["ref0_x"] == S.W - bw, lambda j, bw, bh: j["ref0_y"] == S.H - bh):
            assert any(edge(j, S.BLOCK_W[j["bsize"]], S.BLOCK_H[j["bsize"]]) and j["subpel0_x"] and j["subpel0_y"] for j in jobs)
        for b in (15, 13):
            assert any(j["bsize"] == b and j["type"] < 0 for j in jobs) and any(j["bsize"] == b and j["type"] >= 0 for j in jobs)
        # samples at 0 and at the top value inside one window
        top = (1 << bd) - 1
        assert any((lambda w: w.min() == 0 and w.max() == top)(S.window(case, 0, j)) for j in jobs)
        # destination rectangles of a page are disjoint
        for page in range(1 + max(j["page"] for j in jobs)):
            cover = np.zeros((S.H, S.W), np.int32)
            for j in jobs:
                if j["page"] == page:
                    cover[j["dst_y"]:j["dst_y"] + S.BLOCK_H[j["bsize"]], j["dst_x"]:j["dst_x"] + S.BLOCK_W[j["bsize"]]] += 1
            assert cover.max() == 1


def test_depth_8_in_16_bit_words_is_depth_8(cases):
    strip = lambda got: [(r, c) for r, c, _ in got]
    assert strip(cases[0][1]) == strip(cases[1][1]) and strip(cases[0][1]) != strip(cases[2][1])


# ------------------------------------------------------------------------------------------------------------------ the library's host form
def _host(pkg, case, jobs=None, dst=None, cands=True):
    return pkg.ifs_search_host(case["src"], S.ref_view(case["ref"][0]), S.ref_view(case["ref"][1]), S.c_jobs(pkg, case["jobs"] if jobs is None else jobs), dst=dst, bd=case["bd"],
                               cands=cands)


@pytest.mark.parametrize("f", range(3), ids=IDS)
def test_host_form_equals_the_restatement(pkg, cases, f):
    case, got, _ = cases[f]
    res, cand = _host(pkg, case)
    for k, (r, c, _) in enumerate(got):
        assert S.result_tuple(res[k]) == r and S.cand_tuples(cand, k) == c, (k, case["jobs"][k])
    for page in range(1 + max(j["page"] for j in case["jobs"])):
        idx = [k for k, j in enumerate(case["jobs"]) if j["page"] == page]
        dst = np.full((S.H, S.W), 0x5A, case["src"].dtype)
        want = dst.copy()
        for k in idx:
            j = case["jobs"][k]
            want[j["dst_y"]:j["dst_y"] + S.BLOCK_H[j["bsize"]], j["dst_x"]:j["dst_x"] + S.BLOCK_W[j["bsize"]]] = got[k][2]
        res, cand = _host(pkg, case, [case["jobs"][k] for k in idx], dst=dst, cands=False)
        assert cand is None and [S.result_tuple(r) for r in res] == [got[k][0] for k in idx]
        assert np.array_equal(dst, want)


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_standalone_program(pkg, cases, flags, tmp_path):
    """csrc/ifs_search.h in a program of its own (no Python, nothing preloaded) over case files: every result, candidate record, destination sample and model point,
    byte for byte, against what the library's host form and the restatement gave here; the reference pictures have exactly the contracted border"""
    if flags:
        probe = tmp_path / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this compiler has no sanitizer runtime")
    exe = str(tmp_path / "ifs_search_host_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", *flags, os.path.join(ROOT, "tests", "ifs_search_host_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    points = S.model_points()
    for f in range(3):
        case, got, _ = cases[f]
        src = case["src"]
        jobs, n = S.c_jobs(pkg, case["jobs"]), len(case["jobs"])
        dst = np.zeros((S.H, S.W), src.dtype)
        res, cand = _host(pkg, case, dst=dst)
        path = str(tmp_path / ("run%d.bin" % f))
        with open(path, "wb") as fh:
            fh.write(np.array([src.itemsize, case["bd"], S.W, S.H, src.base.shape[1], n, 1, len(points)], np.int32).tobytes())
            fh.write(src.base.tobytes() + case["ref"][0].tobytes() + case["ref"][1].tobytes() + bytes(jobs)[:C.sizeof(pkg.IfsJob) * n])
            fh.write(bytes(res)[:C.sizeof(pkg.IfsResult) * n] + bytes(cand)[:C.sizeof(pkg.IfsCand) * S.NCAND * n] + dst.tobytes())
            fh.write(np.array(points, np.int64).tobytes() + np.array([S.model_lapndz(*p) for p in points], np.int64).tobytes())
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok %d jobs" % n), (f, (r.stdout + r.stderr)[-3000:])


# ------------------------------------------------------------------------------------------------------------------ the refusals
def test_refusals_come_before_anything_is_read(pkg):
    L = pkg.lib()
    for name, cj, ca in S.refusals():
        keep, args = S.refusal_args(pkg, cj, ca)
        assert L.svt_hip_ifs_search_host(*args) == 2, name   # SVT_HIP_ERR_BAD_ARG
    keep, args = S.refusal_args(pkg, {}, {"njobs": 0})
    assert L.svt_hip_ifs_search_host(*args) == 0
