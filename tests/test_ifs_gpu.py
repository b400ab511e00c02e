"""GPU: svt_hip_ifs_search_batch_dev against the numpy restatement of interpolation_filter_search (tests/ifs_common.py, pinned to the reference in
tests/test_ifs_ref_cpu.py) on the shared job list, in the three sample formats: every field of every record, the winner's prediction against the two prediction
calls, and independence from how the list is composed and launched."""

import numpy as np
import pytest

import ifs_common as S

pytestmark = pytest.mark.gpu
FORMATS = [(np.uint8, 8), (np.uint16, 8), (np.uint16, 10)]
IDS = ["u8", "u16_bd8", "u16_bd10"]
FILL = 0xC3


@pytest.fixture(scope="module")
def cases():
    out = {}
    for f, (dtype, bd) in enumerate(FORMATS):
        case = S.build_case(bd, dtype)
        out[f] = (case, S.run_case(case))
    return out


def _launch(hip, pkg, case, jobs=None, **kw):
    jobs = case["jobs"] if jobs is None else jobs
    return hip.ifs_search_batch(case["src"], S.ref_view(case["ref"][0]), S.ref_view(case["ref"][1]), S.c_jobs(pkg, jobs), bd=case["bd"], fill=FILL, **kw)


def _records(res, cand, n):
    return [(S.result_tuple(res[k]), S.cand_tuples(cand, k) if cand is not None else None) for k in range(n)]


@pytest.mark.parametrize("f", range(3), ids=IDS)
def test_every_record_equals_the_restatement(hip, pkg, cases, f):
    case, got = cases[f]
    n = len(case["jobs"])
    res, cand, _ = _launch(hip, pkg, case)
    assert S.fill_words_left(res, FILL) == 0 and S.fill_words_left(cand, FILL) == 0
    for k, (r, c, _) in enumerate(got):
        assert S.result_tuple(res[k]) == r and S.cand_tuples(cand, k) == c, (k, case["jobs"][k], S.result_tuple(res[k]), r)
    whole = _records(res, cand, n)
    # the list reversed; cut into single-job calls; twice back to back with no synchronisation in between; without candidate records
    res_r, cand_r, _ = _launch(hip, pkg, case, jobs=case["jobs"][::-1])
    assert _records(res_r, cand_r, n)[::-1] == whole
    res_1, cand_1, _ = _launch(hip, pkg, case, lists=[(k, 1) for k in range(n)])
    assert _records(res_1, cand_1, n) == whole
    res_2, cand_2, _ = _launch(hip, pkg, case, calls=2)
    assert _records(res_2, cand_2, n) == whole
    res_n, cand_n, _ = _launch(hip, pkg, case, cands=False)
    assert cand_n is None and [S.result_tuple(r) for r in res_n][:n] == [r for r, _ in whole]


def _prediction_calls(hip, pkg, case, jobs, winners, dst):
    """the same rectangles from svt_hip_subpel_predict_batch_dev / svt_hip_compound_predict_batch_dev with the winners' banks.  Those calls read whole 16 x 16 tiles,
    so they get reference planes with a wider border of zeros; the samples inside the contracted border are the same."""
    pb = case["src"].itemsize
    wide = [np.zeros((S.H + 40, S.W + 40), case["src"].dtype) for _ in range(2)]
    for a, w in zip(case["ref"], wide):
        w[8 - S.REACH_LO:8 - S.REACH_LO + a.shape[0], 8 - S.REACH_LO:8 - S.REACH_LO + a.shape[1]] = a
    conv, comp = [], []
    for j, best in zip(jobs, winners):
        fy, fx = S.FILTER_SETS[best]
        bw, bh = S.BLOCK_W[j["bsize"]], S.BLOCK_H[j["bsize"]]
        if j["type"] < 0:
            conv.append(pkg.ConvBlk(j["ref0_x"], j["ref0_y"], j["dst_x"], j["dst_y"], bw, bh, fx, fy, j["subpel0_x"], j["subpel0_y"], 0, 0))
        else:
            b = pkg.CompBlk(j["ref0_x"], j["ref0_y"], j["ref1_x"], j["ref1_y"], j["dst_x"], j["dst_y"], bw, bh, fx, fy, j["subpel0_x"], j["subpel0_y"], j["subpel1_x"],
                            j["subpel1_y"], j["type"], j["fwd_offset"], j["bck_offset"], 0)
            b.mask_off, b.mask_stride = -1, 0
            comp.append(b)
    with hip.scope() as s:
        r = [s.plane(w[8:8 + S.H, 8:8 + S.W]) for w in wide]
        d = s.plane(dst)
        if conv:
            hip.call("subpel_predict_batch_dev", pb, case["bd"], r[0].ptr, r[0].stride, d.ptr, d.stride, s.structs((pkg.ConvBlk * len(conv))(*conv)), len(conv))
        if comp:
            hip.call("compound_predict_batch_dev", pb, case["bd"], r[0].ptr, r[0].stride, r[1].ptr, r[1].stride, d.ptr, d.stride, None, s.structs((pkg.CompBlk * len(comp))(*comp)),
                     len(comp))
        hip.sync()
        return s.plane_back(d)


@pytest.mark.parametrize("f", range(3), ids=IDS)
def test_the_winners_prediction_is_what_the_prediction_calls_write(hip, pkg, cases, f):
    case, got = cases[f]
    for page in range(1 + max(j["page"] for j in case["jobs"])):
        idx = [k for k, j in enumerate(case["jobs"]) if j["page"] == page]
        jobs = [case["jobs"][k] for k in idx]
        start = np.full((S.H + 2, S.W + 24), 0x5A, case["src"].dtype)[1:1 + S.H, 8:8 + S.W]   # a view: what lies around the plane comes back too
        res, cand, dst = _launch(hip, pkg, case, jobs=jobs, dst=start)
        assert _records(res, cand, len(idx)) == [(got[k][0], got[k][1]) for k in idx]   # d_dst changes nothing else
        want = start.copy()
        for k in idx:
            j = case["jobs"][k]
            want[j["dst_y"]:j["dst_y"] + S.BLOCK_H[j["bsize"]], j["dst_x"]:j["dst_x"] + S.BLOCK_W[j["bsize"]]] = got[k][2]
        assert np.array_equal(dst, want)
        assert (dst.base == 0x5A)[np.pad(np.zeros((S.H, S.W), bool), ((1, 1), (8, 16)), constant_values=True)].all()   # nothing outside the plane
        assert np.array_equal(_prediction_calls(hip, pkg, case, jobs, [got[k][0][0] for k in idx], start), want)


def test_refusals_leave_the_device_alone(hip, pkg):
    for name, cj, ca in S.refusals():
        keep, args = S.refusal_args(pkg, cj, ca)
        assert hip.L.svt_hip_ifs_search_batch_dev(hip.h, *args) == 2, name   # SVT_HIP_ERR_BAD_ARG
    hip.sync()
