"""GPU: svt_hip_ibc_full_search_batch_dev against the numpy restatement (tests/ibc_search_common.py), which tests/test_ibc_search_ref_cpu.py pins to the
reference's recorded results: every field of every result, the nested hash result included, on the case lists whose conditions the CPU test asserts, in the three
sample formats.  The results start as a byte pattern and guard bytes lie around them and around the scratch."""
import ctypes as C

import numpy as np
import pytest

import ibc_hash_common as H
import ibc_search_common as S
import test_ibc_search_abi as abi

pytestmark = pytest.mark.gpu
FILL, GUARD = 0xC3, 256
FORMATS = [(np.uint8, 8), (np.uint16, 10), (np.uint16, 8)]
IDS = ["u8", "u16_bd10", "u16_bd8"]
CASES = S.cases()
NAMES = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def prepared():
    """(case, format) -> (plane, table, cost tables, jobs with bad and empty ones between the good, what the restatement says), made once"""
    memo = {}

    def get(case, fmt):
        if (case, fmt) not in memo:
            c, (dtype, bd) = CASES[case], FORMATS[fmt]
            plane = H.as_format(c["pic"], dtype, bd)
            table = H.table(H.pyramid(plane))
            jc, cc = H.cost_tables(zero=c["zero"])
            odd = S.BAD_JOBS + S.EMPTY_JOBS
            jobs = [j for i, g in enumerate(c["jobs"]) for j in ([g] if i % 6 else [dict(g, **odd[(i // 6) % len(odd)]), g])]
            p32 = plane.astype(np.int32)
            want = [S.full_search(plane, bd, table, jc, cc, c["patterns"], j, p32=p32) for j in jobs]
            memo[case, fmt] = (plane, table, jc, cc, jobs, want)
        return memo[case, fmt]
    return get


def check(got, want, jobs, guards):
    for i, (g, r) in enumerate(zip(got, want)):
        assert g == r, (i, jobs[i])
    assert all((g == FILL).all() for g in guards)


@pytest.mark.parametrize("fmt", range(3), ids=IDS)
@pytest.mark.parametrize("case", range(len(CASES)), ids=NAMES)
def test_every_case_field_for_field(hip, pkg, prepared, case, fmt):
    plane, table, jc, cc, jobs, want = prepared(case, fmt)
    assert any(r["status"] == 0 for r in want)
    res, guards = hip.ibc_full_search_batch(plane, table, jc, cc, CASES[case]["patterns"], S.c_jobs(pkg, jobs), bd=FORMATS[fmt][1], guard=GUARD, fill=FILL)
    check(S.c_results(res, len(jobs)), want, jobs, guards)


def test_on_the_table_the_device_built_and_without_a_table(hip, pkg, prepared):
    case = NAMES.index("text_glyphs")
    plane, table, jc, cc, jobs, want = prepared(case, 0)
    start, entries, info, _ = hip.ibc_hash_table(plane)
    assert info[1] == 1
    res, guards = hip.ibc_full_search_batch(plane, (start, entries[:info[0]]), jc, cc, CASES[case]["patterns"], S.c_jobs(pkg, jobs), guard=GUARD, fill=FILL)
    check(S.c_results(res, len(jobs)), want, jobs, guards)
    assert sum(r["source"] == 2 for r in want) >= 5
    # NULL tables: a job that sets use_hash is a bad job; with the flag cleared the hash stage is "not applied"
    cleared = [dict(j, use_hash=0) for j in jobs]
    p32 = plane.astype(np.int32)
    for lst in (jobs, cleared):
        want = [S.full_search(plane, 8, None, jc, cc, CASES[case]["patterns"], j, p32=p32) for j in lst]
        res, guards = hip.ibc_full_search_batch(plane, None, jc, cc, CASES[case]["patterns"], S.c_jobs(pkg, lst), guard=GUARD, fill=FILL)
        check(S.c_results(res, len(lst)), want, lst, guards)
    assert all(r["status"] == -1 for r in [S.full_search(plane, 8, None, jc, cc, CASES[case]["patterns"], j, p32=p32) for j in jobs])
    assert any(r["status"] == 0 and r["source"] != 2 for r in want)


def test_an_empty_list_writes_nothing(hip, pkg, prepared):
    plane, table, jc, cc, jobs, want = prepared(0, 0)
    res, guards = hip.ibc_full_search_batch(plane, table, jc, cc, S.PATTERNS["two"], (pkg.IbcFullSearchJob * 0)(), guard=GUARD, fill=FILL)
    assert bytes(res) == bytes([FILL]) * C.sizeof(res) and all((g == FILL).all() for g in guards)


@pytest.mark.parametrize("fmt", range(3), ids=IDS)
def test_a_strided_plane(hip, pkg, prepared, fmt):
    case = NAMES.index("noise_four")
    plane, table, jc, cc, jobs, want = prepared(case, fmt)
    wide = np.full((plane.shape[0], plane.shape[1] + 13), 7, plane.dtype)
    wide[:, :plane.shape[1]] = plane
    res, guards = hip.ibc_full_search_batch(wide[:, :plane.shape[1]], table, jc, cc, CASES[case]["patterns"], S.c_jobs(pkg, jobs), bd=FORMATS[fmt][1], guard=GUARD, fill=FILL)
    check(S.c_results(res, len(jobs)), want, jobs, guards)


def test_a_long_list_of_every_shape_shares_its_launches(hip, pkg, prepared):
    """workgroups that leave at once (bad jobs, jobs whose mesh does not run, ended walks) and workgroups that scan, in the same launches"""
    plane, table, jc, cc = prepared(NAMES.index("noise"), 0)[:4]
    lists = [prepared(NAMES.index(n), 0)[4] for n in ("noise", "noise_open", "noise_full", "noise_four")]   # all on the noise picture
    jobs = [l[k] for k in range(max(map(len, lists))) for l in lists if k < len(l)]                            # interleaved
    p32 = plane.astype(np.int32)
    want = [S.full_search(plane, 8, table, jc, cc, S.PATTERNS["two"], j, p32=p32) for j in jobs]
    assert len(jobs) >= 200 and {(j["block_w"], j["block_h"]) for j, r in zip(jobs, want) if r["status"] == 0} == set(S.SHAPES)
    assert sum(r["mesh_ran"] for r in want) >= 20 and sum(r["status"] != 0 for r in want) >= 10
    res, guards = hip.ibc_full_search_batch(plane, table, jc, cc, S.PATTERNS["two"], S.c_jobs(pkg, jobs), guard=GUARD, fill=FILL)
    check(S.c_results(res, len(jobs)), want, jobs, guards)


def test_refusals_with_a_live_context(hip, pkg):
    L = hip.L
    d = hip.to_device(np.zeros(8 << 20, np.uint8))   # zeros: a flat picture, jobs with a bad shape
    quarters = dict(d_luma=0, d_bucket_start=1, d_entries=10, d_mv_joint_cost=11, d_mv_comp_cost=12, d_jobs=14, d_results=15, d_scratch=16)
    own = {k: d.value + (q << 18) for k, q in quarters.items()}
    try:
        assert abi.call_full(L, hip.h, own) == 0 and abi.call_full(L, hip.h, own, njobs=0) == 0
        assert abi.call_full(L, hip.h, own, d_bucket_start=None, d_entries=None) == 0
        hip.check(L.svt_hip_sync(hip.h), "sync")
        assert hip.to_host(C.c_void_p(own["d_results"]), (C.sizeof(pkg.IbcFullSearchResult) // 4,), np.int32).tolist()[:4] == [-1, 0, 0, S.INT_MAX]
        for c in abi.FULL_BAD:
            assert abi.call_full(L, hip.h, d.value, **c) == abi.BAD_ARG, c
            assert L.svt_hip_last_error(hip.h).decode().startswith("svt_hip_ibc_full_search_batch_dev: bad argument"), c
        assert abi.call_full(L, hip.h, d.value, d_scratch=d.value + 8) == abi.BAD_ARG   # not 256-byte aligned
        hip.check(L.svt_hip_sync(hip.h), "sync")
    finally:
        hip.free(d)
