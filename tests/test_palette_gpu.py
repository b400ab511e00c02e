"""GPU: svt_hip_palette_search_batch_dev against search_palette_luma restated around the reference's own functions (tests/palette_common.py: ref_search), every
field of every record and every map byte, bit for bit.  The case list is the one tests/test_palette_ref_cpu.py proves to hold its conditions (colour counts,
reseeds of empty clusters at every n 3 .. 8, two in one iteration, 4096 samples, long runs, ties, cache distances, every shape whole and cut); one launch per
sample format, sources at odd x on a stride wider than the picture, all three outputs pre-filled so that a store outside a job's own region shows."""
import ctypes as C

import numpy as np
import pytest

import palette_common as P
import test_palette_abi as abi

pytestmark = pytest.mark.gpu
FILL = 0xC3


@pytest.fixture(scope="module")
def lists():
    return {(np.dtype(t).name, bd): P.build_cases(t, bd) for t, bd in P.FORMATS}


def _launch(hip, pkg, plane, jobs, bd, spacing=3):
    tab, nbytes = P.c_jobs(pkg, jobs, spacing=spacing)
    res, cands = (pkg.PaletteResult * max(len(jobs), 1))(), (pkg.PaletteCand * (P.MAX_CANDS * max(len(jobs), 1)))()
    C.memset(res, FILL, C.sizeof(res)); C.memset(cands, FILL, C.sizeof(cands))
    if not len(jobs): tab = (pkg.PaletteJob * 0)()
    return hip.palette_search_batch(plane, tab, res, cands, np.full(nbytes, FILL, np.uint8), bd=bd)


def _check(jobs, want, res, cands, maps):
    for i, j in enumerate(jobs):
        got = P.c_result(j, res, cands, maps, i)
        assert all(c["reserved"] == 0 for c in got["cands"]), i
        assert P.same_result(got, want[i]) is None, (i, {k: v for k, v in j.items() if k != "cache"}, P.same_result(got, want[i]))
    assert P.untouched(jobs, want, res, cands, maps, FILL) is None


@pytest.mark.parametrize("dtype,bd", P.FORMATS, ids=["u8", "u16_bd8", "u16_bd10"])
def test_case_list(hip, pkg, ref, lists, dtype, bd):
    plane, jobs = lists[(np.dtype(dtype).name, bd)]
    assert len({(j["bw"], j["bh"]) for j in jobs}) == 16 and plane.strides[0] > plane.shape[1] * plane.itemsize and any(j["x"] & 1 for j in jobs)
    want = [P.ref_search(ref, plane, j, bd) for j in jobs]
    assert sum(len(w["cands"]) for w in want) > 500 and any(len(w["cands"]) == 12 for w in want)
    _check(jobs, want, *_launch(hip, pkg, plane, jobs, bd))


def test_bad_jobs_between_good_ones_and_an_empty_list(hip, pkg, ref, lists):
    plane, jobs = lists[("uint16", 10)]
    good = [j for j in jobs if 2 < len(j["cache"])][:4]
    bad = [dict(good[0], bw=8, bh=64), dict(good[0], bw=12, bh=12), dict(good[0], bw=4, bh=8), dict(good[0], cols=0), dict(good[0], cols=good[0]["bw"] + 1), dict(good[0], rows=0),
           dict(good[0], rows=good[0]["bh"] + 1), dict(good[0], n_cache=17), dict(good[0], n_cache=-1), dict(good[0], step=0), dict(good[0], step=3), dict(good[0], x=-1), dict(good[0], y=-1)]
    seq = [dict(good[0])] + [dict(j) for i, b in enumerate(bad) for j in (b, good[i % 4])]
    want = [P.ref_search(ref, plane, j, 10) if P.job_ok(j) and 0 <= j.get("n_cache", 0) <= 16 else dict(colors=-1, cands=[]) for j in seq]
    assert [w["colors"] < 0 for w in want] == [bool(i & 1) for i in range(len(seq))]
    res, cands, maps = _launch(hip, pkg, plane, seq, 10)
    assert all((res[i].colors, res[i].n_cands) == (-1, 0) for i in range(1, len(seq), 2))
    _check(seq, want, res, cands, maps)
    # njobs = 0: accepted, nothing launched, nothing written
    res, cands, maps = _launch(hip, pkg, plane, [], 10)
    assert bytes(res) == bytes([FILL]) * C.sizeof(res) and bytes(cands) == bytes([FILL]) * C.sizeof(cands) and (maps == FILL).all()


@pytest.mark.parametrize("dtype,bd", [(np.uint8, 8), (np.uint16, 10)], ids=["u8", "u16_bd10"])
def test_more_workgroups_than_compute_units(hip, pkg, ref, dtype, bd):
    """3072 jobs of 8x8, one workgroup each, of 40 kinds of content, cache and step: the reference runs once per kind"""
    plane, jobs, which = P.build_tiles(dtype, bd)
    assert len(jobs) == 3072
    kinds = {}
    for j, k in zip(jobs, which):
        if k not in kinds: kinds[k] = P.ref_search(ref, plane, j, bd)
    assert len(kinds) == 40 and any(w["cands"] for w in kinds.values()) and any(not w["cands"] for w in kinds.values())
    _check(jobs, [kinds[k] for k in which], *_launch(hip, pkg, plane, jobs, bd, spacing=0))


def test_refusals_with_a_live_context(hip, pkg):
    L = hip.L
    d = hip.to_device(np.zeros(1 << 20, np.uint8))   # a job of zeros has a bad size: the accepted call writes one result and nothing else
    try:
        assert abi.call_search(L, hip.h, d.value) == 0 and abi.call_search(L, hip.h, d.value, njobs=0) == 0
        hip.check(L.svt_hip_sync(hip.h), "sync")
        assert hip.to_host(d, (2,), np.int32).tolist() == [-1, 0]
        for c in abi.SEARCH_BAD:
            assert abi.call_search(L, hip.h, d.value, **c) == abi.BAD_ARG, c
            assert L.svt_hip_last_error(hip.h).decode().startswith("svt_hip_palette_search_batch_dev: bad argument"), c
        hip.check(L.svt_hip_sync(hip.h), "sync")
    finally:
        hip.free(d)
