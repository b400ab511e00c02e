"""GPU: svt_hip_wedge_masks_dev and svt_hip_compound_search_batch_dev against the numpy restatement (tests/comp_search_common.py), which
tests/test_comp_search_ref_cpu.py pins to the reference's recorded results: the table byte for byte, and every field of every result and of every candidate record
on the mixed list whose conditions the CPU test asserts, in the three sample formats.  Integers and bit patterns of doubles turned integers: no tolerance."""
import ctypes as C

import numpy as np
import pytest

import comp_search_common as S
import test_comp_search_abi as abi

pytestmark = pytest.mark.gpu
FILL = 0xC3
FORMATS = [(np.uint8, 8), (np.uint16, 8), (np.uint16, 10)]
IDS = ["u8", "u16_bd8", "u16_bd10"]


@pytest.fixture(scope="module")
def grids():
    return S.golden_grids()


@pytest.fixture(scope="module")
def prepared(grids):
    """(format, "real" | "synthetic") -> (case, what the restatement says), made once"""
    memo = {}

    def get(fmt, name="real"):
        if (fmt, name) not in memo:
            dtype, bd = FORMATS[fmt]
            case = memo[fmt, "real"][0] if (fmt, "real") in memo else S.build_case(S.job_specs("mixed"), bd, dtype)
            memo[fmt, name] = (case, S.run_case(case, grids if name == "real" else S.synthetic_grids(grids)))
        return memo[fmt, name]
    return get


def check(pkg, res, cand, case, want):
    n = len(case["jobs"])
    for k, (r, c, (wr, wc)) in enumerate(zip(S.c_results(res, n), S.c_cands(cand, n), want)):
        assert r == wr and c == wc, (k, case["jobs"][k])
    # every field of every job was written: no 4-byte word of a result (the reserved one included) or of a candidate record is still the fill
    for arr, size in ((res, n * C.sizeof(pkg.CompSearchResult)), (cand, n * S.MAX_CANDS * C.sizeof(pkg.CompSearchCand))):
        assert not (np.frombuffer(bytes(arr), np.uint8)[:size].reshape(-1, 4) == FILL).all(axis=1).any()


# ------------------------------------------------------------------------------------------------------------------ the wedge table
def test_the_device_table_is_the_host_table(hip, pkg):
    d = hip.wedge_masks()
    assert d.value and hip.wedge_masks().value == d.value   # built once
    dev = hip.to_host(d, (S.TABLE_BYTES,), np.uint8)
    assert (dev == pkg.wedge_masks_host()).all() and (dev == S.wedge_table()).all()


def test_compound_predict_reads_the_device_table(hip, pkg):
    """one type-3 block of svt_hip_compound_predict_batch_dev fed the context's table equals the same call fed the table from outside"""
    rng = np.random.default_rng(3)
    refs = [rng.integers(0, 256, (48, 64)).astype(np.uint8) for _ in range(2)]
    bsize, w, sign = 8, 11, 1   # 32x16
    blk = pkg.CompBlk(src0_x=9, src0_y=8, src1_x=12, src1_y=10, dst_x=16, dst_y=8, w=32, h=16, bank_x=0, bank_y=0, subpel0_x=4, subpel0_y=0, subpel1_x=0, subpel1_y=6,
                      type=3, fwd_offset=0, bck_offset=0, mask_type=0, mask_sub=0, mask_off=S.wedge_offset(bsize, sign, w), mask_stride=32)
    blks = (pkg.CompBlk * 1)(blk)
    outs = []
    with hip.scope() as s:
        d0, d1, d_blk = s.upload(refs[0]), s.upload(refs[1]), s.structs(blks)
        for d_masks in (s.upload(S.wedge_table()), hip.wedge_masks()):
            d_dst = s.filled((48, 64), 7, np.uint8)
            hip.call("compound_predict_batch_dev", 1, 8, d0, 64, d1, 64, d_dst, 64, d_masks, d_blk, 1)
            hip.sync()
            outs.append(s.download(d_dst, (48, 64), np.uint8))
    assert (outs[0] == outs[1]).all() and (outs[0][8:24, 16:48] != 7).any() and (outs[0][:8] == 7).all()


# ------------------------------------------------------------------------------------------------------------------ the searches
@pytest.mark.parametrize("fmt", range(3), ids=IDS)
def test_mixed_list_field_for_field(hip, pkg, grids, prepared, fmt):
    case, want = prepared(fmt)
    assert {j["kind"] for j in case["jobs"]} == {0, 1, 2} and len(case["jobs"]) <= 300
    hip.set_rd_curvfit_grids(grids)
    jobs = S.c_jobs(pkg, case["jobs"])
    res, cand = hip.compound_search_batch(case["plane"], case["pool"], case["rates"], jobs, bd=case["bd"], fill=FILL)
    check(pkg, res, cand, case, want)
    # a second call on the same context: identical output; without candidate records: the same results
    res2, cand2 = hip.compound_search_batch(case["plane"], case["pool"], case["rates"], jobs, bd=case["bd"], fill=0x5A)
    assert bytes(res2) == bytes(res) and bytes(cand2) == bytes(cand)
    res3, none = hip.compound_search_batch(case["plane"], case["pool"], case["rates"], jobs, bd=case["bd"], cands=False)
    assert none is None and bytes(res3) == bytes(res)


@pytest.mark.parametrize("fmt", range(3), ids=IDS)
def test_the_grids_are_the_callers(hip, pkg, grids, prepared, fmt):
    """grids with cleared rate columns: the model's rate_i == 0 branch; set again, the first answers return"""
    case, want = prepared(fmt, "synthetic")
    assert want != prepared(fmt)[1]
    jobs = S.c_jobs(pkg, case["jobs"])
    hip.set_rd_curvfit_grids(S.synthetic_grids(grids))
    res, cand = hip.compound_search_batch(case["plane"], case["pool"], case["rates"], jobs, bd=case["bd"], fill=FILL)
    hip.set_rd_curvfit_grids(grids)
    check(pkg, res, cand, case, want)
    sub = dict(case, jobs=case["jobs"][::9])
    res, cand = hip.compound_search_batch(case["plane"], case["pool"], case["rates"], S.c_jobs(pkg, sub["jobs"]), bd=case["bd"], fill=FILL)
    check(pkg, res, cand, sub, prepared(fmt)[1][::9])


def test_an_empty_list_writes_nothing(hip, pkg, grids, prepared):
    case, _ = prepared(0)
    hip.set_rd_curvfit_grids(grids)
    res, cand = hip.compound_search_batch(case["plane"], case["pool"], case["rates"], (pkg.CompSearchJob * 0)(), fill=FILL)
    assert bytes(res) == bytes([FILL]) * C.sizeof(res) and bytes(cand) == bytes([FILL]) * C.sizeof(cand)


# ------------------------------------------------------------------------------------------------------------------ the context's checks
def test_refusals_with_a_live_context(hip, pkg, grids):
    L = hip.L
    hip.set_rd_curvfit_grids(grids)
    d = hip.to_device(np.zeros(1 << 16, np.uint8))   # zeros: a flat picture and flat predictors
    try:
        for c in abi.SEARCH_GOOD:
            assert abi.call_search(pkg, hip.h, d, **c) == 0, c
        hip.check(L.svt_hip_sync(hip.h), "sync")
        for c in abi.SEARCH_BAD:
            assert abi.call_search(pkg, hip.h, d, **c) == abi.BAD_ARG, c
            assert L.svt_hip_last_error(hip.h).decode().startswith("svt_hip_compound_search_batch_dev: bad argument"), c
        g = pkg.rd_curvfit_grids(grids)
        bad_cat = g[2].copy(); bad_cat[0] = -1
        for rate, dist, cat in ((None, g[1], g[2]), (g[0], None, g[2]), (g[0], g[1], None), (g[0], g[1], bad_cat)):
            args = [None if x is None else x.ctypes.data_as(C.c_void_p) for x in (rate, dist, cat)]
            assert L.svt_hip_set_rd_curvfit_grids(hip.h, *args) == abi.BAD_ARG
        assert L.svt_hip_wedge_masks_dev(hip.h, None) == abi.BAD_ARG
        assert abi.call_search(pkg, hip.h, d) == 0   # the refused tables changed nothing
        hip.check(L.svt_hip_sync(hip.h), "sync")
    finally:
        hip.free(d)


def test_a_fresh_context_has_no_grids(pkg, grids):
    ctx = pkg.Context(0)
    try:
        d = ctx.to_device(np.zeros(1 << 16, np.uint8))
        assert abi.call_search(pkg, ctx.h, d) == abi.BAD_ARG
        assert "svt_hip_set_rd_curvfit_grids has not been called" in ctx.L.svt_hip_last_error(ctx.h).decode()
        assert abi.call_search(pkg, ctx.h, d, njobs=0) == abi.BAD_ARG   # refused whatever the list
        ctx.set_rd_curvfit_grids(grids)
        assert abi.call_search(pkg, ctx.h, d) == 0
        ctx.sync()
        ctx.free(d)
    finally:
        ctx.close()
