"""GPU: the intra-block-copy hash planes, hash table and hash search against the numpy restatement (tests/ibc_hash_common.py), which
tests/test_ibc_hash_ref_cpu.py pins to the reference: every hash, same_info byte, bucket start, entry and result field, bit for bit.  The planes are compared over
their valid regions only; the table bucket by bucket and in order; the search on the job lists whose conditions the CPU test asserts."""
import ctypes as C

import numpy as np
import pytest

import ibc_hash_common as I
import test_ibc_hash_abi as abi

pytestmark = pytest.mark.gpu
FILL = 0xC3
FORMATS = [(np.uint8, 8), (np.uint16, 10), (np.uint16, 8)]
IDS = ["u8", "u16_bd10", "u16_bd8"]
BD = dict(zip(IDS, (8, 10, 8)))


@pytest.fixture(scope="module")
def tables():
    """{(picture, format id): (plane, bucket_start, entries)} of the restatement, made once"""
    out = {}
    for name, pic in I.table_pictures().items():
        for (dtype, bd), fid in zip(FORMATS, IDS):
            plane = I.as_format(pic, dtype, bd)
            out[name, fid] = (plane,) + I.table(I.pyramid(plane))
    return out


@pytest.mark.parametrize("fmt", range(3), ids=IDS)
def test_block_hashes_every_size_over_the_valid_region(hip, fmt):
    dtype, bd = FORMATS[fmt]
    for w, h in I.SMALL:
        plane = I.as_format(I.small_picture(w, h), dtype, bd)
        pyr = I.pyramid(plane)
        for size in (2,) + I.SIZES:
            h1, h2, same = hip.ibc_block_hashes(plane, size, bd=bd, fill=FILL)
            if size not in pyr:   # an empty region: accepted, nothing written
                assert (h1.view(np.uint8) == FILL).all() and (h2.view(np.uint8) == FILL).all() and (same.view(np.uint8) == FILL).all(), (w, h, size)
                continue
            want = pyr[size]
            ny, nx = want["h1"].shape
            assert (ny, nx) == (h - size + 1, w - size + 1)
            assert (h1[:ny, :nx] == want["h1"]).all() and (h2[:ny, :nx] == want["h2"]).all(), (w, h, size)
            for k in range(2 if size == 2 else 3):
                assert (same[k, :ny, :nx] == want["s%d" % k]).all(), (w, h, size, k)


@pytest.mark.parametrize("fmt", IDS)
@pytest.mark.parametrize("name", ["noise", "flat", "rows", "cols", "tiled", "text"])
def test_table_bucket_by_bucket_in_order(hip, tables, name, fmt):
    plane, start, entries = tables[name, fmt]
    got_start, got_entries, info, guards = hip.ibc_hash_table(plane, bd=BD[fmt], guard=64, fill=FILL)
    assert info.tolist() == [len(entries), 1]
    assert (got_start == start).all()
    assert (got_entries[:len(entries)] == entries).all()
    assert (got_entries[len(entries):].view(np.uint8) == FILL).all() and all((g == FILL).all() for g in guards)


@pytest.mark.parametrize("name,strided", [("tiled", False), ("noise", True)])
def test_capacity_one_short_stores_nothing(hip, tables, name, strided):
    plane, start, entries = tables[name, "u8"]
    if strided:   # a stride wider than the picture
        wide = np.full((plane.shape[0], plane.shape[1] + 13), 7, plane.dtype)
        wide[:, :plane.shape[1]] = plane
        plane = wide[:, :plane.shape[1]]
    got_start, got_entries, info, guards = hip.ibc_hash_table(plane, capacity=len(entries) - 1, guard=64, fill=FILL)
    assert info.tolist() == [len(entries), 0]
    assert (got_start == start).all()
    assert (got_entries.view(np.uint8) == FILL).all() and all((g == FILL).all() for g in guards)
    # ... and with exactly enough room everything is stored
    got_start, got_entries, info, guards = hip.ibc_hash_table(plane, capacity=len(entries), guard=64, fill=FILL)
    assert info.tolist() == [len(entries), 1] and (got_start == start).all() and (got_entries == entries).all() and all((g == FILL).all() for g in guards)


@pytest.fixture(scope="module")
def searches():
    return I.search_cases()


@pytest.mark.parametrize("fmt", range(3), ids=IDS)
@pytest.mark.parametrize("case", range(4), ids=["tiled", "noise", "text_zero_costs", "text"])
def test_search_field_for_field(hip, pkg, searches, case, fmt):
    dtype, bd = FORMATS[fmt]
    c = searches[case]
    plane = I.as_format(c["pic"], dtype, bd)
    h, w = plane.shape
    start, entries = I.table(I.pyramid(plane))
    jc, cc = I.cost_tables(zero=c["zero"])
    good = c["jobs"]
    jobs = [j for i, g in enumerate(good) for j in ([g] if i % 8 else [dict(g, **I.BAD_JOBS[(i // 8) % len(I.BAD_JOBS)]), g])]   # bad jobs between good ones
    want = [I.search(plane, bd, start, entries, jc, cc, j) for j in jobs]
    assert any(r["count"] < 0 for r in want) and any(r["found"] for r in want)
    got = I.c_results(hip.ibc_hash_search_batch(plane, start, entries, jc, cc, I.c_jobs(pkg, jobs), bd=bd, fill=FILL), len(jobs))
    for i, (g, r) in enumerate(zip(got, want)):
        assert g == r, (i, jobs[i])


@pytest.mark.parametrize("fmt", range(3), ids=IDS)
def test_search_costs_real_differences(hip, pkg, fmt):
    """a hand-made table whose entries differ from the job's block (ibc_hash_common.forged_case): variances other than 0, at depth 10 in the scaled form"""
    dtype, bd = FORMATS[fmt]
    plane, start, entries, jobs = I.forged_case(dtype, bd)
    jc, cc = I.cost_tables()
    want = [I.search(plane, bd, start, entries, jc, cc, j) for j in jobs]
    assert all(r["found"] and r["n_matched"] < r["count"] for r in want) and sum(r["best_cost"] > 1000 for r in want) == 3 and any(r["n_valid"] > 64 for r in want)
    assert I.c_results(hip.ibc_hash_search_batch(plane, start, entries, jc, cc, I.c_jobs(pkg, jobs), bd=bd), len(jobs)) == want


def test_search_on_the_table_the_device_built_and_an_empty_list(hip, pkg, searches):
    c = searches[0]
    plane = c["pic"]
    start, entries, info, _ = hip.ibc_hash_table(plane)
    assert info[1] == 1
    entries = entries[:info[0]]
    jc, cc = I.cost_tables()
    jobs = c["jobs"][::5]
    want = [I.search(plane, 8, start, entries, jc, cc, j) for j in jobs]
    assert I.c_results(hip.ibc_hash_search_batch(plane, start, entries, jc, cc, I.c_jobs(pkg, jobs)), len(jobs)) == want
    res = hip.ibc_hash_search_batch(plane, start, entries, jc, cc, (pkg.IbcSearchJob * 0)(), fill=FILL)   # njobs = 0: accepted, nothing launched, nothing written
    assert bytes(res) == bytes([FILL]) * C.sizeof(res)


def test_refusals_with_a_live_context(hip, pkg):
    L = hip.L
    d = hip.to_device(np.zeros(12 << 20, np.uint8))   # zeros: a flat picture, a job with a bad size
    # the calls that run get a region of their own for every buffer, in quarters of a MiB; the table's starts take 2 MiB + 4, the scratch the rest
    quarters = dict(d_luma=0, d_bucket_start=4, d_entries=14, d_info=16, d_hash1=17, d_hash2=18, d_same=19, d_mv_joint_cost=20, d_mv_comp_cost=21, d_jobs=23, d_results=24,
                    d_scratch=28)
    own = {k: d.value + (q << 18) for k, q in quarters.items()}
    assert L.svt_hip_ibc_hash_scratch_bytes(abi.TABLE_OK["width"], abi.TABLE_OK["height"]) <= (12 << 20) - (28 << 18)
    try:
        assert abi.call_hashes(L, hip.h, own) == 0 and abi.call_table(L, hip.h, own) == 0 and abi.call_search(L, hip.h, own) == 0
        assert abi.call_search(L, hip.h, own, njobs=0) == 0
        hip.check(L.svt_hip_sync(hip.h), "sync")
        assert hip.to_host(C.c_void_p(own["d_info"]), (2,), np.int32).tolist() == [128 + 32 + 8 + 2, 0]   # the grid positions of 4 .. 32 in 64 x 32; capacity 16
        assert hip.to_host(C.c_void_p(own["d_results"]), (7,), np.int32).tolist() == [-1, 0, 0, 0, I.INT32_MAX, 0, 0]
        for calls, bad, name in ((abi.call_hashes, abi.HASHES_BAD, "svt_hip_ibc_block_hashes_dev"), (abi.call_table, abi.TABLE_BAD, "svt_hip_ibc_hash_table_dev"),
                                 (abi.call_search, abi.SEARCH_BAD, "svt_hip_ibc_hash_search_batch_dev")):
            for c in bad:
                assert calls(L, hip.h, d.value, **c) == abi.BAD_ARG, c
                assert L.svt_hip_last_error(hip.h).decode().startswith(name + ": bad argument"), c
        assert abi.call_table(L, hip.h, d.value, d_scratch=d.value + 8) == abi.BAD_ARG   # not 256-byte aligned
        hip.check(L.svt_hip_sync(hip.h), "sync")
    finally:
        hip.free(d)
