"""GPU: svt_hip_cfl_predict_batch_dev, bit for bit against the reference's composition svt_cfl_luma_subsampling_420 -> svt_subtract_average -> svt_cfl_predict
(tests/cfl_common.py), 8-bit and 10-bit.  What the generator's jobs contain is checked with the reference alone in tests/test_cfl_ref_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import cfl_common as cc
import intra_common as ic
import test_cfl_abi as abi
from conftest import ROOT

pytestmark = pytest.mark.gpu
BDS = cc.BDS + [(np.uint16, 8)]     # (uint16, 8): 8-bit samples in 16-bit planes, against the reference's high-bit-depth functions with bd 8
_basic = {}


def basic(ref, dtype, bd):
    """The 420 generator jobs of a format and their reference results: computed once, shared, never modified (variants are shallow copies).
    8-bit samples in 16-bit planes are the (uint8, 8) jobs widened (the generator draws the same values), and the reference's 8-bit and high-bit-depth functions
    must agree on them -- AC values and both predicted planes, which stay inside 0 .. 255 and reach both ends."""
    if (dtype, bd) not in _basic:
        jobs = cc.cfl_basic_jobs(dtype, bd)
        refs = cc.ref_cfl_jobs(ref, jobs, bd)
        if dtype == np.uint16 and bd == 8:
            jobs8, refs8 = basic(ref, np.uint8, 8)
            outs = []
            for j, j8, r, r8 in zip(jobs, jobs8, refs, refs8):
                assert np.array_equal(j["luma"], j8["luma"]) and np.array_equal(j["pred"], j8["pred"]) and np.array_equal(j["recs"], j8["recs"])
                assert np.array_equal(r[0], r8[0]) and all(a.dtype == np.uint16 and b.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(r[1], r8[1])), j["tx_size"]
                outs += r[1]
            assert max(int(o.max()) for o in outs) == 255 and min(int(o.min()) for o in outs) == 0
        _basic[dtype, bd] = (jobs, refs)
    return _basic[dtype, bd]


@pytest.mark.parametrize("dtype,bd", BDS)
def test_all_shapes_inplace_and_dc(hip, pkg, ref, dtype, bd):
    """14 shapes x (random alphas, extreme content at alpha +-16, an all-maximum block) x (in-place, dc_from_edges with dc_have 0..3) in one launch; planes and d_ac."""
    jobs, refs = basic(ref, dtype, bd)
    got = cc.cfl_check(hip, pkg, jobs, refs, dtype, what="basic", bd=bd)
    if dtype == np.uint16 and bd == 8:        # the second witness: the device on the same jobs as uint8 planes (job i sits at the same place; the guard bands hold another marker)
        jobs8, refs8 = basic(ref, np.uint8, 8)
        got8 = cc.cfl_check(hip, pkg, jobs8, refs8, np.uint8, what="basic, uint8", bd=8)
        _, _, _, pos = cc.cfl_layout(jobs, dtype)
        for j, (x, y) in zip(jobs, pos):
            w, h = cc.cfl_dims(j)
            assert all(np.array_equal(got[pl][y:y + h, x:x + w], got8[pl][y:y + h, x:x + w]) for pl in (0, 1)), j["tx_size"]
        assert np.array_equal(got[2], got8[2])


@pytest.mark.parametrize("dtype,bd", BDS)
def test_plane_masks(hip, pkg, ref, dtype, bd):
    """plane_mask 1 / 2 / 3: the unselected plane keeps what it held; a plane that is not given (NULL) is written by no job whatever the masks say."""
    jobs, refs = basic(ref, dtype, bd)
    jobs = [dict(j, plane_mask=1 + i % 3) for i, j in enumerate(jobs[::3])]
    refs = refs[::3]
    assert {(j["plane_mask"], j["dc_from_edges"]) for j in jobs} == {(m, d) for m in (1, 2, 3) for d in (0, 1)}
    cc.cfl_check(hip, pkg, jobs, refs, dtype, what="masks", bd=bd)
    cc.cfl_check(hip, pkg, jobs, refs, dtype, give=(True, False), what="cb only", bd=bd)
    cc.cfl_check(hip, pkg, jobs, refs, dtype, give=(False, True), want_ac=False, what="cr only", bd=bd)


@pytest.mark.parametrize("dtype,bd", BDS)
def test_offset_odd_stride_views(hip, pkg, ref, dtype, bd):
    """Luma and chroma planes as offset views with an odd row stride: no wide access is aligned; the guard bands and what surrounds the views survive."""
    jobs, refs = basic(ref, dtype, bd)
    cc.cfl_check(hip, pkg, jobs[::2], refs[::2], dtype, view=True, what="views", bd=bd)


@pytest.mark.parametrize("dtype,bd", BDS)
def test_order_and_counts(hip, pkg, ref, dtype, bd):
    """Shuffled jobs (a wave then mixes shapes), njobs 0 and 1, and counts that leave the last workgroup (32 jobs) and its last wave (8 jobs) partly filled."""
    jobs, refs = basic(ref, dtype, bd)
    rng = np.random.default_rng(61 + bd)
    perm = rng.permutation(len(jobs))
    cc.cfl_check(hip, pkg, jobs, refs, dtype, order=perm, what="shuffled", bd=bd)
    for n in (0, 1, 37, 75):
        cc.cfl_check(hip, pkg, jobs[:96], refs[:96], dtype, order=perm[perm < 96][:n], what=f"njobs {n}", bd=bd)
    cc.cfl_check(hip, pkg, [], [], dtype, what="no jobs at all", bd=bd)


@pytest.mark.parametrize("dtype,bd", BDS)
def test_unusable_jobs_write_nothing(hip, pkg, ref, dtype, bd):
    """tx_size with a 64-sample side or out of range, |alpha| = 17 on either plane: nothing written, neither planes nor d_ac, while their neighbours in the wave are right."""
    good, grefs = basic(ref, dtype, bd)
    rng = np.random.default_rng(62 + bd)
    jobs, refs = list(good[:64]), list(grefs[:64])
    bad = {3: dict(tx_size=4), 9: dict(tx_size=11), 10: dict(tx_size=12), 17: dict(tx_size=17), 18: dict(tx_size=18), 30: dict(tx_size=19), 31: dict(tx_size=255),
           40: dict(alpha=(17, 0)), 41: dict(alpha=(0, -17)), 42: dict(alpha=(-17, 17)), 63: dict(alpha=(5, 17))}
    for i, chg in bad.items():
        j = cc.cfl_job(rng, dtype, bd, chg.get("tx_size", jobs[i]["tx_size"]), chg.get("alpha", jobs[i]["alpha"]), "random", 3, i & 1, 3)
        assert not cc.cfl_valid(j)
        jobs[i], refs[i] = j, None
    cc.cfl_check(hip, pkg, jobs, refs, dtype, what="unusable jobs", bd=bd)


@pytest.mark.parametrize("dtype,bd", BDS)
def test_dc_by_the_batch_predictor_then_cfl_in_place(hip, pkg, ref, dtype, bd):
    """Two dependent calls on one stream without a synchronisation between them: svt_hip_intra_predict_batch_dev writes DC_PRED into both chroma planes, the
    in-place CfL call follows.  The result is what dc_from_edges gives in one call (= the reference)."""
    jobs, refs = basic(ref, dtype, bd)
    keep = [i for i, j in enumerate(jobs) if j["dc_from_edges"]][::4]
    jobs, refs = [jobs[i] for i in keep], [refs[i] for i in keep]
    luma, cb, cr, pos = cc.cfl_layout(jobs, dtype)
    order = list(range(len(jobs)))
    arr = cc.cfl_job_array(pkg, jobs, pos, order)
    ij = [(pkg.IntraJob * len(jobs))(), (pkg.IntraJob * len(jobs))()]
    for i, j in enumerate(jobs):
        arr[i].dc_from_edges = 0
        for pl in (0, 1):
            J = ij[pl][i]
            J.edge_off, J.dst_x, J.dst_y, J.tx_size, J.mode, J.dc_have = arr[i].edge_off[pl], pos[i][0], pos[i][1], j["tx_size"], 0, j["dc_have"]
    L, pb = hip.L, dtype().itemsize
    held = [hip.to_device(a) for a in (luma, cc.cfl_edges(jobs, dtype), cb, cr)]
    d_luma, d_edges, d_cb, d_cr = held
    try:
        for a in (arr, ij[0], ij[1]):
            held.append(hip.empty(C.sizeof(a)))
            hip.check(L.svt_hip_memcpy_h2d(hip.h, held[-1], C.cast(a, C.c_void_p), C.sizeof(a)), "h2d")
        d_arr, d_ij0, d_ij1 = held[4:]
        hip.check(L.svt_hip_intra_predict_batch_dev(hip.h, pb, bd, d_edges, d_ij0, len(jobs), d_cb, cb.shape[1]), "dc cb")
        hip.check(L.svt_hip_intra_predict_batch_dev(hip.h, pb, bd, d_edges, d_ij1, len(jobs), d_cr, cr.shape[1]), "dc cr")
        hip.check(L.svt_hip_cfl_predict_batch_dev(hip.h, pb, bd, d_luma, luma.shape[1], d_edges, d_arr, len(jobs), d_cb, d_cr, cb.shape[1], None), "cfl")
        hip.check(L.svt_hip_sync(hip.h), "sync")
        got = hip.to_host(d_cb, cb.shape, dtype), hip.to_host(d_cr, cr.shape, dtype)
    finally:
        hip.free(*held)
    ecb, ecr, _ = cc.cfl_expected(jobs, refs, cb, cr, pos, order)
    assert np.array_equal(got[0], ecb) and np.array_equal(got[1], ecr)


@pytest.mark.parametrize("tw", [8, 16])
@pytest.mark.parametrize("dtype,bd", BDS)
def test_whole_picture(hip, pkg, ref, dtype, bd, tw):
    """A 352x288 4:2:0 picture tiled completely with 8x8 / 16x16 chroma blocks, in place, against the reference run tile by tile on the planes."""
    luma, cb, cr, tiles = cc.cfl_picture_jobs(dtype, bd, tw)
    assert len(tiles) == (176 // tw) * (144 // tw)
    ecb, ecr = cc.ref_cfl_picture(ref, luma, cb, cr, tiles, bd)
    assert (ecb != cb).mean() > 0.5 and (ecr != cr).mean() > 0.5
    gcb, gcr = hip.cfl_predict_batch(luma, np.zeros(4, dtype), cc.cfl_picture_array(pkg, tiles), cb, cr, bd=bd)
    assert np.array_equal(gcb, ecb) and np.array_equal(gcr, ecr)


@pytest.mark.parametrize("dtype,bd", cc.BDS)
def test_golden(hip, pkg, dtype, bd):
    """The stored case (tests/golden/make_cfl_golden.py): holds where the reference library is absent."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_cfl_golden as mk
    jobs, refs = mk.load_cfl(np.load(os.path.join(ROOT, "tests", "golden", "cfl_filter_intra.npz")), dtype, bd)
    assert len(jobs) >= 5
    cc.cfl_check(hip, pkg, jobs, refs, dtype, what="golden", bd=bd)
    cc.cfl_check(hip, pkg, jobs, refs, dtype, view=True, order=range(len(jobs) - 1, -1, -1), what="golden, views", bd=bd)


def test_bad_arguments_with_a_context(hip, pkg):
    L = pkg.lib()
    d = hip.empty(1 << 16)
    try:
        assert abi.call_cfl(L, hip.h, d, njobs=0) == 0 and abi.call_cfl(L, hip.h, d, njobs=0, pix_bytes=2, bd=10) == 0 and abi.call_cfl(L, hip.h, d, njobs=0, pix_bytes=2) == 0
        assert abi.call_cfl(L, hip.h, d, njobs=0, d_ac=None) == 0 and abi.call_cfl(L, hip.h, d, njobs=0, d_cb=None) == 0 and abi.call_cfl(L, hip.h, d, njobs=0, d_cr=None) == 0
        for bad in abi.CFL_BAD:
            assert abi.call_cfl(L, hip.h, d, **dict(dict(njobs=0), **bad)) == abi.BAD_ARG, bad
    finally:
        hip.free(d)
