"""GPU: svt_hip_filter_intra_predict_batch_dev, bit for bit against svt_av1_filter_intra_predictor_c / highbd_filter_intra_predictor (tests/cfl_common.py), 8-bit and
10-bit.  That the extreme records clip at both ends in every mode is checked with the reference alone in tests/test_cfl_ref_cpu.py."""
import os
import sys

import numpy as np
import pytest

import cfl_common as cc
import test_cfl_abi as abi
from conftest import ROOT

pytestmark = pytest.mark.gpu
BDS = cc.BDS + [(np.uint16, 8)]     # (uint16, 8): 8-bit samples in 16-bit planes, against highbd_filter_intra_predictor with bd 8
_cases = {}


def case(ref, dtype, bd, kind):
    """14 shapes x 5 modes, one record each, and the reference blocks: computed once and shared.  8-bit samples in 16-bit planes are the (uint8, 8) records widened,
    and the reference's 8-bit and high-bit-depth predictors must agree on them (asserted here, on the CPU)."""
    if (dtype, bd, kind) not in _cases:
        jobs = cc.fi_all_jobs()
        recs = cc.fi_records(np.random.default_rng(9000 + bd + (2 if kind == "extreme" else 1)), len(jobs), dtype, bd, kind)
        refs = [cc.ref_filter_intra(ref, r, bd, t, m) for (t, m), r in zip(jobs, recs)]
        if dtype == np.uint16 and bd == 8:
            _, recs8, refs8 = case(ref, np.uint8, 8, kind)
            assert np.array_equal(recs, recs8) and all(a.dtype == np.uint16 and b.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(refs, refs8))
            assert max(int(r.max()) for r in refs) == 255 and min(int(r.min()) for r in refs) == 0
        _cases[dtype, bd, kind] = (jobs, recs, refs)
    return _cases[dtype, bd, kind]


@pytest.mark.parametrize("kind", ["random", "extreme"])
@pytest.mark.parametrize("dtype,bd", BDS)
def test_all_shapes_and_modes(hip, pkg, ref, dtype, bd, kind):
    jobs, recs, refs = case(ref, dtype, bd, kind)
    assert len(jobs) == 70
    got = cc.fi_check(hip, pkg, jobs, recs, refs, what=kind, bd=bd)
    if dtype == np.uint16 and bd == 8:        # the second witness: the device on the same records as uint8
        _, recs8, refs8 = case(ref, np.uint8, 8, kind)
        got8 = cc.fi_check(hip, pkg, jobs, recs8, refs8, what=kind + ", uint8", bd=8)
        _, pos = cc.fi_layout(jobs, dtype)
        for j, (x, y) in zip(jobs, pos):
            w, h = cc.fi_dims(j)
            assert np.array_equal(got[y:y + h, x:x + w], got8[y:y + h, x:x + w]), j


@pytest.mark.parametrize("dtype,bd", BDS)
def test_offset_odd_stride_view(hip, pkg, ref, dtype, bd):
    """The destination as an offset view with an odd row stride; the guard band around every block and what surrounds the view survive."""
    jobs, recs, refs = case(ref, dtype, bd, "extreme")
    cc.fi_check(hip, pkg, jobs, recs, refs, view=True, what="view", bd=bd)


@pytest.mark.parametrize("dtype,bd", BDS)
def test_order_and_counts(hip, pkg, ref, dtype, bd):
    """Shuffled jobs (a wave then mixes shapes and runs at its largest job's width), njobs 0 and 1, counts that leave the last workgroup / wave partly filled."""
    jobs, recs, refs = case(ref, dtype, bd, "random")
    perm = np.random.default_rng(71 + bd).permutation(len(jobs))
    cc.fi_check(hip, pkg, jobs, recs, refs, order=perm, what="shuffled", bd=bd)
    for n in (0, 1, 37, 59):
        cc.fi_check(hip, pkg, jobs, recs, refs, order=perm[:n], view=bool(n & 1), what=f"njobs {n}", bd=bd)
    cc.fi_check(hip, pkg, [], recs[:0], [], what="no jobs at all", bd=bd)


@pytest.mark.parametrize("dtype,bd", BDS)
def test_unusable_jobs_write_nothing(hip, pkg, ref, dtype, bd):
    good, recs, grefs = case(ref, dtype, bd, "extreme")
    jobs, refs = list(good), list(grefs)
    for i, j in {2: (0, 5), 11: (1, 255), 20: (4, 0), 33: (11, 2), 34: (12, 1), 47: (17, 3), 48: (18, 4), 60: (19, 0), 69: (255, 2)}.items():
        assert not cc.fi_valid(j)
        jobs[i], refs[i] = j, None
    cc.fi_check(hip, pkg, jobs, recs, refs, what="unusable jobs", bd=bd)


@pytest.mark.parametrize("dtype,bd", cc.BDS)
def test_golden(hip, pkg, dtype, bd):
    """The stored case (tests/golden/make_cfl_golden.py): holds where the reference library is absent."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_cfl_golden as mk
    jobs, recs, blocks = mk.load_fi(np.load(os.path.join(ROOT, "tests", "golden", "cfl_filter_intra.npz")), dtype, bd)
    assert len(jobs) == 14 and {m for _, m in jobs} == set(range(5))
    cc.fi_check(hip, pkg, jobs, recs, blocks, what="golden", bd=bd)


def test_bad_arguments_with_a_context(hip, pkg):
    L = pkg.lib()
    d = hip.empty(1 << 16)
    try:
        assert abi.call_fi(L, hip.h, d, njobs=0) == 0 and abi.call_fi(L, hip.h, d, njobs=0, pix_bytes=2, bd=10) == 0 and abi.call_fi(L, hip.h, d, njobs=0, pix_bytes=2) == 0
        for bad in abi.FI_BAD:
            assert abi.call_fi(L, hip.h, d, **dict(dict(njobs=0), **bad)) == abi.BAD_ARG, bad
    finally:
        hip.free(d)
