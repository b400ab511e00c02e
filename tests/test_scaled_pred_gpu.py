"""GPU: svt_hip_scaled_predict_batch_dev and svt_hip_scaled_jobs_dev against the numpy restatement of tests/scaled_common.py (which
tests/test_scaled_pred_ref_cpu.py holds against the reference itself on these very lists).  One launch per list and format; the destination array is
pre-filled with a pattern and compared whole, margins included, so a stray store shows.  Bit-exact: no comparison carries a tolerance."""
import ctypes as C

import numpy as np
import pytest

import scaled_common as sc
from test_scaled_pred_abi import BAD_ARG, PREDICT_BAD, JOBS_BAD, call_predict, call_jobs

pytestmark = pytest.mark.gpu
FMTS = [pytest.param(bd, dt, id="%s-%d" % (np.dtype(dt).name, bd)) for bd, dt in sc.FMTS]


def launch(hip, c, bd, dt, compound, jobs=None):
    views, root = sc.ref_views(bd, dt), sc.dst_root(c, bd, dt)
    out = hip.scaled_predict(views[0], views[1] if compound else None, sc.dst_view(root), c.jobs if jobs is None else jobs, bd=bd)
    assert out.base.shape == root.shape
    return out.base, root


def first_difference(c, got, want):
    for i, (b, d) in enumerate(zip(c.jobs, c.desc)):
        g, w = (sc.dst_view(a)[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w] for a in (got, want))
        if not np.array_equal(g, w): return i, d, np.argwhere(g != w)[:4].tolist()
    return "outside every job's destination", np.argwhere(got != want)[:4].tolist()


@pytest.mark.parametrize("bd,dt", FMTS)
def test_single_reference_list(hip, bd, dt):
    """all 22 sizes x the step pairs (x alone, both axes), phases 0 / 63 / 64 / 1023, random / flat maximum / 0-max noise, 128 x 128 at 2048 x 2048, windows that start
    left of and above the plane inside a larger array of odd stride"""
    c = sc.single_cases()
    got, _ = launch(hip, c, bd, dt, False)
    want = sc.expected("single", bd, dt)
    assert np.array_equal(got, want), first_difference(c, got, want)


@pytest.mark.parametrize("bd,dt", FMTS)
def test_compound_list(hip, bd, dt):
    """plain average and every distance-weight pair in both orders; the two references with different steps and strides; either one unscaled"""
    c = sc.compound_cases()
    got, _ = launch(hip, c, bd, dt, True)
    want = sc.expected("compound", bd, dt)
    assert np.array_equal(got, want), first_difference(c, got, want)


def test_a_job_outside_the_domain_writes_nothing(hip):
    """what the kernel's window arithmetic cannot hold is refused per job: the rest of the launch is as it would be without those jobs"""
    c = sc.single_cases()
    jobs = (sc.ScaledBlk * 6)(*[c.jobs[i] for i in range(6)])
    jobs[0].xs0, jobs[1].ys0, jobs[2].subpel0_x, jobs[3].w, jobs[4].bank_y = 2049, 0, 1024, 129, 6
    got, root = launch(hip, c, 8, np.uint8, False, jobs)
    want, b = root.copy(), c.jobs[5]
    sc.dst_view(want)[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w] = sc.predict_job(b, sc.planes_of(8, np.uint8), 8)
    assert np.array_equal(got, want)


def test_job_builder_equals_block_params(hip, pkg):
    """svt_hip_scaled_jobs_dev record for record on the clamp cases of the CPU test, with two different scale-factor sets and with reference 1 as the twin"""
    sets = sc.clamp_records()
    total = 0
    for k, (sizes, recs) in enumerate(sets):
        other = sets[(k + 1) % len(sets)][0]
        for sizes1 in (other, None):
            sf0, sf1 = sc.scale_factors(*sizes), sc.scale_factors(*(sizes1 or sizes))
            frames = ((sizes[0], sizes[1]), (sizes1 or sizes)[:2])
            jobs = hip.scaled_jobs(pkg.ScaleFactors(*sf0), pkg.ScaleFactors(*sf1) if sizes1 else None, frames if sizes1 else (frames[0], (0, 0)), recs)
            for i, (r, b) in enumerate(zip(recs, jobs)):
                assert sc.job_tuple(b) == sc.job_of_record(r, sf0, sf1, frames), (sizes, sizes1, i)
            total += len(recs)
    assert total == 2 * 315


def test_bad_arguments_with_a_live_context(hip, pkg):
    """the refusals of tests/test_scaled_pred_abi.py again, now with their texts"""
    L = pkg.lib()
    with hip.scope() as s:
        p = s.empty(4096)
        for chg in PREDICT_BAD:
            assert call_predict(L, hip.h, p, **chg) == BAD_ARG and L.svt_hip_last_error(hip.h).decode().startswith("svt_hip_scaled_predict_batch_dev: "), chg
        for chg in JOBS_BAD:
            assert call_jobs(pkg, L, hip.h, p, **chg) == BAD_ARG and L.svt_hip_last_error(hip.h).decode().startswith("svt_hip_scaled_jobs_dev: "), chg
        assert call_predict(L, hip.h, p, n=0) == 0 and call_jobs(pkg, L, hip.h, p, n=0) == 0
