"""GPU: svt_hip_gm_fit_batch_dev against the reference's fit functions on every named list and model type (tests/gm_fit_common.py), bit for bit: return value,
inlier counts and indices, the eight doubles, the converted model, the job written for the refinement.  Also several jobs in one call, calls back to back on one
scratch, the optional outputs left out, the refinement run on the jobs the fit wrote, and bad arguments with a live context."""
import ctypes as C

import numpy as np
import pytest

import gm_common as g
import gm_fit_common as fc
import gm_front_common as f
import test_gm_fit_abi as abi

pytestmark = pytest.mark.gpu


def _packed(names, capacity):
    """the named lists in one buffer of the correspondence call's layout"""
    ls = fc.lists()
    corr = np.full((len(names), capacity, 4), -12345, np.int32)
    counts = np.zeros(len(names), np.int32)
    for i, n in enumerate(names):
        l = ls[n]
        assert l["n"] <= capacity
        corr[i, :l["n"]] = l["corr"][:l["n"]]
        counts[i] = l["n"]
    return corr, counts


def _check(ref, fits, inl, jobs, job_list, names, n_refinements):
    for k, (li, t) in enumerate(job_list):
        want = fc.ref_fit(ref, names[li], t)
        assert not fc.same_fit(fc.fit_record(fits[k], inl[k] if inl is not None else None), want, with_inliers=inl is not None), (k, names[li], t)
        if jobs is not None:
            j = jobs[k]
            assert (j.ref, j.wmtype, list(j.wmmat), j.n_refinements, j.best_frame_error) == fc.expected_job(want, li, n_refinements), (k, names[li], t)


@pytest.mark.parametrize("name", fc.LIST_NAMES)
def test_every_list_and_type(hip, ref, name):
    """one call per list, a job per model type; the list's own capacity is max_points and its device-side count is passed as it is (over capacity, negative)"""
    l = fc.lists()[name]
    job_list = [(0, t) for t in fc.TYPES]
    fits, inl, jobs, _ = hip.gm_fit_batch(l["corr"][None], np.array([l["count"]], np.int32), job_list)
    _check(ref, fits, inl, jobs, job_list, [name], 5)


MIXED = ["rz_4096", "af_2500", "rz_300", "tr_300", "identity_100", "outliers_300", "rz_15", "collinear_100"]


@pytest.mark.parametrize("njobs", [1, 3, 16])
def test_jobs_in_one_call_shuffled_and_back_to_back(hip, ref, njobs):
    corr, counts = _packed(MIXED, 4096)
    rng = np.random.default_rng(njobs)
    every = [(li, t) for li in range(len(MIXED)) for t in fc.TYPES]
    job_list = [every[i] for i in rng.permutation(len(every))[:njobs]]
    fits, inl, jobs, _ = hip.gm_fit_batch(corr, counts, job_list, n_refinements=3, repeat=2)
    _check(ref, fits, inl, jobs, job_list, MIXED, 3)


def test_null_optional_outputs(hip, ref):
    corr, counts = _packed(["rz_300", "rz_15"], 300)
    job_list = [(0, fc.ROTZOOM), (1, fc.TRANSLATION), (0, fc.AFFINE)]
    fits, inl, jobs, _ = hip.gm_fit_batch(corr, counts, job_list, want_inliers=False, want_jobs=False)
    assert inl is None and jobs is None
    _check(ref, fits, None, None, job_list, ["rz_300", "rz_15"], 5)


def test_no_jobs(hip):
    corr, counts = _packed(["rz_15"], 16)
    fits, inl, jobs, _ = hip.gm_fit_batch(corr, counts, [])
    assert len(fits) == 0


def test_refinement_runs_on_the_jobs_the_fit_wrote(hip, ref):
    """the fit's jobs stay on the device and svt_hip_gm_refine_picture_dev reads them there: skipped jobs come back with wmtype -1, the others equal
    svt_av1_refine_integerized_param on the converted model"""
    src, rf = f.rot_pair(32, 96, 80)
    real = f.ref_correspondences(ref, src, f.ref_corners(ref, src), rf, f.ref_corners(ref, rf))
    assert len(real) >= 100
    names = ["rz_300", "identity_100", "outliers_300", "rz_15"]
    corr, counts = _packed(names, 300)
    corr = np.concatenate([np.full((1, 300, 4), -12345, np.int32), corr])
    corr[0, :len(real)] = real
    counts = np.concatenate([[len(real)], counts]).astype(np.int32)
    job_list = [(0, fc.ROTZOOM), (0, fc.AFFINE), (1, fc.TRANSLATION), (1, fc.ROTZOOM), (1, fc.AFFINE), (2, fc.ROTZOOM), (3, fc.AFFINE), (4, fc.TRANSLATION), (0, fc.TRANSLATION)]
    n_ref = 3
    fits, inl, jobs, res = hip.gm_fit_batch(corr, counts, job_list, n_refinements=n_ref, refine=(src, [rf] * 5))
    skipped = 0
    for k, (li, t) in enumerate(job_list):
        want = fc.ref_fit_points(ref, real, t) if li == 0 else fc.ref_fit(ref, names[li - 1], t)
        assert not fc.same_fit(fc.fit_record(fits[k], inl[k]), want), k
        exp = fc.expected_job(want, li, n_ref)
        assert (jobs[k].ref, jobs[k].wmtype, list(jobs[k].wmmat), jobs[k].n_refinements, jobs[k].best_frame_error) == exp, k
        if exp[1] < 0:
            assert res[k].wmtype == -1, k
            skipped += 1
        else:
            assert (list(res[k].wmmat), res[k].wmtype, res[k].best_error) == g.ref_refine(ref, want["wmmat"], want["wmtype"], rf, src, n_ref), k
    assert 3 <= skipped <= len(job_list) - 4   # both kinds occurred


def test_bad_arguments_with_a_live_context(hip, pkg):
    L = pkg.lib()
    d = hip.empty(1 << 16)
    try:
        for c in abi.FIT_BAD:
            assert abi.call_fit(pkg, L, hip.h, d.value, **c) == abi.BAD_ARG, c
            assert b"svt_hip_gm_fit_batch_dev" in L.svt_hip_last_error(hip.h)
        assert abi.call_fit(pkg, L, hip.h, d.value, num_motions=2) == abi.BAD_ARG and b"num_motions must be 1" in L.svt_hip_last_error(hip.h)
    finally:
        hip.free(d)
