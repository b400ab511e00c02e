"""CPU: the entry points of the global-motion model fit, the decision and the picture call have their Context methods and the header cites the reference (declarations, exports, prototypes and layouts: tests/test_abi_binding.py), and calls
the host can see to be wrong are refused with SVT_HIP_ERR_BAD_ARG before anything touches HIP (no device exists here).  The same bad arguments with a live context
are checked in tests/test_gm_fit_gpu.py and tests/test_gm_estimate_gpu.py."""
import ctypes as C
import os
import re

from conftest import ROOT

BAD_ARG = 2   # SVT_HIP_ERR_BAD_ARG


def _header():
    return open(os.path.join(ROOT, "include", "svt_hip.h")).read()


def test_declared_exported_bound(pkg):
    hdr = _header()
    for m in ("gm_fit_batch", "gm_estimate_picture"):
        assert hasattr(pkg.Context, m)
    assert int(re.search(r"#define SVT_HIP_GM_FIT_MAX_JOBS (\d+)", hdr).group(1)) == pkg.GM_FIT_MAX_JOBS
    assert C.sizeof(pkg.GmFit) % 8 == 0 and C.sizeof(pkg.GmFit) == 120
    # the header no longer says that the fit stays on the host, and cites the reference's lines
    assert not re.search(r"RANSAC[^.;]*stays? on the host", hdr) and "RANSAC takes the" not in hdr
    assert "ransac.c:359-542" in hdr and "EbGlobalMotionEstimation.c:303-399" in hdr


def test_scratch_sizes(pkg):
    L = pkg.lib()
    fit = L.svt_hip_gm_fit_scratch_bytes
    assert fit(1, 4096) == 20 * 4096 * 8 and fit(16, 4096) == 16 * fit(1, 4096) and fit(3, 200) == 3 * 20 * 200 * 8 and fit(0, 4096) == 0
    # what the call would refuse has no size
    assert fit(-1, 4096) == 0 and fit(65, 4096) == 0 and fit(1, 0) == 0 and fit(1, 4097) == 0

    def est(w, h, n, rz=0, mp=4096, nr=5):
        return L.svt_hip_gm_estimate_scratch_bytes(w, h, n, C.byref(pkg.GmEstimateOptions(rz, 0, nr, mp)))

    one = est(352, 288, 1)
    assert one >= 2 * 352 * 288 + 2 * fit(1, 4096) + 4096 * 4 * 4 and one % 256 == 0
    assert est(352, 288, 8) > 4 * one and est(352, 288, 1, rz=1) < one and est(352, 288, 1, mp=256) < est(352, 288, 1, rz=1)
    assert est(7, 288, 1) == 0 and est(352, 16385, 1) == 0 and est(352, 288, 0) == 0 and est(352, 288, 9) == 0 and est(352, 288, 1, mp=0) == 0
    assert est(352, 288, 1, mp=4097) == 0 and est(352, 288, 1, nr=13) == 0 and est(352, 288, 1, nr=-1) == 0 and L.svt_hip_gm_estimate_scratch_bytes(352, 288, 1, None) == 0


# one thing wrong at a time; shared with the GPU tests, which repeat them with a live context.  1 = "a valid pointer"
FIT_OK = dict(d_corr=1, d_ncorr=1, n_lists=2, max_points=4096, jobs=1, njobs=3, num_motions=1, n_refinements=5, d_fits=1, d_inliers=1, d_refine_jobs=1, d_scratch=1,
              ref=1, type=2)
FIT_BAD = [dict(d_corr=None), dict(d_ncorr=None), dict(jobs=None), dict(d_fits=None), dict(d_scratch=None), dict(n_lists=0), dict(n_lists=9), dict(max_points=0),
           dict(max_points=4097), dict(njobs=-1), dict(njobs=65), dict(num_motions=0), dict(num_motions=2), dict(n_refinements=-1), dict(n_refinements=13),
           dict(ref=-1), dict(ref=2), dict(type=0), dict(type=4), dict(scratch_off=4)]
EST_OK = dict(d_src=1, stride=96, w=96, h=80, refs=1, n_refs=2, options=1, results=1, d_scratch=1, ref_plane=1, ref_w=96, ref_h=80, ref_stride=100, max_points=4096,
              n_refinements=5)
EST_BAD = [dict(d_src=None), dict(refs=None), dict(options=None), dict(results=None), dict(d_scratch=None), dict(ref_plane=None), dict(n_refs=0), dict(n_refs=9),
           dict(w=7), dict(h=7), dict(w=16385, stride=16385, ref_w=16385, ref_stride=16385), dict(stride=95), dict(ref_stride=95), dict(ref_w=95), dict(ref_h=79),
           dict(max_points=0), dict(max_points=4097), dict(n_refinements=-1), dict(n_refinements=13), dict(scratch_off=8)]


def _q(a, p):
    return lambda k: p if a[k] == 1 else a[k]


def call_fit(pkg, L, ctx, p, **chg):
    """`p` stands in for every pointer that is 1 in the OK set (256-byte aligned)"""
    a = dict(FIT_OK); a.update(chg); q = _q(a, p)
    tab = (pkg.GmFitJob * 64)(*[pkg.GmFitJob(a["ref"], a["type"]) for _ in range(64)])
    scratch = q("d_scratch")
    if scratch is not None:
        scratch += a.get("scratch_off", 0)
    return L.svt_hip_gm_fit_batch_dev(ctx, q("d_corr"), q("d_ncorr"), a["n_lists"], a["max_points"], tab if a["jobs"] == 1 else None, a["njobs"], a["num_motions"],
                                      a["n_refinements"], q("d_fits"), q("d_inliers"), q("d_refine_jobs"), scratch)


def call_estimate(pkg, L, ctx, p, **chg):
    a = dict(EST_OK); a.update(chg); q = _q(a, p)
    tab = (pkg.GmRef * 9)()
    for i in range(9):
        tab[i] = pkg.GmRef(q("ref_plane"), a["ref_w"], a["ref_h"], a["ref_stride"], 0)
    opt = pkg.GmEstimateOptions(0, 0, a["n_refinements"], a["max_points"])
    out = (pkg.GmEstimate * 9)()
    scratch = q("d_scratch")
    if scratch is not None:
        scratch += a.get("scratch_off", 0)
    return L.svt_hip_gm_estimate_picture_dev(ctx, q("d_src"), a["stride"], a["w"], a["h"], tab if a["refs"] == 1 else None, a["n_refs"],
                                             C.byref(opt) if a["options"] == 1 else None, out if a["results"] == 1 else None, scratch)


def test_null_context_and_bad_arguments_are_refused(pkg):
    L = pkg.lib()
    buf = (C.c_uint8 * 8192)()
    p = (C.cast(buf, C.c_void_p).value + 255) & ~255
    for c in [{}] + FIT_BAD:
        assert call_fit(pkg, L, None, p, **c) == BAD_ARG, c
    for c in [{}] + EST_BAD:
        assert call_estimate(pkg, L, None, p, **c) == BAD_ARG, c
    assert L.svt_hip_gm_decide_host(None, 0, 0, 0, None, None) == BAD_ARG
    assert L.svt_hip_gm_params_cost_host(None, 2, 0) == -1 and L.svt_hip_gm_params_cost_host((C.c_int32 * 8)(), 4, 0) == -1
