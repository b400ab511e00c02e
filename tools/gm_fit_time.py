"""Times the global-motion model fit and the picture call on resident planes (HIP events around back-to-back calls, windows of at least --window ms), at
1920x1080, 960x540 and 480x270 with 1 and with 7 references, 4096 corners per plane at most, 5 refinements, ROTZOOM and AFFINE per reference:
  fit      svt_hip_gm_fit_batch_dev alone, on the lists the correspondence call left on the device
  picture  svt_hip_gm_estimate_picture_dev, the whole call (its own synchronisations and the host decision included)
  3 calls  the way without the device fit: corners + correspondences on the device, the lists downloaded, the reference's fit functions and
           svt_av1_convert_model_to_params on this host (one thread, through ctypes), jobs uploaded, svt_hip_gm_refine_picture_dev, the frame errors,
           svt_hip_gm_decide_host -- same inputs, downloads and uploads included
  CPU      the reference's own path on this host, one thread, C path of oracle/_ref/libsvtav1_ref.so: corners of the source, then per model type
           svt_av1_compute_global_motion and svt_av1_refine_integerized_param, for ONE reference (wall clock, one run), times the number of references
    python tools/gm_fit_time.py [--window 150] [--sizes 1920x1080,960x540,480x270]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402
import gm_common as g  # noqa: E402
import gm_fit_common as fc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=150.0, help="least length of a timed window, ms")
ap.add_argument("--sizes", default="1920x1080,960x540,480x270")
args = ap.parse_args()
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
cref = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libsvtav1_ref.so"))
cref.setup_common_rtcd_internal(0); cref.setup_rtcd_internal(0)
per_call = lambda fn: hip.timed(fn, args.window)[0]
ONE = g.ONE
TRUTH = (3 * ONE + 8192, -2 * ONE - 4096, ONE + 160, 96, -96, ONE + 160)
MAXP = pkg.GM_MAX_CORNERS
N_REF = 5


for size in args.sizes.split(","):
    w, h = (int(v) for v in size.split("x"))
    src, ref = g.picture_pair(7, w, h, TRUTH, margin=64)
    d_src, d_ref = hip.to_device(src), hip.to_device(ref)
    for n_refs in (1, 7):
        n, njobs = 1 + n_refs, 2 * n_refs
        tab = (pkg.GmRef * (1 + pkg.GM_MAX_REFS))()
        tab[0] = pkg.GmRef(d_src, w, h, w, 0)
        for i in range(n_refs):
            tab[1 + i] = pkg.GmRef(d_ref, w, h, w, 0)
        rtab = (pkg.GmRef * pkg.GM_MAX_REFS)(*[tab[1 + i] for i in range(n_refs)])
        d_p, d_c = hip.empty(n * MAXP * 8), hip.empty(n * 4)
        d_x = hip.empty(L.svt_hip_gm_corners_scratch_bytes(tab, n))
        d_o, d_n = hip.empty(n_refs * MAXP * 16), hip.empty(n_refs * 4)
        d_rp, d_rc = C.c_void_p(d_p.value + MAXP * 8), C.c_void_p(d_c.value + 4)
        d_fits, d_jobs, d_res = hip.empty(njobs * C.sizeof(pkg.GmFit)), hip.empty(njobs * C.sizeof(pkg.GmJob)), hip.empty(njobs * C.sizeof(pkg.GmResult))
        d_fx, d_rx = hip.empty(L.svt_hip_gm_fit_scratch_bytes(njobs, MAXP)), hip.empty(L.svt_hip_gm_refine_scratch_bytes(njobs))
        d_fe = hip.empty(n_refs * 8)
        opt = pkg.GmEstimateOptions(0, 0, N_REF, MAXP)
        d_ex = hip.empty(L.svt_hip_gm_estimate_scratch_bytes(w, h, n_refs, C.byref(opt)))
        est = (pkg.GmEstimate * n_refs)()
        fit_jobs = (pkg.GmFitJob * njobs)(*[pkg.GmFitJob(r, t) for r in range(n_refs) for t in (fc.ROTZOOM, fc.AFFINE)])

        def front():
            hip.check(L.svt_hip_gm_corners_batch_dev(hip.h, tab, n, MAXP, d_p, d_c, None, d_x), "gm_corners_batch")
            hip.check(L.svt_hip_gm_correspondences_batch_dev(hip.h, d_src, w, w, h, d_p, d_c, rtab, n_refs, d_rp, d_rc, MAXP, d_o, d_n), "gm_correspondences_batch")

        fit = lambda: hip.check(L.svt_hip_gm_fit_batch_dev(hip.h, d_o, d_n, n_refs, MAXP, fit_jobs, njobs, 1, N_REF, d_fits, None, d_jobs, d_fx), "gm_fit_batch")
        picture = lambda: hip.check(L.svt_hip_gm_estimate_picture_dev(hip.h, d_src, w, w, h, rtab, n_refs, C.byref(opt), est, d_ex), "gm_estimate_picture")
        three_out = [None] * n_refs

        def three_calls():
            front()
            hip.check(L.svt_hip_sync(hip.h), "sync")
            corr, cnt = hip.to_host(d_o, (n_refs, MAXP, 4), np.int32), hip.to_host(d_n, (n_refs,), np.int32)
            jobs, fits = (pkg.GmJob * njobs)(), []
            for r in range(n_refs):
                for m, t in enumerate((fc.ROTZOOM, fc.AFFINE)):
                    ft = fc.ref_fit_points(cref, corr[r, :cnt[r]], t)
                    fits.append(ft)
                    skip = ft["num_inliers_kept"] == 0 or ft["wmtype"] == 0
                    jobs[2 * r + m] = pkg.GmJob(r, -1 if skip else ft["wmtype"], (C.c_int32 * 8)(*ft["wmmat"]), N_REF, 0, g.INT64_MAX)
            hip.check(L.svt_hip_memcpy_h2d(hip.h, d_jobs, C.cast(jobs, C.c_void_p), C.sizeof(jobs)), "h2d")
            hip.check(L.svt_hip_gm_frame_error_batch_dev(hip.h, d_src, w, w, h, rtab, n_refs, d_fe), "gm_frame_error_batch")
            hip.check(L.svt_hip_gm_refine_picture_dev(hip.h, d_src, w, w, h, rtab, n_refs, d_jobs, njobs, d_res, d_rx, None), "gm_refine_picture")
            res = (pkg.GmResult * njobs)()
            hip.check(L.svt_hip_memcpy_d2h(hip.h, C.cast(res, C.c_void_p), d_res, C.sizeof(res)), "d2h")
            fe = hip.to_host(d_fe, (n_refs,), np.int64)
            for r in range(n_refs):
                recs = (pkg.GmModelRecord * 2)()
                for m in range(2):
                    j = 2 * r + m
                    recs[m] = pkg.GmModelRecord(fits[j]["num_inliers_kept"], fits[j]["wmtype"], res[j].wmmat, res[j].wmtype, 0, res[j].best_error)
                wm, wt = (C.c_int32 * 8)(), C.c_int32()
                L.svt_hip_gm_decide_host(recs, int(fe[r]), 0, 0, wm, C.byref(wt))
                three_out[r] = (list(wm), wt.value)

        front()
        t_fit = per_call(fit)
        t_picture = per_call(picture)
        t_three = per_call(three_calls)
        t0 = time.perf_counter()
        want = fc.ref_estimate(cref, src, ref, 0, 0, N_REF)
        t_cpu = (time.perf_counter() - t0) * 1e3 * n_refs
        same = all((list(est[r].wmmat), est[r].wmtype) == (want["wmmat"], want["wmtype"]) == three_out[r] for r in range(n_refs))
        ncorr = hip.to_host(d_n, (n_refs,), np.int32)
        print(f"{w}x{h} {n_refs} reference(s): fit {t_fit:8.3f} ms  picture {t_picture:8.3f} ms  3 calls + host fit {t_three:8.3f} ms per call   "
              f"CPU, 1 thread, C path {t_cpu:9.1f} ms   {int(ncorr[0])} correspondences per reference, model type {want['wmtype']}, "
              f"inliers {[r['num_inliers_kept'] for r in want['records']]}   results {'equal' if same else 'DIFFER'}", flush=True)
        hip.free(d_p, d_c, d_x, d_o, d_n, d_fits, d_jobs, d_res, d_fx, d_rx, d_fe, d_ex)
    hip.free(d_src, d_ref)
hip.close()
