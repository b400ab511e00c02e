"""Times the global-motion front half on resident planes (HIP events around back-to-back calls, windows of at least --window ms): svt_hip_gm_corners_batch_dev
over the source and its references, svt_hip_gm_correspondences_batch_dev on the lists that call left on the device, and the chain of the two, at 1920x1080,
960x540 and 480x270 (the pictures the three gm_levels work on) with 1 and with 7 references, 4096 corners per plane at most.  Beside it the reference's
svt_av1_fast_corner_detect (once per plane) and svt_av1_determine_correspondence (once per reference) on the same arrays on this host, one thread: the C path
of oracle/_ref/libsvtav1_ref.so, whose results the device's are checked against, and the x86 kernels of libsvtav1_ref_simd.so.
    python tools/gm_front_time.py [--window 150] [--sizes 1920x1080,960x540,480x270]"""
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
import gm_front_common as f  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=150.0, help="least length of a timed window, ms")
ap.add_argument("--sizes", default="1920x1080,960x540,480x270")
args = ap.parse_args()
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
cref = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libsvtav1_ref.so"))
cref.setup_common_rtcd_internal(0); cref.setup_rtcd_internal(0)
simd = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libsvtav1_ref_simd.so"))
simd.refb_setup.restype = C.c_uint64; simd.refb_setup.argtypes = [C.c_uint64]
simd.refb_setup(0xFFFFFFFFFFFFFFFF)
per_call = lambda fn: hip.timed(fn, args.window)[0]
ONE = g.ONE
TRUTH = (3 * ONE + 8192, -2 * ONE - 4096, ONE + 160, 96, -96, ONE + 160)
MAXP = pkg.GM_MAX_CORNERS


def host(lib, src, ref, n_refs):
    """-> (ms of the corner detection of 1 + n_refs planes, ms of n_refs correspondence searches, the source's corners, the reference's, the correspondences)"""
    t0 = time.perf_counter()
    sp = f.ref_corners(lib, src)
    rp = [f.ref_corners(lib, ref) for _ in range(n_refs)]
    t1 = time.perf_counter()
    out = [f.ref_correspondences(lib, src, sp, ref, rp[0]) for _ in range(n_refs)]
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, sp, rp[0], out[0]


for size in args.sizes.split(","):
    w, h = (int(v) for v in size.split("x"))
    src, ref = g.picture_pair(7, w, h, TRUTH, margin=64)
    d_src, d_ref = hip.to_device(src), hip.to_device(ref)
    for n_refs in (1, 7):
        n = 1 + n_refs
        tab = (pkg.GmRef * (1 + pkg.GM_MAX_REFS))()
        tab[0] = pkg.GmRef(d_src, w, h, w, 0)
        for i in range(n_refs):
            tab[1 + i] = pkg.GmRef(d_ref, w, h, w, 0)
        rtab = (pkg.GmRef * pkg.GM_MAX_REFS)(*[tab[1 + i] for i in range(n_refs)])
        d_p, d_c, d_k = hip.empty(n * MAXP * 8), hip.empty(n * 4), hip.empty(n * 4)
        d_x = hip.empty(L.svt_hip_gm_corners_scratch_bytes(tab, n))
        d_o, d_n = hip.empty(n_refs * MAXP * 16), hip.empty(n_refs * 4)
        d_rp, d_rc = C.c_void_p(d_p.value + MAXP * 8), C.c_void_p(d_c.value + 4)
        corners = lambda: hip.check(L.svt_hip_gm_corners_batch_dev(hip.h, tab, n, MAXP, d_p, d_c, d_k, d_x), "gm_corners_batch")
        match = lambda: hip.check(L.svt_hip_gm_correspondences_batch_dev(hip.h, d_src, w, w, h, d_p, d_c, rtab, n_refs, d_rp, d_rc, MAXP, d_o, d_n),
                                  "gm_correspondences_batch")

        def chain():
            corners(); match()

        t_corners = per_call(corners)
        t_match = per_call(match)
        t_chain = per_call(chain)
        cnt, kept, ncorr = hip.to_host(d_c, (n,), np.int32), hip.to_host(d_k, (n,), np.int32), hip.to_host(d_n, (n_refs,), np.int32)
        pts, corr = hip.to_host(d_p, (n, MAXP, 2), np.int32), hip.to_host(d_o, (n_refs, MAXP, 4), np.int32)
        c_corners, c_match, sp, rp, want = host(cref, src, ref, n_refs)
        s_corners, s_match, _, _, swant = host(simd, src, ref, n_refs)
        same = (np.array_equal(pts[0, :cnt[0]], sp) and all(np.array_equal(pts[1 + i, :cnt[1 + i]], rp) and np.array_equal(corr[i, :ncorr[i]], want)
                                                            for i in range(n_refs)))
        print(f"{w}x{h} {n_refs} reference(s): corners {t_corners:8.3f} ms  correspondences {t_match:8.3f} ms  chain {t_chain:8.3f} ms per call   "
              f"corners kept {int(kept[0])} / {int(kept[1])} (lists of {int(cnt[0])} / {int(cnt[1])}), {int(ncorr[0])} correspondences per reference   "
              f"CPU, 1 thread: C path corners {c_corners:8.1f} ms, correspondences {c_match:8.1f} ms; x86 kernels corners {s_corners:8.1f} ms, correspondences "
              f"{s_match:8.1f} ms   results {'equal' if same else 'DIFFER'} to the C path, x86 kernels {'equal' if np.array_equal(want, swant) else 'DIFFER'}", flush=True)
        hip.free(d_p, d_c, d_k, d_x, d_o, d_n)
    hip.free(d_src, d_ref)
hip.close()
