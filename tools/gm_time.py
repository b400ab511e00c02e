"""Times svt_hip_gm_refine_picture_dev (HIP events around back-to-back calls on resident planes, windows of at least --window ms; a call ends with the host's
last poll, so the figure is the time of whole calls): one ROTZOOM and one AFFINE walk from a near-miss start, at 1920x1080, 960x540 and 480x270 (the pictures the
three gm_levels refine on), with 1 and with 7 jobs per call (the same walk against 7 resident reference planes).  Prints ms per call, the probes the reference
would evaluate, the device rounds and the host polls, and beside it the same walk by svt_av1_refine_integerized_param of oracle/_ref/libsvtav1_ref_simd.so (the
reference's x86 kernels on this host, one thread) on the same arrays, after checking that both end at the same parameters and error.
    python tools/gm_time.py [--window 150] [--sizes 1920x1080,960x540,480x270]"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=150.0, help="least length of a timed window, ms")
ap.add_argument("--sizes", default="1920x1080,960x540,480x270")
args = ap.parse_args()
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
simd = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libsvtav1_ref_simd.so"))
simd.refb_setup.restype = C.c_uint64; simd.refb_setup.argtypes = [C.c_uint64]
simd.refb_setup(0xFFFFFFFFFFFFFFFF)
g.prepare(simd)
ONE = g.ONE
TRUTH = (3 * ONE + 8192, -2 * ONE - 4096, ONE + 160, 96, -96, ONE + 160)
WALKS = [("ROTZOOM", g.ROTZOOM, (3 * ONE + 2048, -2 * ONE, ONE + 128, 64, 0, 0)), ("AFFINE", g.AFFINE, (3 * ONE + 2048, -2 * ONE, ONE + 128, 64, -64, ONE + 140))]
N_REF = 5


for size in args.sizes.split(","):
    w, h = (int(v) for v in size.split("x"))
    src, ref = g.picture_pair(7, w, h, TRUTH, margin=64)
    d_src, d_ref = hip.to_device(src), hip.to_device(ref)
    tab = (pkg.GmRef * pkg.GM_MAX_REFS)()
    for i in range(7):
        tab[i] = pkg.GmRef(d_ref, w, h, w, 0)
    for name, wmtype, start in WALKS:
        t0 = time.perf_counter()
        want = g.ref_refine(simd, start, wmtype, ref, src, N_REF)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        for njobs in (1, 7):
            jobs = (pkg.GmJob * njobs)()
            for i, j in enumerate(jobs):
                j.ref, j.wmtype, j.n_refinements, j.best_frame_error = i, wmtype, N_REF, g.INT64_MAX
                for k, v in enumerate(start): j.wmmat[k] = v
            with hip.scope() as s:
                d_jobs, d_out, d_x = s.structs(jobs), s.empty(njobs * C.sizeof(pkg.GmResult)), s.empty(L.svt_hip_gm_refine_scratch_bytes(njobs))
                polls = C.c_int()
                call = lambda: hip.call("gm_refine_picture_dev", d_src, w, w, h, tab, 7, d_jobs, njobs, d_out, d_x, C.byref(polls))
                t, window, reps = hip.timed(call, args.window)
                out = s.structs_back(d_out, pkg.GmResult * njobs)
            same = all((list(o.wmmat), o.wmtype, o.best_error) == want for o in out)
            print(f"{w}x{h} {name:8s} {njobs} job(s): {t:9.3f} ms per call  probes {out[0].probes:4d}  rounds {out[0].rounds:3d}  polls {polls.value}  "
                  f"(window {window:.0f} ms, {reps} calls)   CPU (x86 kernels, 1 thread) {cpu_ms:9.1f} ms per walk  results {'equal' if same else 'DIFFER'}", flush=True)
    hip.free(d_src, d_ref)
hip.close()
