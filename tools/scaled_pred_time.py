"""Times the scaled-reference predictor (HIP events around back-to-back calls on resident planes, windows of at least --window ms):
svt_hip_scaled_predict_batch_dev on every 16 x 16 block of a luma plane, single reference, at steps 1024 / 1152 / 1536 / 2048 -- x scaled alone (what
super-resolution produces) and both axes -- in 8-bit samples and in 16-bit samples at bit depth 10.  Block (bx, by) reads at its own position times the
scale plus a 5/16-sample phase, so both passes filter.  From the same run: svt_hip_subpel_predict_batch_dev (the unscaled predictor, conv.hip) on the same block
list at the same phase, and a device-to-device copy of the bytes a prediction needs (svt_hip_memcpy_d2d of (samples read + pixels written) / 2 bytes: it reads
and writes that many).  The ratio to the unscaled predictor at step 1024 says what the per-sample phase costs.
    python tools/scaled_pred_time.py [--window 100] [--size 3840x2160] [--steps 1024,1152,1536,2048]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=100.0, help="least length of a timed window, ms")
ap.add_argument("--size", default="3840x2160")
ap.add_argument("--steps", default="1024,1152,1536,2048")
args = ap.parse_args()
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
W, H = (int(v) & ~15 for v in args.size.split("x"))
BORDER, PHASE = 8, 5 << 6
per_call = lambda fn: hip.timed(fn, args.window)[0]
bx, by = np.meshgrid(np.arange(W // 16), np.arange(H // 16))
bx, by, n = bx.ravel(), by.ravel(), (W // 16) * (H // 16)


def scaled_jobs(xs, ys):
    j = np.zeros(n, np.dtype(pkg.ScaledBlk))
    qx, qy = bx * 16 * xs + PHASE, by * 16 * ys + PHASE
    j["pos0_x"], j["pos0_y"], j["subpel0_x"], j["subpel0_y"] = BORDER + (qx >> 10), BORDER + (qy >> 10), qx & 1023, qy & 1023
    j["xs0"], j["ys0"], j["dst_x"], j["dst_y"], j["w"], j["h"] = xs, ys, bx * 16, by * 16, 16, 16
    return j


def unscaled_jobs():
    j = np.zeros(n, np.dtype(pkg.ConvBlk))
    j["src_x"], j["src_y"], j["dst_x"], j["dst_y"], j["w"], j["h"] = BORDER + bx * 16, BORDER + by * 16, bx * 16, by * 16, 16, 16
    j["subpel_x"] = j["subpel_y"] = PHASE >> 6
    return j


for dtype, bd in ((np.uint8, 8), (np.uint16, 10)):
    pix = np.dtype(dtype).itemsize
    smax = max(int(v) for v in args.steps.split(","))
    rw, rh = ((W * smax) >> 10) + 2 * BORDER + 16, ((H * smax) >> 10) + 2 * BORDER + 16       # the largest reference; smaller steps read its top-left part
    d_ref = hip.to_device(np.random.default_rng(bd).integers(0, 1 << bd, (rh, rw)).astype(dtype))
    d_dst, d_conv = hip.empty(W * H * pix), hip.to_device(unscaled_jobs())
    t_conv = per_call(lambda: hip.check(L.svt_hip_subpel_predict_batch_dev(hip.h, pix, bd, d_ref, rw, d_dst, W, d_conv, n), "subpel_predict_batch"))
    print(f"{W}x{H} luma, {n} blocks of 16x16, {8 * pix:2d}-bit samples bd {bd:2d}: unscaled predictor (svt_hip_subpel_predict_batch_dev) {t_conv * 1e3:7.1f} us", flush=True)
    for step in (int(v) for v in args.steps.split(",")):
        for xs, ys in ((step, 1024), (step, step)) if step != 1024 else ((1024, 1024),):
            d_jobs = hip.to_device(scaled_jobs(xs, ys))
            nbytes = (((W * xs) >> 10) * ((H * ys) >> 10) + W * H) * pix                       # samples read once + pixels written
            d_a, d_b = hip.empty(nbytes // 2), hip.empty(nbytes // 2)
            t = per_call(lambda: hip.check(L.svt_hip_scaled_predict_batch_dev(hip.h, pix, bd, d_ref, rw, None, 0, d_dst, W, d_jobs, n), "scaled_predict_batch"))
            t_copy = per_call(lambda: hip.check(L.svt_hip_memcpy_d2d(hip.h, d_a, d_b, nbytes // 2), "d2d"))
            print(f"  steps {xs:4d} x {ys:4d}: scaled predictor {t * 1e3:7.1f} us = {t / t_conv:4.2f} x unscaled, {t / t_copy:5.2f} x copy of {nbytes / 1e6:5.1f} MB in + out "
                  f"({t_copy * 1e3:6.1f} us, {nbytes / t_copy / 1e6:.0f} GB/s)", flush=True)
            hip.free(d_a, d_b, d_jobs)
    hip.free(d_ref, d_dst, d_conv)
hip.close()
