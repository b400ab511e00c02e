"""Times the super-resolution kernels (HIP events around back-to-back calls on resident planes, windows of at least --window ms): the normative upscale
(svt_hip_superres_upscale_planes_dev) of a 4:2:0 picture whose coded width is width * 8 / denom, at denominators 9, 12 and 16, and the downscale of the
full-width picture to that coded width (svt_hip_resize_planes_dev, width alone, as super-resolution scales), three planes per call, in 8-bit samples and in
16-bit samples at bit depth 10.  Beside each time: a device-to-device copy of the same bytes in plus bytes out (svt_hip_memcpy_d2d of (in + out) / 2 bytes:
it reads and writes that many), measured in the same run, and the ratio.  The kernels are memory-bound; that copy is the yardstick.
    python tools/superres_time.py [--window 100] [--size 3840x2160] [--denoms 9,12,16]"""
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
ap.add_argument("--denoms", default="9,12,16")
args = ap.parse_args()
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
W, H = (int(v) for v in args.size.split("x"))
per_call = lambda fn: hip.timed(fn, args.window)[0]

for dtype, bd in ((np.uint8, 8), (np.uint16, 10)):
    pix = np.dtype(dtype).itemsize
    full = [(W, H), ((W + 1) // 2, (H + 1) // 2), ((W + 1) // 2, (H + 1) // 2)]
    d_full = [hip.to_device(np.random.default_rng(i).integers(0, 1 << bd, (h, w)).astype(dtype)) for i, (w, h) in enumerate(full)]
    d_back = [hip.empty(w * h * pix) for w, h in full]
    for denom in (int(v) for v in args.denoms.split(",")):
        small = [(L.svt_hip_superres_scaled_dim(W, denom) + s) >> s for s in (0, 1, 1)]
        d_small = [hip.empty(sw * h * pix) for sw, (_, h) in zip(small, full)]
        down = (pkg.ResizePlane * 3)(*[pkg.ResizePlane(d_full[i], full[i][0], full[i][0], full[i][1], d_small[i], small[i], small[i], full[i][1]) for i in range(3)])
        up = (pkg.UpscalePlane * 3)(*[pkg.UpscalePlane(d_small[i], small[i], small[i], d_back[i], full[i][0], full[i][0], full[i][1]) for i in range(3)])
        assert L.svt_hip_resize_scratch_bytes(pix, down, 3) == 0
        nbytes = sum((sw + w) * h * pix for sw, (w, h) in zip(small, full))   # bytes in + bytes out, the same for both directions
        d_a, d_b = hip.empty(nbytes // 2), hip.empty(nbytes // 2)
        t_down = per_call(lambda: hip.check(L.svt_hip_resize_planes_dev(hip.h, pix, bd, down, 3, None, 0), "resize_planes"))
        t_up = per_call(lambda: hip.check(L.svt_hip_superres_upscale_planes_dev(hip.h, pix, bd, up, 3), "superres_upscale_planes"))
        t_copy = per_call(lambda: hip.check(L.svt_hip_memcpy_d2d(hip.h, d_a, d_b, nbytes // 2), "d2d"))
        print(f"{W}x{H} 4:2:0 {8 * pix:2d}-bit samples bd {bd:2d} denom {denom:2d} (coded width {small[0]}): upscale {t_up * 1e3:7.1f} us ({t_up / t_copy:4.2f} x copy)  "
              f"downscale {t_down * 1e3:7.1f} us ({t_down / t_copy:4.2f} x copy)  copy of {nbytes / 1e6:.1f} MB in + out {t_copy * 1e3:7.1f} us "
              f"({nbytes / t_copy / 1e6:.0f} GB/s)", flush=True)
        hip.free(d_a, d_b, *d_small)
    hip.free(*d_full, *d_back)
hip.close()
