"""Times svt_hip_cfl_predict_batch_dev and svt_hip_filter_intra_predict_batch_dev on a 3840x2160 4:2:0 8-bit picture (HIP events around back-to-back launches
on resident planes, windows of at least --window ms), and svt_hip_subpel_predict_batch_dev on the same luma plane for comparison:
  - the chroma planes tiled with 8x8 CfL blocks, both planes, in place and with dc_from_edges; the same with 16x16 blocks (1920x1072 of the 1920x1080 planes);
  - the luma plane tiled with 16x16 and with 4x4 filter-intra blocks;
  - the luma plane tiled with 16x16 sub-pel blocks (subpel_predict_kernel), the HBM -> LDS -> HBM stage these kernels resemble most.
GB/s are ALGORITHMIC bytes over the time of a call: what the job list has to read and write once (luma areas, chroma blocks read in place and written, the edge
samples a job uses, the job descriptors), not what the memory system moved.
    python tools/intra_cfl_time.py [--window 150]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402
import intra_common as ic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=150.0, help="least length of a timed window, ms")
args = ap.parse_args()
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
W, H = 3840, 2160
CW, CH = W // 2, H // 2
rng = np.random.default_rng(5)
luma = ic.mixed_frame(W, H)[:H, :W]
d_luma = hip.to_device(luma)
d_cb, d_cr = hip.to_device(rng.integers(0, 256, (CH, CW)).astype(np.uint8)), hip.to_device(rng.integers(0, 256, (CH, CW)).astype(np.uint8))
d_dst = hip.empty(W * H)
NREC = 4096   # a pool of edge records shared by the jobs
d_edges = hip.to_device(rng.integers(0, 256, (NREC, 2, 160)).astype(np.uint8))


def report(name, fn, nbytes, njobs):
    t, window, reps = hip.timed(fn, args.window, warm=5, reps=20)   # this tool has always warmed five times and started at 20 launches
    print(f"{name:44s} {t * 1e3:9.1f} us per call  {njobs:7d} jobs  {nbytes / 1e6:7.2f} MB algorithmic -> {nbytes / t / 1e6:8.1f} GB/s  (window {window:.0f} ms, {reps} launches)",
          flush=True)


def device_jobs(arr):
    d = hip.empty(C.sizeof(arr))
    hip.check(L.svt_hip_memcpy_h2d(hip.h, d, C.cast(arr, C.c_void_p), C.sizeof(arr)), "h2d")
    return d


for tw, tx in ((8, 1), (16, 2)):
    tiles = [(x, y) for y in range(0, CH - tw + 1, tw) for x in range(0, CW - tw + 1, tw)]
    for dc in (0, 1):
        arr = (pkg.CflJob * len(tiles))()
        for i, (J, (x, y)) in enumerate(zip(arr, tiles)):
            J.luma_x, J.luma_y, J.dst_x, J.dst_y, J.tx_size, J.plane_mask, J.dc_from_edges, J.dc_have = 2 * x, 2 * y, x, y, tx, 3, dc, 3
            J.alpha_q3[0], J.alpha_q3[1] = (i % 33) - 16, ((i * 7) % 33) - 16
            J.edge_off[0], J.edge_off[1] = (i % NREC) * 320, ((i + 1) % NREC) * 320
        d_jobs = device_jobs(arr)
        n = len(tiles)
        # luma area + per plane (block read unless the DC comes from 2 tw edge samples) + block written, + the descriptor
        nbytes = n * (4 * tw * tw + 2 * ((0 if dc else tw * tw) + (2 * tw if dc else 0) + tw * tw) + C.sizeof(pkg.CflJob))
        report(f"cfl {tw}x{tw} chroma blocks, {'dc_from_edges' if dc else 'in place'}",
               lambda d_jobs=d_jobs, n=n: hip.check(L.svt_hip_cfl_predict_batch_dev(hip.h, 1, 8, d_luma, W, d_edges, d_jobs, n, d_cb, d_cr, CW, None), "cfl"), nbytes, n)
        hip.free(d_jobs)

for tw, tx in ((16, 2), (4, 0)):
    tiles = [(x, y) for y in range(0, H, tw) for x in range(0, W, tw)]
    arr = (pkg.FilterIntraJob * len(tiles))()
    for i, (J, (x, y)) in enumerate(zip(arr, tiles)):
        J.edge_off, J.dst_x, J.dst_y, J.tx_size, J.mode = (i % NREC) * 320, x, y, tx, i % 5
    d_jobs = device_jobs(arr)
    n = len(tiles)
    nbytes = n * ((2 * tw + 1) + tw * tw + C.sizeof(pkg.FilterIntraJob))
    report(f"filter-intra {tw}x{tw} luma blocks",
           lambda d_jobs=d_jobs, n=n: hip.check(L.svt_hip_filter_intra_predict_batch_dev(hip.h, 1, 8, d_edges, d_jobs, n, d_dst, W), "filter-intra"), nbytes, n)
    hip.free(d_jobs)

# the comparison: 16x16 sub-pel blocks over the same luma plane (padded by 32), random fractional positions within +-8 samples
PAD = 32
refp = np.ascontiguousarray(np.pad(luma, PAD, mode="edge"))
d_refp = hip.to_device(refp)
n16 = (W // 16) * (H // 16)
CB = (pkg.ConvBlk * n16)()
k = 0
for by in range(0, H, 16):
    for bx in range(0, W, 16):
        CB[k] = pkg.ConvBlk(bx + int(rng.integers(-8, 9)), by + int(rng.integers(-8, 9)), bx, by, 16, 16, 0, 0, int(rng.integers(0, 16)), int(rng.integers(0, 16)), 0, 0)
        k += 1
d_cbk = device_jobs(CB)
report("subpel_predict 16x16 luma blocks (8-tap window)",
       lambda: hip.check(L.svt_hip_subpel_predict_batch_dev(hip.h, 1, 8, d_refp.value + PAD * refp.shape[1] + PAD, refp.shape[1], d_dst, W, d_cbk, n16), "subpel"),
       n16 * (23 * 23 + 256 + C.sizeof(pkg.ConvBlk)), n16)
hip.free(d_luma, d_cb, d_cr, d_dst, d_edges, d_refp, d_cbk)
hip.close()
