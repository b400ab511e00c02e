"""Times the dual interpolation filter search on the device, svt_hip_ifs_search_batch_dev (HIP events around back-to-back calls on resident data, windows of at least
--window ms after two warm-up calls), next to the only other way the library has to do the same job: nine svt_hip_subpel_predict_batch_dev (one reference) or
svt_hip_compound_predict_batch_dev (two) launches, one per filter pair, each into a prediction plane of its own, plus nine svt_hip_block_sse_batch_dev launches, on the same
list.  The composition still lacks the model and the decision, a host pass that is not timed here, so its time is a lower bound.
  - Picture: a seeded 1920x1080 luma plane (low-pass noise and texture) as the reference, with a border of 32 samples; the source is the reference displaced by a
    sample with a little noise.  Three sample formats: 8-bit, 8-bit samples in 16-bit words, 10-bit.
  - Job lists, one launch each: every 16x16 block and every 32x32 block, with a random vector of up to 8 whole samples and random quarter-pel phases (q4 phase 0, 4, 8
    or 12 in either direction); one reference, and the average of two.  order 0, random rates.  The job list is uploaded by every call: that copy is part of its time.
  - The check: every candidate's sse of the fused call equals what the composition's block_sse gives.
    python tools/ifs_time.py [--window 100] [--size 1920x1080]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402
import ifs_common as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=100.0, help="least length of a timed window, ms")
ap.add_argument("--size", default="1920x1080")
args = ap.parse_args()
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
W, H = (int(v) for v in args.size.split("x"))
PAD = 32
BSIZE = {16: 6, 32: 9}
print(f"{W}x{H}, border {PAD}", flush=True)
for dtype, bd, name in ((np.uint8, 8, "8-bit"), (np.uint16, 8, "8-bit in 16-bit words"), (np.uint16, 10, "10-bit")):
    rng = np.random.default_rng(3)
    top = (1 << bd) - 1
    n0 = rng.standard_normal((H + 2 * PAD + 2, W + 2 * PAD + 2))
    for _ in range(3):
        n0 = (n0 + np.roll(n0, 1, 0) + np.roll(n0, 1, 1) + np.roll(n0, (1, 1), (0, 1))) / 4
    base = np.clip(np.rint((0.5 + 1.6 * n0) * top), 0, top).astype(np.int64)
    padded = [np.ascontiguousarray(base[1:-1, 1:-1].astype(dtype)), np.ascontiguousarray(base[2:, :-2].astype(dtype))]
    source = np.clip(base[1 + PAD:1 + PAD + H, 2 + PAD:2 + PAD + W] + rng.integers(-2, 3, (H, W)), 0, top).astype(dtype)
    pb, stride = source.itemsize, padded[0].shape[1]
    with hip.scope() as s:
        d_src = s.upload(source)
        d_pad = [s.upload(p) for p in padded]
        d_ref = [C.c_void_p(d.value + (PAD * stride + PAD) * pb) for d in d_pad]
        d_pred = [s.empty(W * H * pb) for _ in range(S.NCAND)]
        for b in (16, 32):
            cols, rows = W // b, H // b
            n = cols * rows
            for two in (False, True):
                jobs, pairs = [], (pkg.BlkPair * n)()
                for k in range(n):
                    x, y = (k % cols) * b, (k // cols) * b
                    ri = lambda lo, hi: int(rng.integers(lo, hi))
                    j = S.job(BSIZE[b], 0, 0, type=0 if two else -1, order=0, q=ri(8, 2000), lam=ri(100, 60000), rates=[[ri(0, 3000) for _ in range(3)] for _ in range(2)])
                    j.update(x=x, y=y, ref0_x=x + ri(-8, 9), ref0_y=y + ri(-8, 9), ref1_x=x + ri(-8, 9), ref1_y=y + ri(-8, 9), subpel0_x=4 * ri(0, 4), subpel0_y=4 * ri(0, 4),
                             subpel1_x=4 * ri(0, 4), subpel1_y=4 * ri(0, 4), dst_x=x, dst_y=y)
                    jobs.append(j)
                    pairs[k] = pkg.BlkPair(x, y, x, y, b, b)
                cj = S.c_jobs(pkg, jobs)
                d_res, d_cand, d_pairs, d_sse = s.empty(n * C.sizeof(pkg.IfsResult)), s.empty(n * S.NCAND * C.sizeof(pkg.IfsCand)), s.structs(pairs), s.empty(S.NCAND * n * 8)
                d_blks = []
                for fy, fx in S.FILTER_SETS:
                    if two:
                        blks = (pkg.CompBlk * n)(*[pkg.CompBlk(j["ref0_x"], j["ref0_y"], j["ref1_x"], j["ref1_y"], j["x"], j["y"], b, b, fx, fy, j["subpel0_x"], j["subpel0_y"],
                                                               j["subpel1_x"], j["subpel1_y"], 0, 8, 8, 0) for j in jobs])
                    else:
                        blks = (pkg.ConvBlk * n)(*[pkg.ConvBlk(j["ref0_x"], j["ref0_y"], j["x"], j["y"], b, b, fx, fy, j["subpel0_x"], j["subpel0_y"], 0, 0) for j in jobs])
                    d_blks.append(s.structs(blks))

                def fused(cand=True, dst=None):
                    hip.check(L.svt_hip_ifs_search_batch_dev(hip.h, pb, bd, d_src, W, W, H, d_ref[0], stride, d_ref[1] if two else None, stride, dst, W, C.cast(cj, C.c_void_p), n,
                                                             d_res, d_cand if cand else None), "ifs_search")

                def composed():
                    for i in range(S.NCAND):
                        if two:
                            hip.check(L.svt_hip_compound_predict_batch_dev(hip.h, pb, bd, d_ref[0], stride, d_ref[1], stride, d_pred[i], W, None, d_blks[i], n), "compound_predict")
                        else:
                            hip.check(L.svt_hip_subpel_predict_batch_dev(hip.h, pb, bd, d_ref[0], stride, d_pred[i], W, d_blks[i], n), "subpel_predict")
                        hip.check(L.svt_hip_block_sse_batch_dev(hip.h, pb, d_src, W, d_pred[i], W, d_pairs, n, C.c_void_p(d_sse.value + i * n * 8)), "block_sse")

                t_f, win_f, reps_f = hip.timed(lambda: fused(False), args.window)
                t_c, _, _ = hip.timed(fused, args.window)
                t_d, _, _ = hip.timed(lambda: fused(False, d_pred[0]), args.window)
                t_b, win_b, reps_b = hip.timed(composed, args.window)
                fused()
                hip.sync()
                cand = s.structs_back(d_cand, pkg.IfsCand * (S.NCAND * n))
                sse = s.download(d_sse, (S.NCAND, n), np.uint64)
                same = all(cand[k * S.NCAND + i].sse == int(sse[i, k]) for k in range(0, n, 7) for i in range(S.NCAND))
                print(f"  {name:22s} {b}x{b} {'average of two' if two else 'one reference'}: {n} jobs  fused {t_f:7.3f} ms (window {win_f:.0f} ms, {reps_f} calls; with "
                      f"candidate records {t_c:7.3f}, with the winner's prediction {t_d:7.3f})  |  9 + 9 launches {t_b:7.3f} ms (window {win_b:.0f} ms, {reps_b} calls)  |  "
                      f"ratio {t_b / t_f:5.2f}  |  sse {'equal' if same else 'DIFFER'}", flush=True)
hip.close()
