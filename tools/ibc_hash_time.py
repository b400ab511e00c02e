"""Times the intra-block-copy hash table and hash search (HIP events around back-to-back calls on resident data, windows of at least --window ms).
  - svt_hip_ibc_hash_table_dev of a synthetic screen-like 8-bit picture (plain grounds, panels, text strokes, a gradient, a band of camera-like noise) and of a
    noise picture, at 1920x1080 and 3840x2160; the output states the work: positions hashed over all levels, entries, the largest bucket.
  - svt_hip_ibc_hash_search_batch_dev on that table for --jobs blocks spread evenly over the picture's 8x8, 16x16 and 64x64 grids, intra, limits open, one
    launch per size; the output states the entries compared and the candidates costed, which is what the time follows (a flat block of a screen picture shares
    its bucket with every other flat block on the grid).
  - The serial host forms (svt_hip_ibc_hash_table_host once, svt_hip_ibc_hash_search_host on --host-jobs of the jobs, scaled) on one thread: the only CPU figure
    available without the reference's structures; the reference's own serial pass adds a malloc-backed push_back per entry to the same arithmetic.
    python tools/ibc_hash_time.py [--window 100] [--jobs 4096] [--host-jobs 64] [--sizes 1920x1080,3840x2160]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402
import ibc_hash_common as I  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=100.0, help="least length of a timed window, ms")
ap.add_argument("--jobs", type=int, default=4096, help="blocks per size the device search is timed on")
ap.add_argument("--host-jobs", type=int, default=64, help="of those, the blocks the host form is timed on")
ap.add_argument("--sizes", default="1920x1080,3840x2160")
args = ap.parse_args()
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
per_call = lambda fn: hip.timed(fn, args.window)[0]


def screen_picture(w, h, seed):
    rng = np.random.default_rng(seed)
    pic = np.full((h, w), 240, np.int64)
    for _ in range(w * h // 20000):   # panels of one colour
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        pic[y:y + int(rng.integers(20, 300)), x:x + int(rng.integers(40, 500))] = int(rng.integers(0, 256))
    for _ in range(w * h // 150):     # text strokes in a few ink colours
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        pic[y:y + int(rng.integers(1, 3)), x:x + int(rng.integers(1, 9))] = (10, 30, 60, 200)[int(rng.integers(0, 4))]
    pic[h // 2:h // 2 + h // 8, :] = (np.arange(w) * 255 // w)[None, :]                               # a gradient
    pic[h - h // 6:, :] = np.clip(rng.normal(128, 30, (h // 6, w)), 0, 255).astype(np.int64)           # camera-like
    return pic.astype(np.uint8)


jc, cc = I.cost_tables()
d_jc, d_cc = hip.to_device(jc), hip.to_device(cc)
for size in args.sizes.split(","):
    W, H = (int(v) for v in size.split("x"))
    for kind, pic in (("screen", screen_picture(W, H, 1)), ("noise", I.noise(W, H))):
        cap, nbytes = int(L.svt_hip_ibc_hash_max_entries(W, H)), L.svt_hip_ibc_hash_scratch_bytes(W, H)
        d_pic, d_start, d_ent, d_info, d_scr = hip.to_device(pic), hip.empty((I.N_BUCKETS + 1) * 4), hip.empty(cap * 8), hip.empty(8), hip.empty(nbytes)
        t = per_call(lambda: hip.check(L.svt_hip_ibc_hash_table_dev(hip.h, 1, 8, d_pic, W, W, H, d_start, d_ent, cap, d_info, d_scr, nbytes), "ibc_hash_table"))
        n_entries, stored = hip.to_host(d_info, (2,), np.int32).tolist()
        start = hip.to_host(d_start, (I.N_BUCKETS + 1,), np.int32)
        positions = sum((W - s + 1) * (H - s + 1) for s in (2,) + I.SIZES)
        t0 = time.perf_counter(); h_start, h_ent, h_info = pkg.ibc_hash_table_host(pic); host = time.perf_counter() - t0
        same = bool((h_start == start).all() and (hip.to_host(d_ent, (n_entries,), I.ENTRY_DTYPE) == h_ent[:n_entries]).all())
        print(f"hash table {W}x{H} {kind:6s}: {t:8.3f} ms per call  {positions / 1e6:6.1f} M positions hashed (twice), {n_entries / 1e6:6.2f} M entries (stored {stored}), "
              f"largest bucket {int(np.diff(start).max())}, scratch {nbytes / 1e6:.0f} MB  | host form, one thread: {host * 1e3:8.1f} ms ({host / (t * 1e-3):5.0f} x), "
              f"tables {'equal' if same else 'DIFFER'}", flush=True)
        for n in (8, 16, 64):
            grid = [(x, y) for y in range(0, H - n + 1, n) for x in range(0, W - n + 1, n)]
            grid = grid[::max(1, len(grid) // args.jobs)][:args.jobs]
            jobs = [I.job(x, y, n, 1, limits=(-1023, 1023, -1023, 1023), w=W, h=H, log2=4) for x, y in grid]
            tab = I.c_jobs(pkg, jobs)
            with hip.scope() as s:
                d_jobs, d_res = s.structs(tab), s.empty(len(jobs) * C.sizeof(pkg.IbcSearchResult))
                t = per_call(lambda: hip.check(L.svt_hip_ibc_hash_search_batch_dev(hip.h, 1, 8, d_pic, W, W, H, d_start, d_ent, d_jc, d_cc, d_jobs, len(jobs), d_res),
                                               "ibc_hash_search"))
                res = s.download(d_res, (len(jobs), 7), np.int32)
            few = jobs[::max(1, len(jobs) // args.host_jobs)]
            t0 = time.perf_counter(); h_res = pkg.ibc_hash_search_host(pic, h_start, h_ent, jc, cc, I.c_jobs(pkg, few)); host = (time.perf_counter() - t0) * len(jobs) / len(few)
            step = max(1, len(jobs) // args.host_jobs)
            same = all([getattr(h_res[i], k) for k in I.RESULT_FIELDS] == res[i * step].tolist() for i in range(len(few)))
            print(f"  hash search {n:3d}x{n:<3d}: {t * 1e3:9.1f} us per launch  {len(jobs):5d} jobs, {int(np.maximum(res[:, 0], 0).sum()):9d} entries compared, "
                  f"{int(res[:, 2].sum()):9d} candidates costed, {int(res[:, 3].sum()):5d} found  | host form, one thread ({len(few)} jobs timed, scaled): {host * 1e3:9.1f} ms "
                  f"({host / (t * 1e-3):6.0f} x), results {'equal' if same else 'DIFFER'}", flush=True)
        hip.free(d_pic, d_start, d_ent, d_info, d_scr)
hip.free(d_jc, d_cc)
hip.close()
