"""Times the palette luma search and the screen-content detection (HIP events around back-to-back launches on resident data, windows of at least --window ms).
  - svt_hip_palette_search_batch_dev for every whole 8x8, 16x16, 32x32 and 64x64 block of a synthetic 1920x1080 screen-like 8-bit picture (plain grounds, text
    strokes, flat panels, a gradient and a band of camera-like noise that the search leaves after the colour count), one launch per block size, no colour cache;
    the output states the work: jobs, blocks with 1 < colors <= 64 (the ones that cluster), candidates kept.
  - svt_hip_screen_content_detect_dev of a 3840x2160 plane of the same kind, at 8 and at 10 bits.
  - The same work on one host thread through the reference's own dispatch (svt_av1_count_colors, svt_av1_k_means_dim1 and svt_av1_calc_indices_dim1 as
    libsvtav1_ref_simd.so selects them for this CPU; is_valid_palette_nb_colors and svt_aom_variance16x16 for the detection), when oracle/_ref holds that library:
    the time spent inside those calls for a sample of the blocks (--host-blocks per size), scaled to all of them.  The glue between the calls is not counted.
    python tools/palette_time.py [--window 100] [--host-blocks 200]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402
import palette_common as P  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=100.0, help="least length of a timed window, ms")
ap.add_argument("--host-blocks", type=int, default=200, help="blocks per size the host path is timed on")
args = ap.parse_args()
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
per_call = lambda fn: hip.timed(fn, args.window)[0]


def screen_picture(w, h, bd, seed):
    rng = np.random.default_rng(seed)
    sc = 1 << (bd - 8)
    pic = np.full((h, w), 240 * sc, np.int64)
    for _ in range(w * h // 20000):   # panels of one colour
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        pic[y:y + int(rng.integers(20, 300)), x:x + int(rng.integers(40, 500))] = int(rng.integers(0, 256)) * sc
    for _ in range(w * h // 150):     # text strokes in a few ink colours
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        pic[y:y + int(rng.integers(1, 3)), x:x + int(rng.integers(1, 9))] = (10, 30, 60, 200)[int(rng.integers(0, 4))] * sc
    pic[h // 2:h // 2 + h // 8, :] = (np.arange(w) * 255 // w * sc)[None, :]                                                      # a gradient
    pic[h - h // 6:, :] = np.clip(rng.normal(128, 30, (h // 6, w)), 0, 255).astype(np.int64) * sc + rng.integers(0, sc, (h // 6, w))   # camera-like
    return pic.astype(np.uint8 if bd == 8 else np.uint16)


class TimedRef(P.RefBackend):
    """the reference's dispatched functions, with the time spent inside them"""

    def __init__(self, lib):
        super().__init__(lib)
        kind = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int)
        self.km = kind(C.c_void_p.in_dll(lib, "svt_av1_k_means_dim1").value)
        self.ci = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int)(C.c_void_p.in_dll(lib, "svt_av1_calc_indices_dim1").value)
        self.seconds = 0.0

    def count_colors(self, block, bd):
        t0 = time.perf_counter(); r = super().count_colors(block, bd); self.seconds += time.perf_counter() - t0
        return r

    def calc_indices(self, data, centroids):
        cent, idx = np.asarray(centroids, np.int32), np.zeros(len(data), np.uint8)
        t0 = time.perf_counter()
        self.ci(data.ctypes.data, cent.ctypes.data, idx.ctypes.data, len(data), len(cent))
        self.seconds += time.perf_counter() - t0
        return idx, None

    def k_means(self, data, centroids, k):
        cent, idx = np.asarray(centroids[:k], np.int32).copy(), np.zeros(len(data), np.uint8)
        t0 = time.perf_counter()
        self.km(data.ctypes.data, cent.ctypes.data, idx.ctypes.data, len(data), k, 50)
        self.seconds += time.perf_counter() - t0
        return [int(v) for v in cent]


simd = os.path.join(ROOT, "oracle", "_ref", "libsvtav1_ref_simd.so")
ref = None
if os.path.exists(simd):
    ref = C.CDLL(simd)
    ref.get_cpu_flags_to_use.restype = C.c_uint64
    flags = C.c_uint64(ref.get_cpu_flags_to_use())
    ref.setup_common_rtcd_internal(flags); ref.setup_rtcd_internal(flags)

W, H = 1920, 1080
pic = screen_picture(W, H, 8, 1)
d_pic = hip.to_device(pic)
for size in (8, 16, 32, 64):
    jobs = [dict(x=x, y=y, bw=size, bh=size, cols=size, rows=size, cache=[], step=1) for y in range(0, H - size + 1, size) for x in range(0, W - size + 1, size)]
    tab, nbytes = P.c_jobs(pkg, jobs)
    n = len(jobs)
    with hip.scope() as s:
        d_jobs, d_res, d_cands, d_maps = s.structs(tab), s.empty(n * C.sizeof(pkg.PaletteResult)), s.empty(n * 14 * C.sizeof(pkg.PaletteCand)), s.empty(nbytes)
        t = per_call(lambda: hip.check(L.svt_hip_palette_search_batch_dev(hip.h, 1, 8, d_pic, W, d_jobs, n, d_res, d_cands, d_maps), "palette_search_batch"))
        res = s.download(d_res, (n, 2), np.int32)
    searched = int(((res[:, 0] > 1) & (res[:, 0] <= 64)).sum())
    line = (f"palette search {W}x{H} 8-bit, {size:2d}x{size:<2d}: {t * 1e3:8.1f} us per launch  {n:6d} jobs, {searched:6d} with 1 < colors <= 64, "
            f"{int(res[:, 1].sum()):7d} candidates kept, {t * 1e6 / n:6.1f} ns per job")
    if ref is not None:
        be, step = TimedRef(ref), max(1, n // args.host_blocks)
        sample = jobs[::step]
        kept = sum(len(P.search(be, pic, j, 8)["cands"]) for j in sample)
        host = be.seconds * n / len(sample)
        line += f"  | host, one thread, reference dispatch: {host * 1e3:9.1f} ms ({len(sample)} blocks timed, {kept} candidates; {host / (t * 1e-3):7.0f} x)"
    print(line, flush=True)
hip.free(d_pic)

W, H = 3840, 2160
for bd in (8, 10):
    pic = screen_picture(W, H, bd, 2)
    d_pic, d_out = hip.to_device(pic), hip.empty(16)
    t = per_call(lambda: hip.check(L.svt_hip_screen_content_detect_dev(hip.h, pic.itemsize, bd, d_pic, W, W, H, d_out), "screen_content_detect"))
    out = hip.to_host(d_out, (4,), np.int32).tolist()
    line = (f"screen-content detection {W}x{H} {bd:2d}-bit: {t * 1e3:8.1f} us per call  {(W // 16) * (H // 16)} blocks, {W * H * pic.itemsize / 1e6:.1f} MB read "
            f"-> {W * H * pic.itemsize / t / 1e6:7.1f} GB/s  counts {out[0]}, {out[1]}  detected {out[2]}, {out[3]}")
    if ref is not None:
        t0 = time.perf_counter(); want = P.ref_screen_content(ref, pic, bd); host = time.perf_counter() - t0
        line += f"  | host, one thread, the reference's C functions block by block from Python, the loop included: {host * 1e3:8.1f} ms, outputs {'equal' if want == out else 'DIFFER ' + str(want)}"
    print(line, flush=True)
    hip.free(d_pic, d_out)
hip.close()
