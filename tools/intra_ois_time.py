"""Times svt_hip_intra_ois_picture_dev on the 3840x2160 mixed frame of the intra tests (HIP events, resident plane) for mode_end 0, 8 and 12.
    python tools/intra_ois_time.py [--reps 1000]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402
import intra_common as ic  # noqa: E402

# Lane-operations of one (macroblock, mode) pair, counted from the shapes (not measured): a 16-point forward DCT of txfm_1d.h is 26 half-butterflies
# (2 multiplies, add, shift) and 48 additions; a pair runs 16 column and 16 row transforms, and per sample a prediction (about 6 operations averaged over
# the modes), the residual with its input shift (2), the rounding shift between the passes (2) and |c| with its add (2).
DCT16_OPS = 26 * 4 + 48
PAIR_OPS = 32 * DCT16_OPS + 256 * (6 + 2 + 2 + 2)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=1000)
args = ap.parse_args()
pkg = load_package()
hip = pkg.Context(0)
w, h = 3840, 2160
plane = ic.mixed_frame(w, h)
mbs = ((w + 15) // 16) * ((h + 15) // 16)
d_src, d_mode, d_cost = hip.to_device(plane), hip.empty(mbs), hip.empty(mbs * 4)
ms = C.c_float()
for mode_end in (0, 8, 12):
    def once():
        hip.check(hip.L.svt_hip_intra_ois_picture_dev(hip.h, d_src, plane.shape[1], w, h, mode_end, d_mode, d_cost), "intra ois")
    for _ in range(5): once()
    hip.check(hip.L.svt_hip_sync(hip.h), "sync")
    reps = args.reps * (8 if mode_end == 0 else 1)   # keep the timed window well over 0.1 s
    hip.L.svt_hip_timer_start(hip.h)
    for _ in range(reps): once()
    hip.check(hip.L.svt_hip_timer_stop_ms(hip.h, C.byref(ms)), "timer")
    t = ms.value / reps
    ops = mbs * (mode_end + 1) * PAIR_OPS
    print(f"intra_ois {w}x{h} mode_end {mode_end:2d}: {t:.4f} ms per picture  {mbs / t / 1e3:.2f} M macroblocks/s  "
          f"{ops / 1e9:.2f} G lane-ops counted -> {ops / t / 1e9:.1f} T lane-ops/s  (window {ms.value:.0f} ms, {reps} launches)")
hip.free(d_src, d_mode, d_cost)
hip.close()
