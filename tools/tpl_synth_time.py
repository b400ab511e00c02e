"""Times svt_hip_tpl_window_dev at 3840x2160 with 3, 17 and 33 pictures (HIP events around back-to-back calls on resident records and grids, windows of at
least --window-ms), beside launches x 1.45 us: the call is a chain of dependent launches on one stream (one memset and one scatter per picture, then one
memset and two kernels for r0 / beta), and the microarchitecture guide's figure for a dependent kernel boundary is what such a chain costs at the least.
Records: the seeded generator of tests/tpl_synth_common.py; picture k references k - 1 and, from the third on, k - 2 and picture 0.
    python tools/tpl_synth_time.py [--window-ms 150] [--size 3840x2160] [--pictures 3,17,33]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402
import tpl_synth_common as S  # noqa: E402

BOUNDARY_US = 1.45   # a dependent kernel boundary on one stream (the microarchitecture guide's figure)

ap = argparse.ArgumentParser()
ap.add_argument("--window-ms", type=float, default=150.0)
ap.add_argument("--size", default="3840x2160")
ap.add_argument("--pictures", default="3,17,33")
args = ap.parse_args()
w, h = (int(v) for v in args.size.split("x"))
counts = [int(v) for v in args.pictures.split(",")]
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
P = pkg.tpl_synth_params(w, h, 1234, r0_in=0.75)
dep_bytes = L.svt_hip_tpl_dep_bytes(w, h, P.cell_log2)
rng = np.random.default_rng(1)
n_max = max(counts)
pocs = [16 * k for k in range(n_max)]
d_stats = [hip.to_device(S.random_stats(rng, w, h, 3)) for _ in range(n_max)]
d_dep = [hip.empty(dep_bytes) for _ in range(n_max)]
d_out = hip.empty(L.svt_hip_tpl_r0beta_out_bytes(w, h, P.sb_size))
d_scratch = hip.empty(L.svt_hip_tpl_r0beta_scratch_bytes())
print(f"tpl_window {w}x{h}, {1 << P.cell_log2}x{1 << P.cell_log2} cells, {dep_bytes // 16} source blocks per picture, grid {dep_bytes / 1e6:.2f} MB")
for n in counts:
    slots = [[pocs[k - 1] if k >= 1 else 999, pocs[k - 2] if k >= 2 else 999, pocs[0] if k >= 2 else 999] for k in range(n)]
    F = pkg.tpl_window_frames([(d_stats[k], d_dep[k], 1, pkg.tpl_ref_window(pocs[:n], slots[k])) for k in range(n)])

    def once():
        hip.check(L.svt_hip_tpl_window_dev(hip.h, C.byref(P), F, n, d_out, d_scratch), "tpl_window")

    t, win, reps = hip.timed(once, args.window_ms, growth=1.3)   # this tool has always grown its windows by 1.3, not 1.2
    launches = 2 * n + 3
    print(f"  {n:2d} pictures: {t:.4f} ms per window  (window {win:.0f} ms, {reps} calls); {launches} launches ({n} memsets + {n} scatters + 1 memset + 2 kernels) "
          f"x {BOUNDARY_US} us = {launches * BOUNDARY_US / 1e3:.4f} ms; {1e3 * t / launches:.2f} us per launch")
hip.free(*d_stats, *d_dep, d_out, d_scratch)
hip.close()
