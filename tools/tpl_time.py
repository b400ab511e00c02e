"""Times svt_hip_tpl_dispenser_picture_dev at 3840x2160 (HIP events around back-to-back calls on resident planes, windows of at least --window-ms):
(a) the mostly-inter picture of the test generator, (b) the same picture with no reference (every macroblock intra).  For each the whole call, and by
svt_hip_tpl_set_phases phase A alone, phase B alone (on the decisions the whole call left in the scratch buffer) and the padding alone.
    python tools/tpl_time.py [--window-ms 150] [--size 3840x2160]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402
import intra_common as ic  # noqa: E402
import tpl_common as T  # noqa: E402

BOUNDARY_US = 1.45   # a dependent kernel boundary on one stream (the microarchitecture guide's figure), for comparison with phase B

ap = argparse.ArgumentParser()
ap.add_argument("--window-ms", type=float, default=150.0)
ap.add_argument("--size", default="3840x2160")
ap.add_argument("--golden-qp", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "tpl_dispenser_200x136.npz"),
                help="file whose 'qp' rows (qindex 140) are used: the tool needs no reference library")
args = ap.parse_args()
w, h = (int(v) for v in args.size.split("x"))
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
qp = np.load(args.golden_qp)["qp"]
case = T.make_case(w, h, T.case_seed(w, h))
mbw, mbh = (w + 15) // 16, (h + 15) // 16
steps = mbw + 2 * mbh - 2
held = []


def up(a):
    d = hip.to_device(a); held.append(d)
    return d


S = case["cur"].shape[1]
org = lambda d: C.c_void_p(d.value + T.PAD * S + T.PAD)
d_cur = up(case["cur"])
d_mode, d_cost = hip.empty(mbw * mbh), hip.empty(mbw * mbh * 4); held += [d_mode, d_cost]
hip.check(L.svt_hip_intra_ois_picture_dev(hip.h, org(d_cur), S, w, h, 12, d_mode, d_cost), "intra ois")
refs = (pkg.TplRef * 7)()
for r in range(3):
    sp, rp = case["refs"][r]
    ds = up(sp); dr = ds if rp is sp else up(rp)
    refs[r].d_src, refs[r].d_rec, refs[r].src_stride, refs[r].rec_stride = org(ds).value, org(dr).value, S, S
none = (pkg.TplRef * 7)()
d_mv, d_mask = up(case["mv"]), up(case["mask"])
d_rec = up(np.zeros_like(case["cur"]))
d_stats = hip.empty(mbw * mbh * C.sizeof(pkg.TplMbStats)); held.append(d_stats)
d_scratch = hip.empty(L.svt_hip_tpl_dispenser_scratch_bytes(w, h)); held.append(d_scratch)
P = pkg.TplParams()
P.w, P.h, P.pad, P.q = w, h, T.PAD, T.device_qparams(pkg, qp)
P.use_ois, P.add_residual, P.rate, P.best_ref_only = 1, 1, 1, 0

for name, table in (("generator picture", refs), ("all-intra picture", none)):
    once = lambda: hip.check(L.svt_hip_tpl_dispenser_picture_dev(hip.h, C.byref(P), org(d_cur), S, table, d_mv, d_mask, d_mode, d_cost, org(d_rec), S, d_stats, d_scratch), "tpl")
    hip.check(L.svt_hip_tpl_set_phases(hip.h, 7), "phases")
    once()
    hip.sync()
    st = hip.to_host(d_stats, (mbh, mbw), np.dtype(pkg.TplMbStats))
    print(f"tpl_dispenser {w}x{h} qindex 140, {name}: {mbw * mbh} macroblocks, inter share {float((st['is_inter'] != 0).mean()):.3f}, "
          f"launches per call: 1 (phase A) + {steps} (phase B) + 1 (padding)")
    for label, mask in (("whole call", 7), ("phase A", 1), ("phase B", 2), ("padding", 4)):
        hip.check(L.svt_hip_tpl_set_phases(hip.h, mask), "phases")
        t, win, reps = hip.timed(once, args.window_ms, growth=1.3)   # this tool has always grown its windows by 1.3, not 1.2
        extra = f"  = {1e3 * t / steps:.2f} us per step; {steps} boundaries x {BOUNDARY_US} us = {steps * BOUNDARY_US / 1e3:.3f} ms" if mask == 2 else ""
        print(f"  {label:10s}: {t:.4f} ms per picture  (window {win:.0f} ms, {reps} calls){extra}")
hip.check(L.svt_hip_tpl_set_phases(hip.h, 7), "phases")
hip.free(*held)
hip.close()
