"""Times the in-loop filter search / apply entry points on a 3840x2160 4:2:0 picture at 8 and 10 bit (HIP events):
deblock, CDEF search + apply, SGR search + apply and the 16x16 sub-pel prediction — the stages whose 16-bit paths differ from the 8-bit bench step.
    python tools/hbd_time.py [--bd 10]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

os.environ.setdefault("SVT_HIP_SGR_WALK_CLOCKS", "1")   # the walks' phase clocks are a diagnostic that is off by default

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402
import dlf_common as dc  # noqa: E402

pkg = load_package()
ap = argparse.ArgumentParser()
ap.add_argument("--bd", type=int, default=10)
args = ap.parse_args()
hip = pkg.Context(0)
L = hip.L
W, H, bd = 3840, 2160, args.bd
dt = np.uint8 if bd == 8 else np.uint16
pb = 1 if bd == 8 else 2
rng = np.random.default_rng(4)
src, rec = [], []
for p in range(3):
    w, h = (W, H) if p == 0 else (W // 2, H // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    s = (100 + 60 * np.sin(xx / 11.0 + p) * np.cos(yy / 9.0) + 30 * (((xx + 2 * yy) // 14) % 2)) * (1 << (bd - 8))
    src.append(np.clip(s, 0, (1 << bd) - 1).astype(dt))
    # reconstruction = coarse quantisation of the source (coding-like artefacts, strength per 64x64 region) + mild noise in some regions
    region = (xx // 64 + 2 * (yy // 64)) % 4
    q = np.array([2, 6, 12, 24])[region] * (1 << (bd - 8))
    r = (np.clip(s, 0, (1 << bd) - 1) // q) * q + q // 2 + rng.normal(0, 3 * (1 << (bd - 8)), (h, w)) * (region == 3)
    rec.append(np.clip(r, 0, (1 << bd) - 1).astype(dt))
skip8 = (rng.random((H // 8, W // 8)) < 0.25).astype(np.uint8)
P3, I3 = C.c_void_p * 3, C.c_int * 3
d_src = [hip.to_device(p) for p in src]; d_rec = [hip.to_device(p) for p in rec]; d_out = [hip.to_device(p) for p in rec]
strides = I3(*[p.shape[1] for p in rec])
nfb = ((H + 63) // 64) * ((W + 63) // 64)
d_skip = hip.to_device(skip8)
d_mse = hip.to_device(np.zeros((nfb, 2, 64), np.uint64))
d_dir = hip.to_device(np.zeros((H // 8, W // 8), np.uint8)); d_var = hip.to_device(np.zeros((H // 8, W // 8), np.int32))
ys = rng.integers(0, 64, nfb).astype(np.uint8); uvs = rng.integers(0, 64, nfb).astype(np.uint8)
d_ys, d_uvs = hip.to_device(ys), hip.to_device(uvs)
EXT = 3
ext = [np.ascontiguousarray(np.pad(p, EXT, mode="edge")) for p in rec]
d_ext = [hip.to_device(e) for e in ext]
US = (256, 128, 128)
units = [max((p.shape[1] + US[i] // 2) // US[i], 1) * max((p.shape[0] + US[i] // 2) // US[i], 1) for i, p in enumerate(rec)]
d_sums = [hip.to_device(np.zeros((n, 16, 5), np.int64)) for n in units]
d_ep = [hip.to_device(rng.integers(0, 16, n).astype(np.uint8)) for n in units]
d_xqd = [hip.to_device(np.stack([rng.integers(-96, 32, n), rng.integers(-32, 96, n)], 1).astype(np.int32)) for n in units]


def cdef_search():
    hip.check(L.svt_hip_cdef_search_frame_dev(hip.h, pb, P3(*[p.value for p in d_rec]), strides, P3(*[p.value for p in d_src]), strides, W, H, d_skip, 5, bd,
                                              d_mse, d_dir, d_var), "cdef search")


def cdef_apply():
    hip.check(L.svt_hip_cdef_apply_frame_dev(hip.h, pb, P3(*[p.value for p in d_rec]), P3(*[p.value for p in d_out]), strides, W, H, d_skip, d_ys, d_uvs, 5, bd,
                                             d_dir, d_var), "cdef apply")


def sgr_search():
    for p in range(3):
        st = ext[p].shape[1]
        hip.check(L.svt_hip_sgr_search_plane_dev(hip.h, pb, bd, d_ext[p].value + (EXT * st + EXT) * pb, st, d_src[p], rec[p].shape[1], rec[p].shape[1], rec[p].shape[0],
                                                 US[p], int(p > 0), 0xFFFF, d_sums[p]), "sgr search")


def sgr_apply():
    for p in range(3):
        st = ext[p].shape[1]
        hip.check(L.svt_hip_sgr_apply_plane_dev(hip.h, pb, bd, d_ext[p].value + (EXT * st + EXT) * pb, st, d_out[p], rec[p].shape[1], rec[p].shape[1], rec[p].shape[0],
                                                US[p], int(p > 0), d_rec[p], rec[p].shape[1], d_ep[p], d_xqd[p]), "sgr apply")


mi, cols, rows = dc.make_mode_info(W, H)
edges = [dc.product_host_edges(mi, cols, rows, p, rec[p].shape[1], rec[p].shape[0]) for p in range(3)]
d_ev = [hip.to_device(e[0]) for e in edges]; d_eh = [hip.to_device(e[1]) for e in edges]
d_dbl = [hip.to_device(p) for p in rec]


def deblock():   # in place on a scratch copy (content drifts over the repeats; the work per edge does not depend on it)
    hip.check(L.svt_hip_deblock_frame_dev(hip.h, P3(*[p.value for p in d_dbl]), pb, strides, bd, P3(*[p.value for p in d_ev]), P3(*[p.value for p in d_eh]),
                                          I3(*[e[0].shape[1] for e in edges]), I3(*[e[0].shape[0] for e in edges]), 0), "deblock")


PAD = 32
refp = np.ascontiguousarray(np.pad(rec[0], PAD, mode="edge"))
d_refp = hip.to_device(refp); d_pred = hip.to_device(np.zeros_like(rec[0]))
n16 = (W // 16) * (H // 16)
CB = (pkg.ConvBlk * n16)()
k = 0
for by in range(0, H, 16):
    for bx in range(0, W, 16):
        CB[k] = pkg.ConvBlk(bx + int(rng.integers(-8, 9)), by + int(rng.integers(-8, 9)), bx, by, 16, 16, 0, 0, int(rng.integers(0, 16)), int(rng.integers(0, 16)), 0, 0)
        k += 1
d_cb = hip.to_device(np.frombuffer(bytes(CB), np.uint8))


def subpel():
    hip.check(L.svt_hip_subpel_predict_batch_dev(hip.h, pb, bd, d_refp.value + (PAD * refp.shape[1] + PAD) * pb, refp.shape[1], d_pred, W, d_cb, n16), "subpel")


def sgr_units_search():   # the complete per-unit search, host-output form, all three planes, 16 sets
    global rounds_used
    P = (pkg.SgrSearchPlane * 3)()
    for p in range(3):
        st = ext[p].shape[1]
        P[p] = pkg.SgrSearchPlane(d_ext[p].value + (EXT * st + EXT) * pb, st, d_src[p].value, rec[p].shape[1], rec[p].shape[1], rec[p].shape[0], US[p], int(p > 0), 0xFFFF,
                                  h_xqd[p].ctypes.data, h_err[p].ctypes.data, h_best[p].ctypes.data)
    r = C.c_int(0)
    hip.check(L.svt_hip_sgr_search_units_picture(hip.h, pb, bd, 3, P, C.byref(r)), "sgr units search")
    rounds_used = r.value


h_xqd = [np.zeros((n, 16, 2), np.int32) for n in units]; h_err = [np.zeros((n, 16), np.int64) for n in units]; h_best = [np.zeros(n, np.uint8) for n in units]
rounds_used = []
ms = C.c_float()
for name, fn in (("deblock", deblock), ("subpel_16x16", subpel), ("cdef_search", cdef_search), ("cdef_apply", cdef_apply), ("sgr_search", sgr_search), ("sgr_apply", sgr_apply)):
    for _ in range(3): fn()
    L.svt_hip_timer_start(hip.h)
    for _ in range(10): fn()
    L.svt_hip_timer_stop_ms(hip.h, C.byref(ms))
    print(f"{name:12s} {W}x{H} bd{bd}: {ms.value / 10:.3f} ms")
NCAND = 12   # of SVT_HIP_SGR_MAX_CAND = 24
d_cand = [hip.to_device(np.stack([rng.integers(-96, 32, (n, 16, NCAND)), rng.integers(-32, 96, (n, 16, NCAND))], -1).astype(np.int32)) for n in units]
d_cerr = [hip.to_device(np.zeros((n, 16, NCAND), np.int64)) for n in units]


def sgr_proj_error():
    for p in range(3):
        st = ext[p].shape[1]
        hip.check(L.svt_hip_sgr_proj_error_plane_dev(hip.h, pb, bd, d_ext[p].value + (EXT * st + EXT) * pb, st, d_src[p], rec[p].shape[1], rec[p].shape[1], rec[p].shape[0],
                                                     US[p], int(p > 0), 0xFFFF, NCAND, d_cand[p], d_cerr[p]), "sgr proj error")


for _ in range(3): sgr_proj_error()
L.svt_hip_timer_start(hip.h)
for _ in range(10): sgr_proj_error()
L.svt_hip_timer_stop_ms(hip.h, C.byref(ms))
print(f"sgr_proj_error {W}x{H} bd{bd}: {ms.value / 10:.3f} ms (16 sets x {NCAND} xqd candidates per unit, all three planes)")
import time
sgr_units_search()
hip.sync() if hasattr(hip, "sync") else None
t0 = time.perf_counter()
for _ in range(3): sgr_units_search()
dt = (time.perf_counter() - t0) / 3
print(f"sgr_units_search {W}x{H} bd{bd}: {dt * 1e3:.2f} ms wall per frame (host-output form incl. the result copies; best sets used {sorted(set(int(v) for v in h_best[0]))})")

# the device-output form: two launches per plane, nothing crosses PCIe -- HIP-event time of the whole search
scr = [L.svt_hip_sgr_search_units_scratch_bytes(rec[p].shape[1], rec[p].shape[0], US[p]) for p in range(3)]
d_scr = [hip.empty(n) for n in scr]
d_uxqd = [hip.empty(n * 16 * 8) for n in units]; d_uerr = [hip.empty(n * 16 * 8) for n in units]; d_ubest = [hip.empty(n) for n in units]; d_ubx = [hip.empty(n * 8) for n in units]


def sgr_units_dev(mask=0xFFFF):
    for p in range(3):
        st = ext[p].shape[1]
        hip.check(L.svt_hip_sgr_search_units_plane_dev(hip.h, pb, bd, d_ext[p].value + (EXT * st + EXT) * pb, st, d_src[p], rec[p].shape[1], rec[p].shape[1], rec[p].shape[0],
                                                       US[p], int(p > 0), mask, d_uxqd[p], d_uerr[p], d_ubest[p], d_ubx[p], d_scr[p], scr[p]), "sgr units dev")


for mask in (0xFFFF, 0x0038):
    for _ in range(3): sgr_units_dev(mask)
    L.svt_hip_timer_start(hip.h)
    for _ in range(10): sgr_units_dev(mask)
    L.svt_hip_timer_stop_ms(hip.h, C.byref(ms))
    print(f"sgr_units_dev  {W}x{H} bd{bd}: {ms.value / 10:.3f} ms device time per frame, ep mask {mask:#06x} (sums + difference planes + walk, all three planes, no host sync; scratch {sum(scr) / 1e6:.0f} MB)")
sgr_units_dev(0xFFFF)
for p in range(3):
    st3 = hip.to_host(d_scr[p], (32,), np.uint32)
    nw = units[p] * 16
    print(f"  plane {p} phase clocks per walk (x64 cycles): solve {st3[24] / nw:.0f}, replay {st3[25] / nw:.0f}, first-barrier wait (load) {st3[26] / nw:.0f}, evaluation {st3[27] / nw:.0f}, total {st3[28] / nw:.0f}; candidate loop of a data wave {st3[29] / max(int(st3[30]), 1) * 64:.0f} cycles per candidate")
    print(f"  plane {p}: {units[p]} units x 16 sets: {st3[0] / (units[p] * 16):.2f} evaluation passes, {st3[1] / (units[p] * 16):.2f} evaluated points per walk, unfinished {st3[2]}, "
          f"walks on the histogram {st3[3]}, passes histogram {list(st3[8:24])}")

# ---- how many parameter sets a provable lower bound could prune (VERDICT r05 #1c): e = q + r per sample with |q - continuous| <= 1/2, so the exact error of ANY tap pair is
# >= Q - sqrt(N Q) where Q is the quadratic's value there (Cauchy-Schwarz on the cross term); the final exact error of a set stands in for its Q_min (they differ by the
# rounding noise, ~0.1 %).  A set survives when its bound does not exceed the unit's best exact error.
for p in range(3):
    err = hip.to_host(d_uerr[p], (units[p], 16), np.int64).astype(np.float64)
    ph_, pw_ = rec[p].shape
    n_unit = float(pw_ * ph_) / units[p]   # average samples per unit
    lb = err - np.sqrt(n_unit * err)
    best = err.min(axis=1, keepdims=True)
    surv = (lb <= best).sum(axis=1)
    spread = (err.max(axis=1) - err.min(axis=1)) / err.min(axis=1)
    print(f"  plane {p}: sets surviving the bound Q - sqrt(N Q) <= best: mean {surv.mean():.2f} of 16 (min {surv.min()}, max {surv.max()}); mean squared error per sample "
          f"{(best / n_unit).mean():.1f}; (worst - best) / best over the 16 sets: mean {spread.mean():.3f}, max {spread.max():.3f}; slack sqrt(N Q) / Q: mean {(np.sqrt(n_unit * best) / best).mean():.3f}")

