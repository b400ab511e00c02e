"""Times OBMC in mode decision on the device: svt_hip_obmc_target_batch_dev (the weighted target) and svt_hip_obmc_search_batch_dev (the motion refinement), HIP
events around back-to-back calls on resident data, windows of at least --window ms after two warm-up calls, next to the serial host forms on one thread, and checks
that the two give the same results.
  - Picture: a seeded 8-bit 1920x1080 reference (low-pass noise and a little texture) with a border of 48 samples; the source is the reference displaced by
    (2, -3) samples with noise of a few levels, so the refinement walks a few steps and the sub-pel tree has something to find.
  - Job lists, one launch each: every 16x16 block, and every 32x32 block, each with one above and one left neighbour prediction (the source with other noise).
    The search starts at the zero vector with ref_mv = (1, -1) sample.  The job list is uploaded by every call: that copy is part of the call and of its time.
  - Probes: a probe is one evaluation of the block against the reference, svt_aom_obmc_sad in the refinement or svt_aom_upsampled_pred + svt_aom_obmc_variance in
    the sub-pel tree.  They are counted by the numpy restatement (tests/obmc_common.py) on --host-jobs of the jobs, drawn at random (seeded), and scaled by the
    number of jobs; the host form is timed on the same jobs and scaled the same way.
    python tools/obmc_search_time.py [--window 100] [--host-jobs 200] [--size 1920x1080]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402
import obmc_common as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=100.0, help="least length of a timed window, ms")
ap.add_argument("--host-jobs", type=int, default=200, help="of a list's jobs, those the host form is timed on and the restatement counts probes on")
ap.add_argument("--size", default="1920x1080")
args = ap.parse_args()
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
W, H = (int(v) for v in args.size.split("x"))
PAD = 48
rng = np.random.default_rng(1)
padded = S.pad_picture(S.smooth_picture(H, W, 21), PAD, PAD)
picture = padded[PAD:PAD + H, PAD:PAD + W]
source = np.clip(padded[PAD + 2:PAD + 2 + H, PAD - 3:PAD - 3 + W].astype(np.int16) + rng.integers(-3, 4, (H, W)), 0, 255).astype(np.uint8)
jc, cc = S.cost_tables()
mi_rows, mi_cols = H // 4, W // 4
d_src, d_jc, d_cc = hip.to_device(source), hip.to_device(jc), hip.to_device(cc)
d_pad = hip.to_device(padded)
d_ref = C.c_void_p(d_pad.value + PAD * padded.shape[1] + PAD)
print(f"{W}x{H}, border {PAD}", flush=True)
for b in (16, 32):
    bsize, n4, ov = S.BSIZE_OF[b, b], b // 4, b // 2
    cols, rows = W // b, H // b
    n = cols * rows
    # neighbour predictions: per job ov rows of b samples above, then b rows of ov samples left
    per = 2 * ov * b
    nbr = np.empty(n * per, np.uint8)
    tjobs, sjobs = [], []
    for k in range(n):
        x, y = (k % cols) * b, (k // cols) * b
        blk = source[y:y + b, x:x + b].astype(np.int16)
        nbr[k * per:k * per + ov * b] = np.clip(blk[:ov] + rng.integers(-9, 10, (ov, b)), 0, 255).reshape(-1)
        nbr[k * per + ov * b:(k + 1) * per] = np.clip(blk[:, :ov] + rng.integers(-9, 10, (b, ov)), 0, 255).reshape(-1)
        tjobs.append(dict(bsize=bsize, x=x, y=y, n_above=1, above_rel=[0] * 4, above_len=[n4, 0, 0, 0], n_left=1, left_rel=[0] * 4, left_len=[n4, 0, 0, 0], above_off=k * per,
                          above_stride=b, left_off=k * per + ov * b, left_stride=ov, wm_off=k * b * b))
        sjobs.append(dict(bsize=bsize, mi_row=y // 4, mi_col=x // 4, wm_off=k * b * b, mv_row=0, mv_col=0, ref_mv_row=8, ref_mv_col=-8, sad_per_bit=40, error_per_bit=60,
                          allow_hp=1))
    wm = n * b * b
    tj, sj = S.c_target_jobs(pkg, tjobs), S.c_search_jobs(pkg, sjobs)
    with hip.scope() as s:
        d_nbr, d_w, d_m, d_res = s.upload(nbr), s.empty(wm * 4), s.empty(wm * 4), s.empty(n * C.sizeof(pkg.ObmcSearchResult))
        target = lambda: hip.check(L.svt_hip_obmc_target_batch_dev(hip.h, d_src, W, W, H, d_nbr, nbr.size, C.cast(tj, C.c_void_p), n, d_w, d_m, wm), "obmc_target")
        search = lambda: hip.check(L.svt_hip_obmc_search_batch_dev(hip.h, d_ref, padded.shape[1], W, H, PAD, PAD, mi_rows, mi_cols, d_w, d_m, wm, d_jc, d_cc,
                                                                   C.cast(sj, C.c_void_p), n, d_res), "obmc_search")
        t_t, win_t, reps_t = hip.timed(target, args.window)
        t_s, win_s, reps_s = hip.timed(search, args.window)
        hip.sync()
        wsrc, mask = s.download(d_w, (wm,), np.int32), s.download(d_m, (wm,), np.int32)
        res = s.structs_back(d_res, pkg.ObmcSearchResult * n)
    pick = sorted(np.random.default_rng(n).choice(n, min(n, args.host_jobs), replace=False).tolist())
    t0 = time.perf_counter(); h_w, h_m = pkg.obmc_target_host(source, nbr, tj, wm); host_t = time.perf_counter() - t0
    few = S.c_search_jobs(pkg, [sjobs[i] for i in pick])
    t0 = time.perf_counter(); h_res = pkg.obmc_search_host(picture, PAD, PAD, mi_rows, mi_cols, wsrc, mask, jc, cc, few); host_s = time.perf_counter() - t0
    same_t = bool((h_w == wsrc).all() and (h_m == mask).all())
    same_s = all(bytes(h_res[k]) == bytes(res[i]) for k, i in enumerate(pick))
    sads = probes = 0
    for i in pick:
        info = {}
        j = sjobs[i]
        S.search(j, padded, PAD, PAD, mi_rows, mi_cols, wsrc[j["wm_off"]:j["wm_off"] + b * b].reshape(b, b), mask[j["wm_off"]:j["wm_off"] + b * b].reshape(b, b), jc, cc, info)
        sads += info["n_sads"]; probes += info["n_probes"]
    scale = n / len(pick)
    total = (sads + probes) * scale
    print(f"  {b}x{b}: {n} jobs", flush=True)
    print(f"    target: {t_t:8.3f} ms per call (window {win_t:.0f} ms, {reps_t} calls)  {wm / 1e6:.2f} M samples, {wm * 8 / (t_t * 1e-3) / 1e9:7.1f} GB/s written"
          f"  | host form, one thread: {host_t * 1e3:8.1f} ms ({host_t / (t_t * 1e-3):5.0f} x), arrays {'equal' if same_t else 'DIFFER'}", flush=True)
    print(f"    search: {t_s:8.3f} ms per call (window {win_s:.0f} ms, {reps_s} calls)  {sads * scale / n:.1f} full-pel + {probes * scale / n:.1f} sub-pel probes a job, "
          f"{total / (t_s * 1e-3) / 1e6:8.2f} M probes/s, {total * b * b / (t_s * 1e-3) / 1e9:7.2f} G probe-samples/s"
          f"  | host form, one thread ({len(pick)} jobs timed, scaled by jobs): {host_s * scale * 1e3:9.1f} ms ({host_s * scale / (t_s * 1e-3):6.0f} x), results "
          f"{'equal' if same_s else 'DIFFER'}", flush=True)
hip.free(d_src, d_jc, d_cc, d_pad)
hip.close()
