"""Times the masked-compound and inter-intra searches, svt_hip_compound_search_batch_dev (HIP events around back-to-back calls on resident data, windows of at least
--window ms after two warm-up calls), next to the serial host form on one thread, and checks that the two give the same results.
  - Pictures: a seeded 8-bit picture (ramps, texture, noise) at 1920x1080 and 3840x2160.  Predictors: the picture's own blocks with seeded noise of a few levels,
    as two inter predictions (kinds 0, 1) or four intra predictions and an inter prediction (kind 2).
  - Job lists, one launch each: every 16x16 and every 32x32 block as kind 0 (inter-inter wedge) and as kind 2 (inter-intra), every 64x64 block as kind 1
    (diff-weighted), and all five lists in one launch.  The job list is uploaded by every call: that copy is part of the call and of its time.
  - The grids of the model are the recorded ones of tests/golden/comp_search.npz; the rate tables are the seeded stand-ins of tests/comp_search_common.py.
  - The output states the work: jobs, candidates, sample-candidates (samples of a block times candidates scored on it), and the time the candidate loops alone
    would take at the VALU issue rate: VALU_PER_SAMPLE_CANDIDATE lane-operations a sample-candidate, counted in the gfx950 code of the loops (wedge scan: 3.25 for
    the sign's dot product, 9 for the clamped squares; diff-weighted: 12.5 with the mask built on the fly; the four smooth blends: 10), over 256 CUs x 128 lanes a
    clock x --ghz.  Staging, reductions, the model and the launch are outside that bound.  An LDS bound is ten times lower (three 8-byte reads per four
    samples and candidate against 256 B a clock and CU) and is not the one that matters.
  - The host form runs on --host-jobs of the jobs, drawn at random (seeded), and its time is scaled by the number of jobs.
    python tools/comp_search_time.py [--window 100] [--host-jobs 400] [--sizes 1920x1080,3840x2160] [--ghz 2.4]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402
import comp_search_common as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=100.0, help="least length of a timed window, ms")
ap.add_argument("--host-jobs", type=int, default=400, help="of a list's jobs, those the host form is timed on")
ap.add_argument("--sizes", default="1920x1080,3840x2160")
ap.add_argument("--ghz", type=float, default=2.4)
args = ap.parse_args()
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
GRIDS = S.golden_grids()
hip.set_rd_curvfit_grids(GRIDS)
# lane-operations per sample and candidate in the candidate loops of comp_search.hip, from its gfx950 code
VALU_PER_SAMPLE_CANDIDATE = {"sign": 3.25, "sse": 9.0, "diffwtd": 12.5, "smooth": 10.0}


def picture(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    pic = 60 + (x * 90 // w) + (y * 70 // h) + 12 * ((x // 24 + y // 40) % 3) + rng.integers(-6, 7, (h, w))
    return np.clip(pic, 0, 255).astype(np.uint8)


def blocks_of(pic, b):
    """the picture's b x b blocks in raster order, each contiguous: (n, b * b)"""
    h, w = pic.shape[0] // b * b, pic.shape[1] // b * b
    return pic[:h, :w].reshape(h // b, b, w // b, b).transpose(0, 2, 1, 3).reshape(-1, b * b)


def make_list(pic, b, kind, pool, seed):
    """every b x b block as `kind`; appends its predictors to `pool` -> jobs"""
    rng = np.random.default_rng(seed)
    blk = blocks_of(pic, b).astype(np.int16)
    n, cols = blk.shape[0], pic.shape[1] // b
    npred = 5 if kind == S.KIND_INTERINTRA else 2
    preds = np.stack([np.clip(blk + rng.integers(-a, a + 1, blk.shape), 0, 255).astype(np.uint8) for a in (3, 5, 9, 14, 7)[:npred]], axis=1)   # (n, npred, b * b)
    base = sum(p.size for p in pool)
    pool.append(preds.reshape(-1))
    bsize = S.BSIZE[b, b]
    jobs = []
    for k in range(n):
        off = base + k * npred * b * b
        jobs.append(dict(kind=kind, bsize=bsize, x=(k % cols) * b, y=(k // cols) * b, pred0=off, pred1=off + (npred - 1) * b * b, quantizer=S.QUANT[8][2 + k % 4],
                         full_lambda=S.LAMBDAS[2 + k % 3], wedge_rate=bsize * 16 if kind == S.KIND_INTERINTRA else 0,
                         mode_rate=22 * 16 + 4 * S.SIZE_GROUP[bsize] if kind == S.KIND_INTERINTRA else 0))
    return jobs


def work(jobs):
    """-> (candidates, sample-candidates, seconds of the candidate loops at the VALU issue rate)"""
    cand = sc = ops = 0
    for j in jobs:
        n = S.BLOCK_W[j["bsize"]] * S.BLOCK_H[j["bsize"]]
        c = {S.KIND_WEDGE: 16, S.KIND_DIFFWTD: 2, S.KIND_INTERINTRA: 20}[j["kind"]]
        cand += c; sc += c * n
        V = VALU_PER_SAMPLE_CANDIDATE
        ops += n * {S.KIND_WEDGE: 16 * (V["sign"] + V["sse"]), S.KIND_DIFFWTD: 2 * V["diffwtd"], S.KIND_INTERINTRA: 4 * V["smooth"] + 16 * V["sse"]}[j["kind"]]
    return cand, sc, ops / (256 * 128 * args.ghz * 1e9)


rates = S.rate_tables()
d_rates = hip.to_device(rates)
for size in args.sizes.split(","):
    W, H = (int(v) for v in size.split("x"))
    pic = picture(W, H, 1)
    pool, lists = [], []
    for b in (16, 32):
        for kind, name in ((S.KIND_WEDGE, "wedge"), (S.KIND_INTERINTRA, "inter-intra")):
            lists.append(("%dx%d %s" % (b, b, name), make_list(pic, b, kind, pool, 10 * b + kind)))
    lists.append(("64x64 diff-weighted", make_list(pic, 64, S.KIND_DIFFWTD, pool, 641)))
    lists.append(("all five lists, one launch", [j for _, js in lists for j in js]))
    pool = np.concatenate(pool)
    d_pic, d_pool = hip.to_device(pic), hip.to_device(pool)
    print(f"{W}x{H}: predictor pool {pool.size / 1e6:.1f} M samples", flush=True)
    for name, jobs in lists:
        n = len(jobs)
        tab = S.c_jobs(pkg, jobs)
        with hip.scope() as s:
            d_res, d_cand = s.empty(n * C.sizeof(pkg.CompSearchResult)), s.empty(n * S.MAX_CANDS * C.sizeof(pkg.CompSearchCand))
            call = lambda: hip.check(L.svt_hip_compound_search_batch_dev(hip.h, 1, 8, d_pic, W, W, H, d_pool, pool.size, d_rates, rates.size, C.cast(tab, C.c_void_p), n,
                                                                         d_res, None), "compound_search")
            t, window, reps = hip.timed(call, args.window)
            hip.check(L.svt_hip_compound_search_batch_dev(hip.h, 1, 8, d_pic, W, W, H, d_pool, pool.size, d_rates, rates.size, C.cast(tab, C.c_void_p), n, d_res, d_cand),
                      "compound_search")
            hip.sync()
            res, cand = s.structs_back(d_res, pkg.CompSearchResult * n), s.structs_back(d_cand, pkg.CompSearchCand * (n * S.MAX_CANDS))
        pick = sorted(np.random.default_rng(n).choice(n, min(n, args.host_jobs), replace=False).tolist())
        few = S.c_jobs(pkg, [jobs[i] for i in pick])
        t0 = time.perf_counter(); h_res, h_cand = pkg.compound_search_host(GRIDS, pic, pool, rates, few); host = time.perf_counter() - t0
        same = all(bytes(h_res[k]) == bytes(res[i]) and bytes(h_cand)[k * 640:(k + 1) * 640] == bytes(cand)[i * 640:(i + 1) * 640] for k, i in enumerate(pick))
        ncand, sc, bound = work(jobs)
        scaled = host * n / len(pick)
        print(f"  {name:28s}: {t:8.3f} ms per call (window {window:.0f} ms, {reps} calls)  {n:6d} jobs, {ncand:7d} candidates, {sc / 1e6:8.1f} M sample-candidates "
              f"({sc / (t * 1e-3) / 1e9:7.1f} G/s); VALU bound of the candidate loops {bound * 1e3:7.4f} ms = {bound * 1e3 / t * 100:5.1f} % of the call  | host form, one "
              f"thread ({len(pick)} jobs timed, scaled by jobs): {scaled * 1e3:9.1f} ms ({scaled / (t * 1e-3):6.0f} x), results {'equal' if same else 'DIFFER'}", flush=True)
    hip.free(d_pic, d_pool)
hip.free(d_rates)
hip.close()
