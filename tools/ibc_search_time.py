"""Times the intra-block-copy full-pel search, svt_hip_ibc_full_search_batch_dev (HIP events around back-to-back calls on resident data, windows of at least
--window ms), next to its serial host form on one thread, and checks that the two give the same results.
  - Pictures: the synthetic screen-like 8-bit picture of tools/ibc_hash_time.py and a noise picture, at 1920x1080 and 3840x2160; the hash table is the one the
    device builds.
  - Job lists, one launch each: up to --jobs blocks spread evenly over the picture's grid of 4x4, 4x16 and 16x4 blocks with exhaustive_allowed (the reference's
    is_exhaustive_allowed) and of 16x16 and 64x64 blocks without, each block twice: with the "above" and with the "left" limits as intra_bc_search builds them
    (Encoder/Codec/EbModeDecision.c:4461-4476) for one tile and 64x64 superblocks.  Blocks whose limits are empty (the first superblock row or column) stay in the
    list as the caller's `continue`.  Mesh patterns {256, 1} x 2, what an intra picture gets (Encoder/Codec/EbModeDecisionConfigurationProcess.c:931-937).
  - The output states the work: jobs searched, jobs that ran the mesh, candidates the mesh scanned (from the walk's windows) and the sample differences that is.
  - The host form runs on --host-jobs of the jobs, drawn at random (seeded), and its time is scaled by the number of jobs: the only CPU figure available without the reference's structures.
    python tools/ibc_search_time.py [--window 100] [--jobs 2048] [--host-jobs 96] [--sizes 1920x1080,3840x2160]"""
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
import ibc_search_common as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=100.0, help="least length of a timed window, ms")
ap.add_argument("--jobs", type=int, default=2048, help="blocks per shape (each is searched with both limits)")
ap.add_argument("--host-jobs", type=int, default=96, help="of the jobs, those the host form is timed on")
ap.add_argument("--sizes", default="1920x1080,3840x2160")
args = ap.parse_args()
pkg = load_package()
hip = pkg.Context(0)
L = hip.L
PATTERNS = S.PATTERNS["full"]
pat = pkg.ibc_mesh_patterns(PATTERNS)


def screen_picture(w, h, seed):
    """as tools/ibc_hash_time.py"""
    rng = np.random.default_rng(seed)
    pic = np.full((h, w), 240, np.int64)
    for _ in range(w * h // 20000):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        pic[y:y + int(rng.integers(20, 300)), x:x + int(rng.integers(40, 500))] = int(rng.integers(0, 256))
    for _ in range(w * h // 150):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        pic[y:y + int(rng.integers(1, 3)), x:x + int(rng.integers(1, 9))] = (10, 30, 60, 200)[int(rng.integers(0, 4))]
    pic[h // 2:h // 2 + h // 8, :] = (np.arange(w) * 255 // w)[None, :]
    pic[h - h // 6:, :] = np.clip(rng.normal(128, 30, (h // 6, w)), 0, 255).astype(np.int64)
    return pic.astype(np.uint8)


def search_range(lim, ref=(0, 0)):
    """svt_av1_set_mv_search_range (Encoder/Codec/av1me.c:249-270), which the caller applies to its limits: at most MAX_FULL_PEL_VAL = 1023 whole samples from
    the reference vector"""
    lo_c, hi_c = (ref[1] >> 3) - 1023 + (1 if ref[1] & 7 else 0), (ref[1] >> 3) + 1023
    lo_r, hi_r = (ref[0] >> 3) - 1023 + (1 if ref[0] & 7 else 0), (ref[0] >> 3) + 1023
    return (max(lim[0], lo_c), min(lim[1], hi_c), max(lim[2], lo_r), min(lim[3], hi_r))


def scanned(jobs, res):
    """candidates of the one {256, 1} scan of every job that ran the mesh, centre included: the window of csrc/ibc_search.h's mesh_geom around the diamond's vector"""
    total = 0
    for j, r in zip(jobs, res):
        if not r["mesh_ran"] or not r["mesh_passes"]: continue
        fr, fc = min(max(r["dia_row"], j["row_min"]), j["row_max"]), min(max(r["dia_col"], j["col_min"]), j["col_max"])
        rng = min(max(256, 5 * max(abs(r["dia_row"]), abs(r["dia_col"])) // 4), 256)
        rows = min(rng, j["row_max"] - fr) - max(-rng, j["row_min"] - fr) + 1
        cols = min(rng, j["col_max"] - fc) - max(-rng, j["col_min"] - fc) + 1
        total += 1 + rows * (cols - (cols % 4 != 0))
    return total


jc, cc = I.cost_tables()
d_jc, d_cc = hip.to_device(jc), hip.to_device(cc)
for size in args.sizes.split(","):
    W, H = (int(v) for v in size.split("x"))
    for kind, pic in (("screen", screen_picture(W, H, 1)), ("noise", I.noise(W, H))):
        cap, nbytes = int(L.svt_hip_ibc_hash_max_entries(W, H)), L.svt_hip_ibc_hash_scratch_bytes(W, H)
        d_pic, d_start, d_ent, d_info, d_scr = hip.to_device(pic), hip.empty((I.N_BUCKETS + 1) * 4), hip.empty(cap * 8), hip.empty(8), hip.empty(nbytes)
        hip.check(L.svt_hip_ibc_hash_table_dev(hip.h, 1, 8, d_pic, W, W, H, d_start, d_ent, cap, d_info, d_scr, nbytes), "ibc_hash_table")
        hip.sync()
        n_entries = int(hip.to_host(d_info, (2,), np.int32)[0])
        table = (hip.to_host(d_start, (I.N_BUCKETS + 1,), np.int32), hip.to_host(d_ent, (n_entries,), I.ENTRY_DTYPE))
        hip.free(d_scr)
        print(f"{W}x{H} {kind}: {n_entries / 1e6:.2f} M table entries", flush=True)
        for bw, bh, ex in ((4, 4, 1), (4, 16, 1), (16, 4, 1), (16, 16, 0), (64, 64, 0)):
            grid = [(x, y) for y in range(0, H - bh + 1, bh) for x in range(0, W - bw + 1, bw)]
            grid = grid[::max(1, len(grid) // args.jobs)][:args.jobs]
            jobs = [S.job(x, y, bw, bh, search_range(S.caller_limits(x, y, bw, bh, W, H, d)), W, H, ex=ex, shift=1, use_hash=int(bw == bh)) for x, y in grid
                    for d in ("above", "left")]
            tab = S.c_jobs(pkg, jobs)
            n, nb = len(jobs), L.svt_hip_ibc_full_search_scratch_bytes(len(jobs))
            with hip.scope() as s:
                d_jobs, d_res, d_s = s.structs(tab), s.empty(n * C.sizeof(pkg.IbcFullSearchResult)), s.empty(max(nb, 256))
                call = lambda: hip.check(L.svt_hip_ibc_full_search_batch_dev(hip.h, 1, 8, d_pic, W, W, H, d_start, d_ent, d_jc, d_cc, pat.ctypes.data_as(C.c_void_p), d_jobs, n,
                                                                             d_res, d_s, nb), "ibc_full_search")
                t = hip.timed(call, args.window)[0]
                res = S.c_results(s.structs_back(d_res, pkg.IbcFullSearchResult * n), n)
            pick = sorted(np.random.default_rng(bw * 1000 + bh).choice(n, min(n, args.host_jobs), replace=False).tolist())   # no stride: the list alternates limits
            few = [jobs[i] for i in pick]
            t0 = time.perf_counter(); h_res = S.c_results(pkg.ibc_full_search_host(pic, table, jc, cc, PATTERNS, S.c_jobs(pkg, few)), len(few)); host = time.perf_counter() - t0
            same = h_res == [res[i] for i in pick]
            cand, cand_few = scanned(jobs, res), scanned(few, [res[i] for i in pick])
            searched, mesh = sum(r["status"] == 0 for r in res), sum(r["mesh_ran"] for r in res)
            src = [sum(r["status"] == 0 and r["source"] == k for r in res) for k in range(3)]
            scaled = host * n / len(few)
            print(f"  {bw:2d}x{bh:<2d}: {t:9.3f} ms per call  {n:5d} jobs, {searched:5d} searched, {mesh:5d} ran the mesh, {cand / 1e6:9.2f} M candidates = "
                  f"{cand * bw * bh / 1e9:8.2f} G sample differences ({cand * bw * bh / (t * 1e-3) / 1e12:6.3f} T/s if the mesh were all of the call), taken from "
                  f"diamond/mesh/hash {src}  | host form, one thread ({len(few)} jobs with {cand_few / 1e6:.2f} M candidates timed, scaled by jobs): {scaled * 1e3:10.1f} ms "
                  f"({scaled / (t * 1e-3):7.0f} x), results {'equal' if same else 'DIFFER'}", flush=True)
        hip.free(d_pic, d_start, d_ent, d_info)
hip.free(d_jc, d_cc)
hip.close()
