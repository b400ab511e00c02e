"""Records tests/golden/cfl_filter_intra.npz through the reference (oracle/_ref/libsvtav1_ref.so): a few CfL jobs and filter-intra jobs per bit depth, inputs and
expected outputs only, so that tests/test_cfl_gpu.py and tests/test_filter_intra_gpu.py have a case that needs no reference library.  Run from the repository
root after build():
    python tests/golden/make_cfl_golden.py
tests/test_cfl_ref_cpu.py checks that the stored file is what record() gives."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cfl_common as cc  # noqa: E402
import intra_common as ic  # noqa: E402

CFL_SHAPES = {8: [0, 1, 8, 13, 15, 3], 10: [0, 6, 7, 2, 16]}   # 4x4 8x8 16x8 4x16 8x32 32x32 | 4x4 8x4 8x16 16x16 32x8


def cfl_jobs(dtype, bd):
    rng = np.random.default_rng(4200 + bd)
    return [cc.cfl_job(rng, dtype, bd, t, (int(rng.integers(-16, 17)), int(rng.integers(-16, 17))), "extreme" if i % 3 == 2 else "random",
                       3 if i % 4 else 1 + (i // 4) % 2, i & 1, (i * 7) % 4) for i, t in enumerate(CFL_SHAPES[bd])]


def fi_jobs(bd):
    return [(t, (i + bd) % 5) for i, t in enumerate(cc.SHAPES)]


def record(L):
    out = {}
    for dtype, bd in cc.BDS:
        jobs = cfl_jobs(dtype, bd)
        refs = cc.ref_cfl_jobs(L, jobs, bd)
        k = f"cfl{bd}_"
        out[k + "spec"] = np.array([[j["tx_size"], j["alpha"][0], j["alpha"][1], j["plane_mask"], j["dc_from_edges"], j["dc_have"]] for j in jobs], np.int32)
        out[k + "luma"] = np.concatenate([j["luma"].ravel() for j in jobs])
        out[k + "pred"] = np.concatenate([j["pred"].ravel() for j in jobs])
        out[k + "recs"] = np.stack([j["recs"] for j in jobs])
        out[k + "out"] = np.concatenate([np.stack(r[1]).ravel() for r in refs])
        out[k + "ac"] = np.concatenate([r[0][:cc.cfl_dims(j)[1], :cc.cfl_dims(j)[0]].ravel() for j, r in zip(jobs, refs)])
        fj = fi_jobs(bd)
        recs = cc.fi_records(np.random.default_rng(4300 + bd), len(fj), dtype, bd, "extreme")
        recs[:, 0, cc.EDGE_ORG + 32:] = 0; recs[:, 0, :cc.EDGE_ORG - 1] = 0; recs[:, 1, cc.EDGE_ORG + 32:] = 0; recs[:, 1, :cc.EDGE_ORG] = 0   # never read: stored as zeros
        k = f"fi{bd}_"
        out[k + "spec"] = np.array(fj, np.int32)
        out[k + "recs"] = recs
        out[k + "out"] = np.concatenate([cc.ref_filter_intra(L, r, bd, t, m).ravel() for (t, m), r in zip(fj, recs)])
    return out


def load_cfl(g, dtype, bd):
    """-> (jobs, refs) in the form tests/cfl_common.py works with"""
    k = f"cfl{bd}_"
    jobs, refs, o = [], [], dict(luma=0, pred=0, out=0, ac=0)
    def take(name, shape):
        n = int(np.prod(shape)); a = g[k + name][o[name]:o[name] + n].reshape(shape); o[name] += n
        return a
    for spec, recs in zip(g[k + "spec"], g[k + "recs"]):
        j = dict(tx_size=int(spec[0]), alpha=(int(spec[1]), int(spec[2])), plane_mask=int(spec[3]), dc_from_edges=int(spec[4]), dc_have=int(spec[5]), kind="golden", recs=recs)
        w, h = cc.cfl_dims(j)
        j["luma"], j["pred"] = take("luma", (2 * h, 2 * w)), take("pred", (2, h, w))
        ac = np.zeros((cc.AC_LINE, cc.AC_LINE), np.int16); ac[:h, :w] = take("ac", (h, w))
        jobs.append(j); refs.append((ac, list(take("out", (2, h, w)))))
    assert g[k + "luma"].dtype == dtype
    return jobs, refs


def load_fi(g, dtype, bd):
    """-> (jobs, records, expected blocks)"""
    k = f"fi{bd}_"
    jobs, blocks, o = [tuple(int(v) for v in s) for s in g[k + "spec"]], [], 0
    for j in jobs:
        w, h = cc.fi_dims(j)
        blocks.append(g[k + "out"][o:o + w * h].reshape(h, w)); o += w * h
    assert g[k + "recs"].dtype == dtype
    return jobs, g[k + "recs"], blocks


def main():
    L = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "libsvtav1_ref.so"))
    L.setup_common_rtcd_internal(0)
    L.setup_rtcd_internal(0)
    out = record(L)
    path = os.path.join(HERE, "cfl_filter_intra.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
