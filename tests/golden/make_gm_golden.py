"""Records tests/golden/gm_walks.npz through the reference (oracle/_ref/libsvtav1_ref.so): one small global-motion walk (planes, start, what
svt_av1_refine_integerized_param returns, the probes the restatement counts, the warp error of the start), so that tests/test_gm_gpu.py has a case that needs no
reference library.  Run from the repository root after build():
    python tests/golden/make_gm_golden.py
tests/test_gm_ref_cpu.py checks that the stored file is what record() gives."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gm_common as g  # noqa: E402

WALK = "rotzoom_near"


def record(L):
    wk = g.walk_by_name(WALK)
    src, ref = g.walk_planes(wk)
    (mat, wmtype, err), r = g.walk_reference(L, WALK)
    start = list(wk["start"]) + [0, 0]
    g.force_wmtype(start, wk["wmtype"])
    return dict(src=src, ref=ref, start=np.array(wk["start"], np.int32), spec=np.array([wk["wmtype"], wk["n"]], np.int32), wmmat=np.array(mat, np.int32),
                result=np.array([wmtype, err, r["probes"], r["invalid"]], np.int64),
                start_error=np.array([g.ref_warp_error(L, g.make_wm(start, wk["wmtype"]), ref, src)], np.int64))


def main():
    L = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "libsvtav1_ref.so"))
    L.setup_common_rtcd_internal(0)
    L.setup_rtcd_internal(0)
    path = os.path.join(HERE, "gm_walks.npz")
    np.savez_compressed(path, **record(L))
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
