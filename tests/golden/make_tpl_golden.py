"""Writes tests/golden/tpl_dispenser_200x136.npz: the 200x136 generator case of tests/tpl_common.py at qindex 140 and its all-intra variant -- inputs (picture
areas only: the borders are replication and are re-created on load), MV words, masks, the open-loop intra tables, the quantiser table rows, and the statistics
and reconstruction the reference's functions give (tpl_common.ref_dispenser).  Needs oracle/_ref/libsvtav1_ref.so.

    python tests/golden/make_tpl_golden.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import intra_common as ic   # noqa: E402
import tpl_common as T      # noqa: E402

W, H, QINDEX = 200, 136, 140


def compose(L):
    case = T.make_case(W, H, T.case_seed(W, H))
    om, oc = ic.ref_ois(L, T.cur_plane(case), W, H)
    qp = T.qparams(L, QINDEX)
    stats, rec = T.ref_dispenser(L, case, om, oc, qp)
    stats_i, rec_i = T.ref_dispenser(L, T.all_intra(case), om, oc, qp)
    area = lambda p: np.ascontiguousarray(p[T.PAD:T.PAD + H, T.PAD:T.PAD + W])
    out = dict(cur=area(case["cur"]), mv=case["mv"][:3], mask=case["mask"], ois_mode=om.astype(np.uint8), ois_cost=oc.astype(np.int32), qp=qp,
               stats=stats, recon=area(rec), stats_intra=stats_i, recon_intra=area(rec_i))
    for r in range(3):
        out[f"src{r}"] = area(case["refs"][r][0])
        if case["refs"][r][1] is not case["refs"][r][0]: out[f"rec{r}"] = area(case["refs"][r][1])
    return out


if __name__ == "__main__":
    L = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "libsvtav1_ref.so"))
    L.setup_common_rtcd_internal(0); L.setup_rtcd_internal(0)
    path = os.path.join(HERE, "tpl_dispenser_200x136.npz")
    np.savez_compressed(path, **compose(L))
    print(path, os.path.getsize(path), "bytes")
