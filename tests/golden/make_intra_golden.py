"""Records tests/golden/intra_ois_200x136.npz through the reference (oracle/_ref/libsvtav1_ref.so): the padded 208x144 plane of the 200x136 mixed frame and
the open-loop intra search's result on it (mode / cost at mode_end 12, and at 0 and 8).  Run from the repository root after build():
    python tests/golden/make_intra_golden.py"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import intra_common as ic  # noqa: E402


def main():
    L = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "libsvtav1_ref.so"))
    L.setup_common_rtcd_internal(0)
    L.setup_rtcd_internal(0)
    plane = ic.mixed_frame(200, 136)
    out = {"plane": plane}
    for me, sfx in ((12, ""), (0, "_0"), (8, "_8")):
        m, c = ic.ref_ois(L, plane, 200, 136, me)
        out["mode" + sfx] = m
        out["cost" + sfx] = c.astype(np.int32)
    np.savez_compressed(os.path.join(HERE, "intra_ois_200x136.npz"), **out)
    print("winners", np.bincount(out["mode"].ravel(), minlength=13).tolist())


if __name__ == "__main__":
    main()
