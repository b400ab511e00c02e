"""CPU: the reference composition of the open-loop intra search (tests/intra_common.py: ref_ois) reproduces the stored golden result and does not read the
reference's uninitialised stack arrays (the fill value of the modelled arrays does not matter)."""
import os

import numpy as np

import intra_common as ic
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "intra_ois_200x136.npz")


def test_golden_file_shape():
    g = np.load(GOLDEN)
    assert g["plane"].shape == (144, 208) and g["mode"].shape == (9, 13) and g["cost"].shape == (9, 13)
    assert (g["plane"][:, 200:] == g["plane"][:, 199:200]).all() and (g["plane"][136:] == g["plane"][135:136]).all()   # the padding rule
    assert len(np.unique(g["mode"])) >= 9


def test_ref_ois_reproduces_golden(ref):
    g = np.load(GOLDEN)
    plane = np.ascontiguousarray(g["plane"])
    m, c = ic.ref_ois(ref, plane, 200, 136)
    assert (m == g["mode"]).all() and (c == g["cost"]).all()
    m2, c2 = ic.ref_ois(ref, plane, 200, 136, fill=0x11)
    assert (m2 == m).all() and (c2 == c).all()
    for me in (0, 8):
        m, c = ic.ref_ois(ref, plane, 200, 136, me)
        assert (m == g[f"mode_{me}"]).all() and (c == g[f"cost_{me}"]).all()
