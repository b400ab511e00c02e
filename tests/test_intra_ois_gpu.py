"""GPU: svt_hip_intra_ois_picture_dev against the reference's own open-loop intra search (tests/intra_common.py: ref_ois), every macroblock, mode and cost."""
import ctypes as C
import os

import numpy as np
import pytest

import intra_common as ic
from conftest import ROOT

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "intra_ois_200x136.npz")


def _compare(hip, L, plane, w, h, mode_end=12, min_share=None, min_count=None):
    rm, rc = ic.ref_ois(L, plane, w, h, mode_end)
    hist = np.bincount(rm.ravel(), minlength=13)
    print(f"{w}x{h} mode_end {mode_end}: reference winners {hist.tolist()}, cost {int(rc.min())} .. {int(rc.max())}")
    # condition on the input, on the reference's result, before the device is looked at
    if min_share is not None:
        assert (hist >= min_share * rm.size).all(), f"generator no longer exercises every mode: {hist.tolist()}"
    if min_count is not None:
        assert (hist[:mode_end + 1] >= min_count).all(), f"generator no longer exercises every mode: {hist.tolist()}"
    dm, dc = ic.device_ois(hip, plane, w, h, mode_end)
    bad = np.argwhere((dm != rm) | (dc != rc))
    assert bad.size == 0, f"{len(bad)} of {rm.size} macroblocks differ; first (row, col) {bad[0].tolist()}: device ({dm[tuple(bad[0])]}, {dc[tuple(bad[0])]}) " \
                          f"reference ({rm[tuple(bad[0])]}, {rc[tuple(bad[0])]})"
    return rm, rc


@pytest.mark.parametrize("mode_end", [12, 11, 8, 0])
def test_cif_mixed(hip, ref, mode_end):
    _compare(hip, ref, ic.mixed_frame(352, 288), 352, 288, mode_end, min_count=1 if mode_end == 12 else None)


def test_trailing_half_macroblocks(hip, ref):
    """200x136: the last macroblock column is 8 wide, the last row 8 high; neighbour counts are clipped at the picture."""
    rm, _ = _compare(hip, ref, ic.mixed_frame(200, 136), 200, 136)
    assert rm.size == 117


def test_noise(hip, ref):
    p = ic.noise(np.random.default_rng(20260 + 176), 176, 144)
    _compare(hip, ref, p, 176, 144)


def test_1080p_mixed(hip, ref):
    _compare(hip, ref, ic.mixed_frame(1920, 1080), 1920, 1080, min_share=0.005)


def test_4k_mixed(hip, ref):
    _compare(hip, ref, ic.mixed_frame(3840, 2160), 3840, 2160, min_share=0.005)


def test_unaligned_base_and_stride(hip, ref):
    """The CIF frame inside a 300 x 416 buffer at column 3: base address not a multiple of 4, stride != width; the view goes to both sides."""
    p = ic.mixed_frame(352, 288)
    buf = np.zeros((300, 416), np.uint8)
    buf[:288, 3:3 + 352] = p
    view = buf[:288, 3:3 + 352]
    rm, rc = _compare(hip, ref, view, 352, 288)
    rm0, rc0 = ic.ref_ois(ref, p, 352, 288)
    assert (rm == rm0).all() and (rc == rc0).all()


def test_flat_plane_first_mode_wins(hip, ref):
    p = np.full((64, 64), 128, np.uint8)
    rm, rc = _compare(hip, ref, p, 64, 64)
    assert (rm == 0).all() and (rc == 0).all()


def test_piecewise_flat_ties(hip, ref):
    """Ties at cost 0 between different sets of modes: the first mode in mode order must win."""
    p = np.kron(np.random.default_rng(7).integers(30, 220, (9, 11)), np.ones((32, 32)))[:288, :352]
    p = np.ascontiguousarray(np.roll(p, (8, 8), (0, 1)).astype(np.uint8))
    rm, rc = _compare(hip, ref, p, 352, 288)
    assert int((rc == 0).sum()) > 200


def test_golden_without_the_reference(hip):
    """The stored result of the 200x136 case (tests/golden/make_intra_golden.py): holds where the reference library is absent."""
    g = np.load(GOLDEN)
    dm, dc = ic.device_ois(hip, np.ascontiguousarray(g["plane"]), 200, 136)
    assert (dm == g["mode"]).all() and (dc == g["cost"]).all()
    for me in (0, 8):
        dm, dc = ic.device_ois(hip, np.ascontiguousarray(g["plane"]), 200, 136, me)
        assert (dm == g[f"mode_{me}"]).all() and (dc == g[f"cost_{me}"]).all()


def test_bad_arguments_with_a_context(hip, pkg):
    L = pkg.lib()
    p = ic.mixed_frame(64, 64)
    d = hip.to_device(p); dm = hip.empty(16); dc = hip.empty(64)
    f = lambda **k: L.svt_hip_intra_ois_picture_dev(hip.h, k.get("src", d), k.get("stride", 64), k.get("w", 64), k.get("h", 64), k.get("mode_end", 12),
                                                    k.get("mode", dm), k.get("cost", dc))
    try:
        assert f() == 0
        for bad in (dict(w=60), dict(h=60), dict(w=8), dict(h=8), dict(mode_end=13), dict(mode_end=-1), dict(stride=63), dict(w=56, stride=56), dict(src=None),
                    dict(mode=None), dict(cost=None)):
            assert f(**bad) == 2, bad
        assert f(w=56, h=56) == 0   # stride 64 = ceil16(56)
        hip.check(L.svt_hip_sync(hip.h), "sync")
    finally:
        hip.free(d, dm, dc)
