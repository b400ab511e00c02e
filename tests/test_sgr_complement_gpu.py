"""GPU parity of the complement form of the 64 x 32-tile self-guided kernels (sgr.hip: the byte table of 256 - A' indexed by the unclamped z, the packed words
(256 - A') << 20 | B', flt - u as ab * -(x + 2^20) + W) against the oracle, on content chosen to sit on the bounds of that form:

    flat 0 / flat maximum            z = 0, 256 - A' = 255 at every position, ab = 8160, the largest B'
    0 / maximum checkerboards with   z in the thousands: table entries far past index 255 (period 1 for r = 1, period 2 and the
    periods 1 and 2, half-plane edge half-plane edge for the 5 x 5 window as well)
    uniform noise, isolated spikes   the general case, and single positions with a large z among flat ones

Planes are 136 x 104 with restoration units of 64: 2 x 2 units, interior tiles (the straight-line body), ragged right and bottom tiles (the general body), as luma
and as a 4:2:0 chroma plane (the tile grid is shifted up by 8 or 4 rows), in the three sample formats, all 16 parameter sets."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import ptr

pytestmark = pytest.mark.gpu
EXT = 3
W, H, US = 136, 104, 64
NU = 4
FORMATS = {"u8": (np.uint8, 8), "u16-8": (np.uint16, 8), "u16-10": (np.uint16, 10)}
CONTENTS = ("flat0", "flatmax", "checker1", "checker2", "edge", "noise", "spikes")


def _content(name, mx):
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(len(name) * 131 + mx)
    if name == "flat0": return np.zeros((H, W), np.int64)
    if name == "flatmax": return np.full((H, W), mx, np.int64)
    if name == "checker1": return mx * ((xx + yy) & 1)
    if name == "checker2": return mx * (((xx >> 1) + (yy >> 1)) & 1)
    if name == "edge": return mx * (xx + yy // 3 >= 70)            # a slanted 0 / maximum edge through the interior tiles and both ragged ones
    if name == "noise": return rng.integers(0, mx + 1, (H, W))
    d = np.where(yy < H // 2, 0, mx)                               # spikes: isolated maxima in flat 0, isolated zeros in flat maximum
    d[3::7, 2::5] = mx - d[3::7, 2::5]
    return d


@functools.lru_cache(maxsize=None)
def _planes(name, fmt):
    """(source, 3-sample-extended degraded picture, deblocked picture) of a case; the source is a smoothed, dimmed copy so that the filters have something to gain"""
    dt, bd = FORMATS[fmt]
    mx = (1 << bd) - 1
    dgd = _content(name, mx)
    p = np.pad(dgd, 1, mode="edge")
    box = sum(p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) // 9
    yy, xx = np.mgrid[0:H, 0:W]
    src = np.clip((3 * box + dgd) // 4 + ((xx + 2 * yy) % 23 - 11) * (mx // 255), 0, mx)
    if name.startswith("flat"): src = mx - dgd                       # the largest dat - src there is
    dbl = np.roll(dgd, (1, 2), (0, 1))                               # what the stripe boundaries see instead: still 0 / maximum content
    dbl[::9, ::4] = mx - dbl[::9, ::4]
    planes = np.ascontiguousarray(src.astype(dt)), np.ascontiguousarray(np.pad(dgd.astype(dt), EXT, mode="edge")), np.ascontiguousarray(dbl.astype(dt))
    for a in planes: a.setflags(write=False)
    return planes


def _off(ext):
    return (EXT * ext.shape[1] + EXT) * ext.itemsize


@pytest.mark.parametrize("ss", [0, 1])
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", CONTENTS)
def test_search_sums(hip, orc, name, fmt, ss):
    """The five projection sums of every (unit, set): sgr_search8_kernel<.., 0>, all sets and a sparse mask (sets 11 - 13 are copies of 2 / 5 / 8 inside the kernel)."""
    dt, bd = FORMATS[fmt]
    src, ext, _ = _planes(name, fmt)
    st = ext.shape[1]
    d_ext, d_src = hip.to_device(ext), hip.to_device(src)
    for mask in (0xFFFF, 0x7801):
        e_sums = np.zeros((NU, 16, 5), np.int64)
        orc.orc_sgr_search_plane(C.c_void_p(ext.ctypes.data + _off(ext)), ext.itemsize, st, ptr(src), W, W, H, ss, ss, US, bd, mask, ptr(e_sums))
        d_sums = hip.to_device(np.zeros_like(e_sums))
        hip.check(hip.L.svt_hip_sgr_search_plane_dev(hip.h, ext.itemsize, bd, d_ext.value + _off(ext), st, d_src, W, W, H, US, ss, mask, d_sums), "search")
        got = hip.to_host(d_sums, e_sums.shape, np.int64)
        hip.free(d_sums)
        assert np.array_equal(got, e_sums), (name, fmt, ss, hex(mask), np.argwhere(got != e_sums)[:5])
    hip.free(d_ext, d_src)


_UNITS = {}


def _expected_units(orc, name, fmt, ss):
    """the oracle's unit search of a case (xqd, errors, best set), computed once: the picture-level and the packed-word tests share it"""
    key = (name, fmt, ss)
    if key not in _UNITS:
        dt, bd = FORMATS[fmt]
        src, ext, _ = _planes(name, fmt)
        e_xqd = np.zeros((NU, 16, 2), np.int32); e_err = np.zeros((NU, 16), np.int64); e_best = np.zeros(NU, np.uint8)
        orc.orc_sgr_search_units_plane(C.c_void_p(ext.ctypes.data + _off(ext)), ext.itemsize, ext.shape[1], ptr(src), W, W, H, ss, ss, US, bd, 0xFFFF, ptr(e_xqd), ptr(e_err), ptr(e_best))
        for a in (e_xqd, e_err, e_best): a.setflags(write=False)
        _UNITS[key] = (e_xqd, e_err, e_best)
    return _UNITS[key]


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", CONTENTS)
def test_search_units_picture(hip, pkg, orc, name, fmt):
    """svt_hip_sgr_search_units_picture_dev on a luma and a 4:2:0 chroma plane of the content in one call: the difference planes (sgr_search8_kernel<.., 1>, the six-byte
    form) feed the walk, so xqd, the errors and the best set of every unit follow from flt - u of every sample and set."""
    dt, bd = FORMATS[fmt]
    src, ext, _ = _planes(name, fmt)
    st = ext.shape[1]
    L = hip.L
    jobs = (pkg.SgrUnitsPlaneDev * 2)()
    nbytes = L.svt_hip_sgr_search_units_scratch_bytes(W, H, US)
    d_ext, d_src = hip.to_device(ext), hip.to_device(src)
    outs = []
    for ss in (0, 1):
        d = dict(scr=hip.empty(nbytes), xqd=hip.to_device(np.zeros((NU, 16, 2), np.int32)), err=hip.to_device(np.zeros((NU, 16), np.int64)), best=hip.empty(NU), bx=hip.empty(NU * 8))
        outs.append(d)
        jobs[ss] = pkg.SgrUnitsPlaneDev(d_ext.value + _off(ext), st, d_src.value, W, W, H, US, ss, 0xFFFF, d["xqd"].value, d["err"].value, d["best"].value, d["bx"].value,
                                        d["scr"].value, nbytes)
    hip.check(L.svt_hip_sgr_search_units_picture_dev(hip.h, ext.itemsize, bd, 2, jobs), "units picture dev")
    for ss, d in enumerate(outs):
        e_xqd, e_err, e_best = _expected_units(orc, name, fmt, ss)
        g_xqd = hip.to_host(d["xqd"], e_xqd.shape, np.int32); g_err = hip.to_host(d["err"], e_err.shape, np.int64); g_best = hip.to_host(d["best"], e_best.shape, np.uint8)
        hip.free(*d.values())
        assert np.array_equal(g_err, e_err), (name, fmt, ss, np.argwhere(g_err != e_err)[:8])
        assert np.array_equal(g_xqd, e_xqd) and np.array_equal(g_best, e_best), (name, fmt, ss)
    hip.free(d_ext, d_src)


@pytest.mark.parametrize("ss", [0, 1])
@pytest.mark.parametrize("fmt", ["u8", "u16-8"])
@pytest.mark.parametrize("name", CONTENTS)
def test_search_units_packed_words_narrow_limit(hip, orc, name, fmt, ss):
    """The packed difference words (sgr_search8_kernel<.., 2>, bit depth 8) with the escape limit narrowed to 3 (|flt - u| is small on all of this content: where the variance is
    large the filters pass the sample through): samples with |flt - u| >= 3 leave through the exact escape lists, the others through the 11-bit fields."""
    dt, bd = FORMATS[fmt]
    src, ext, _ = _planes(name, fmt)
    e_xqd, e_err, e_best = _expected_units(orc, name, fmt, ss)
    L = hip.L
    os.environ["SVT_HIP_SGR_PACKED"] = "1"; os.environ["SVT_HIP_SGR_ESC_LIM"] = "3"
    try:
        nbytes = L.svt_hip_sgr_search_units_scratch_bytes(W, H, US)
        d_ext, d_src = hip.to_device(ext), hip.to_device(src)
        d_scr = hip.empty(nbytes); d_xqd = hip.empty(NU * 16 * 8); d_err = hip.empty(NU * 16 * 8); d_best = hip.empty(NU); d_bx = hip.empty(NU * 8)
        hip.check(L.svt_hip_sgr_search_units_plane_dev(hip.h, ext.itemsize, bd, d_ext.value + _off(ext), ext.shape[1], d_src, W, W, H, US, ss, 0xFFFF, d_xqd, d_err, d_best, d_bx,
                                                       d_scr, nbytes), "units dev, packed words")
    finally:
        os.environ.pop("SVT_HIP_SGR_PACKED", None); os.environ.pop("SVT_HIP_SGR_ESC_LIM", None)
    g_xqd = hip.to_host(d_xqd, e_xqd.shape, np.int32); g_err = hip.to_host(d_err, e_err.shape, np.int64); g_best = hip.to_host(d_best, e_best.shape, np.uint8)
    stats = hip.to_host(d_scr, (32,), np.uint32)   # [2] unfinished walks, [4] listed samples the walks added one by one
    hip.free(d_ext, d_src, d_scr, d_xqd, d_err, d_best, d_bx)
    assert np.array_equal(g_err, e_err), (name, fmt, ss, np.argwhere(g_err != e_err)[:8])
    assert np.array_equal(g_xqd, e_xqd) and np.array_equal(g_best, e_best), (name, fmt, ss)
    assert stats[2] == 0
    if name in ("flatmax", "noise"): assert stats[4] > 1000, stats[:6]   # flt0 - u is 4 on flat maximum, and beyond 3 on most noise samples in the weaker sets


@pytest.mark.parametrize("ss", [0, 1])
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", CONTENTS)
def test_apply_with_stripes(hip, orc, name, fmt, ss):
    """svt_hip_sgr_apply_plane_dev (lr_apply8_kernel) with the deblocked picture across the stripe boundaries: four rounds give each of the four units each of the 16 sets."""
    dt, bd = FORMATS[fmt]
    src, ext, dbl = _planes(name, fmt)
    st = ext.shape[1]
    rng = np.random.default_rng(9 + ss)
    d_ext, d_dbl, d_dst = hip.to_device(ext), hip.to_device(dbl), hip.to_device(np.zeros((H, W), dt))
    changed = False
    for rnd in range(4):
        u_ep = ((4 * rnd + np.arange(NU) * 5) % 16).astype(np.uint8)
        u_xqd = np.stack([rng.integers(-96, 32, NU), rng.integers(-32, 96, NU)], 1).astype(np.int32)
        work = ext.copy()
        exp = np.zeros((H, W), dt)
        orc.orc_sgr_apply_plane(ptr(dbl), W, C.c_void_p(work.ctypes.data + _off(ext)), st, ext.itemsize, W, H, ss, ss, US, bd, ptr(u_ep), ptr(u_xqd), ptr(exp), W)
        assert np.array_equal(work, ext)
        d_ep, d_xqd = hip.to_device(u_ep), hip.to_device(u_xqd)
        hip.check(hip.L.svt_hip_sgr_apply_plane_dev(hip.h, ext.itemsize, bd, d_ext.value + _off(ext), st, d_dst, W, W, H, US, ss, d_dbl, W, d_ep, d_xqd), "apply")
        got = hip.to_host(d_dst, (H, W), dt)
        hip.free(d_ep, d_xqd)
        assert np.array_equal(got, exp), (name, fmt, ss, rnd, np.argwhere(got != exp)[:5])
        changed |= bool((exp != ext[EXT:EXT + H, EXT:EXT + W]).any())   # (binary content at bit depth 8 passes through: A' = 256 or b = 255 a)
    hip.free(d_ext, d_dbl, d_dst)
    if name == "noise": assert changed, "the filter must move some sample of this content"
