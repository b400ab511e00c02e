"""GPU: the normative super-resolution upscale and the scaler (svt-av1_amd/csrc/resize.hip) through Context.superres_upscale_planes / Context.resize_planes,
bit for bit against the reference's [highbd_]upscale_normative_rect (when oracle/_ref/libsvtav1_ref.so is there) and against the restatements of
tests/resize_common.py, which tests/test_resize_ref_cpu.py proves against the reference: the recorded planes of tests/golden/resize_planes.npz and the clamped
whole-row form of the upscale."""
import ctypes as C
import os

import numpy as np
import pytest

import resize_common as rc
import test_resize_abi as abi
from conftest import ROOT

pytestmark = pytest.mark.gpu

FORMATS = [(np.uint8, 8), (np.uint16, 8), (np.uint16, 10), (np.uint16, 12)]
SENTINEL, FILL = 0x5A, 0xA5


@pytest.fixture(scope="module")
def refp():
    """the reference, or None where it has not been built: the restatements then stand alone"""
    path = os.path.join(ROOT, "oracle", "_ref", "libsvtav1_ref.so")
    if not os.path.exists(path):
        return None
    L = C.CDLL(path)
    L.setup_common_rtcd_internal(0)   # as conftest's `ref`: svt_memcpy and the like are dispatch pointers, NULL until then
    L.setup_rtcd_internal(0)
    return rc.prepare(L)


def _rand(seed, h, w, dtype, bd):
    return np.random.default_rng(seed).integers(0, 1 << bd, (h, w)).astype(dtype)


def _want_upscale(refp, p, out_w, bd):
    want = rc.numpy_upscale(p, out_w, bd)
    if refp is not None:
        assert np.array_equal(rc.ref_upscale(refp, p, out_w, bd), want)
    return want


def _embed(plane, top, left, bottom, right, value):
    """`plane` as a view inside a larger array filled with `value`"""
    big = np.full((plane.shape[0] + top + bottom, plane.shape[1] + left + right), value, plane.dtype)
    view = big[top:top + plane.shape[0], left:left + plane.shape[1]]
    view[...] = plane
    return view


def _margin_intact(view, value):
    """`view` as Context returns it -- a view of a fresh copy of the whole destination array: everything of that array outside the view still holds `value`"""
    full = view.base
    assert isinstance(full, np.ndarray) and full.ndim == 2
    top, left = divmod((view.ctypes.data - full.ctypes.data) // view.itemsize, full.shape[1])
    mask = np.ones(full.shape, bool)
    mask[top:top + view.shape[0], left:left + view.shape[1]] = False
    return mask.sum() > 0 and bool((full[mask] == value).all())


@pytest.mark.parametrize("dtype,bd", FORMATS)
def test_upscale_every_width_denominator_rows(hip, refp, dtype, bd):
    for rows in rc.UPSCALE_ROWS:
        for w in rc.UPSCALE_WIDTHS:
            p = _rand(rows * 1000 + w + bd, rows, w, dtype, bd)
            for d in rc.SUPERRES_DENOMS:
                out_w = w * d // 8
                got, = hip.superres_upscale_planes([p], [out_w], bd=bd)
                assert np.array_equal(got, _want_upscale(refp, p, out_w, bd)), (rows, w, d)


@pytest.mark.parametrize("dtype,bd", FORMATS)
def test_upscale_alternating_content_binds_both_clips(hip, refp, dtype, bd):
    """0 / max alternating along the row: the filter overshoots both ways (tests/test_resize_ref_cpu.py shows the unclipped sums), the clip's upper bound is the
    bit depth's"""
    maxv = (1 << bd) - 1
    p = ((np.arange(90)[None, :] & 1) * maxv).astype(dtype).repeat(2, axis=0)
    got, = hip.superres_upscale_planes([p], [101], bd=bd)
    assert np.array_equal(got, _want_upscale(refp, p, 101, bd)) and got.min() == 0 and got.max() == maxv


@pytest.mark.parametrize("dtype,bd", [(np.uint8, 8), (np.uint16, 10)])
def test_upscale_three_planes_of_a_picture_in_one_call(hip, refp, dtype, bd):
    """4:2:0: the chroma planes are half as wide and half as high, so the launch's grid is the luma's and chroma workgroups beyond their plane sit out;
    1090 columns: more than one 1024-sample segment per row"""
    for (w, h), out_w in [((90, 38), 129), ((681, 6), 1090)]:
        planes = [_rand(1, h, w, dtype, bd), _rand(2, h // 2, (w + 1) // 2, dtype, bd), _rand(3, h // 2, (w + 1) // 2, dtype, bd)]
        widths = [out_w, (out_w + 1) // 2, (out_w + 1) // 2]
        got = hip.superres_upscale_planes(planes, widths, bd=bd)
        for g, p, ow in zip(got, planes, widths):
            assert np.array_equal(g, _want_upscale(refp, p, ow, bd))


@pytest.mark.parametrize("dtype,bd", [(np.uint8, 8), (np.uint16, 10)])
def test_upscale_on_embedded_views(hip, refp, dtype, bd):
    """the source's margin holds a value that differs from the edge samples: a read outside [0, in_w) would show; the destination's margin must survive"""
    for w, out_w, rows in [(33, 57, 5), (129, 130, 3), (16, 32, 2)]:
        p = _rand(w, rows, w, dtype, bd)
        p[:, 0] = p[:, -1] = 200   # edge samples unlike the sentinel
        src = _embed(p, 2, 9, 3, 7, SENTINEL)
        dst = _embed(np.full((rows, out_w), FILL, dtype), 1, 6, 2, 11, FILL)
        got, = hip.superres_upscale_planes([src], [out_w], dst=[dst], bd=bd)
        assert np.array_equal(got, _want_upscale(refp, p, out_w, bd)), (w, out_w)
        assert _margin_intact(got, FILL)


@pytest.mark.parametrize("dtype,bd", [(np.uint8, 8), (np.uint16, 10)])
def test_upscale_boundary_lines(hip, refp, dtype, bd):
    """save_deblock_boundary_lines: rows r, r + 1 upscaled alone (rows = 2, and the last row alone with rows = 1) equal those rows of the whole plane's upscale"""
    p = _rand(5, 70, 90, dtype, bd)
    whole, = hip.superres_upscale_planes([p], [157], bd=bd)
    assert np.array_equal(whole, _want_upscale(refp, p, 157, bd))
    for r in (0, 7, 62, 68):
        two, = hip.superres_upscale_planes([p[r:r + 2]], [157], bd=bd)
        assert np.array_equal(two, whole[r:r + 2]), r
    one, = hip.superres_upscale_planes([p[69:70]], [157], bd=bd)
    assert np.array_equal(one, whole[69:70])


@pytest.mark.parametrize("t,bd", [("u8", 8), ("u16", 10)])
def test_scaler_every_golden_case(hip, t, bd):
    golden = rc.load_golden()
    for name, ih, iw, oh, ow, _ in rc.golden_shapes():
        src, want = golden[name, t]
        got, = hip.resize_planes([src.copy()], [(oh, ow)], bd=bd)
        assert np.array_equal(got, want), name


@pytest.mark.parametrize("dtype,bd", [(np.uint8, 8), (np.uint16, 10)])
def test_scaler_picture_and_both_axes(hip, dtype, bd):
    """a 4:2:0 picture scaled in width alone, three planes in one call (no scratch); one plane scaled on both axes; a picture whose planes take different
    paths (width alone, height alone with three column stages, both)"""
    planes = [_rand(11, 288, 352, dtype, bd), _rand(12, 144, 176, dtype, bd), _rand(13, 144, 176, dtype, bd)]
    shapes = [(288, 235), (144, 118), (144, 118)]
    for g, p, s in zip(hip.resize_planes(planes, shapes, bd=bd), planes, shapes):
        assert np.array_equal(g, rc.numpy_resize_plane(p, s[0], s[1], bd))
    p = _rand(14, 70, 130, dtype, bd)
    for shape in [(45, 77), (9, 200), (70, 61), (31, 130)]:
        got, = hip.resize_planes([p], [shape], bd=bd)
        assert np.array_equal(got, rc.numpy_resize_plane(p, shape[0], shape[1], bd)), shape
    planes = [_rand(15, 40, 300, dtype, bd), _rand(16, 100, 48, dtype, bd), _rand(17, 64, 65, dtype, bd)]
    shapes = [(40, 75), (12, 48), (15, 16)]
    for g, q, s in zip(hip.resize_planes(planes, shapes, bd=bd), planes, shapes):
        assert np.array_equal(g, rc.numpy_resize_plane(q, s[0], s[1], bd)), s


@pytest.mark.parametrize("dtype,bd", [(np.uint8, 8), (np.uint16, 12)])
def test_scaler_on_embedded_views(hip, dtype, bd):
    for (ih, iw), (oh, ow) in [((40, 48), (25, 30)), ((20, 33), (20, 50)), ((33, 20), (50, 20))]:
        p = _rand(ih * iw, ih, iw, dtype, bd)
        src = _embed(p, 3, 5, 2, 9, SENTINEL)
        dst = _embed(np.full((oh, ow), FILL, dtype), 2, 7, 1, 4, FILL)
        got, = hip.resize_planes([src], [(oh, ow)], dst=[dst], bd=bd)
        assert np.array_equal(got, rc.numpy_resize_plane(p, oh, ow, bd)), (ih, iw, oh, ow)
        assert _margin_intact(got, FILL)


@pytest.mark.parametrize("dtype,bd", [(np.uint8, 8), (np.uint16, 10)])
def test_equal_sizes_copy_and_leave_the_scratch(hip, dtype, bd):
    p = _rand(3, 37, 53, dtype, bd)
    src = _embed(p, 1, 2, 3, 4, SENTINEL)
    dst = _embed(np.full(p.shape, FILL, dtype), 4, 3, 2, 1, FILL)
    scratch = np.full(4096, 0xC3, np.uint8)
    got, = hip.resize_planes([src], [p.shape], dst=[dst], bd=bd, scratch=scratch)
    assert np.array_equal(got, p) and _margin_intact(got, FILL) and (scratch == 0xC3).all()


def test_refusals_with_a_live_context(hip, pkg):
    L = hip.L
    d = [hip.empty(1 << 20) for _ in range(3)]
    try:
        p, p2, p3 = (x.value for x in d)
        assert abi.call_upscale(pkg, L, hip.h, p, p2) == 0 and abi.call_resize(pkg, L, hip.h, p, p2, p3) == 0
        hip.check(L.svt_hip_sync(hip.h), "sync")
        for c in abi.UPSCALE_BAD:
            assert abi.call_upscale(pkg, L, hip.h, p, p2, **c) == abi.BAD_ARG, c
            assert L.svt_hip_last_error(hip.h).decode().startswith("svt_hip_superres_upscale_planes_dev: bad argument"), c
        for c in abi.RESIZE_BAD:
            assert abi.call_resize(pkg, L, hip.h, p, p2, p3, **c) == abi.BAD_ARG, c
            assert L.svt_hip_last_error(hip.h).decode().startswith("svt_hip_resize_planes_dev: "), c
        hip.check(L.svt_hip_sync(hip.h), "sync")
    finally:
        hip.free(*d)
