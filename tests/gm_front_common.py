"""Shared by the tests of the global-motion front half (corners, cross-correlation, correspondences): the reference side -- svt_av1_fast_corner_detect,
svt_aom_fast9_detect / svt_aom_fast9_score, svt_av1_compute_cross_correlation_c and svt_av1_determine_correspondence of libsvtav1_ref.so through ctypes on numpy
buffers -- the pictures, the point lists and the cases the CPU and GPU tests share.  Reference results are computed once per process."""
import ctypes as C
import functools

import numpy as np

import gm_common as g

VP = C.c_void_p
MAX_CORNERS = 4096
_prepared = set()
_libc = C.CDLL(None)
_libc.free.argtypes = [VP]


def prepare(L):
    if id(L) in _prepared:
        return L
    i = C.c_int
    L.svt_av1_fast_corner_detect.argtypes = [VP, i, i, i, VP, i]
    L.svt_av1_fast_corner_detect.restype = i
    L.svt_aom_fast9_detect.argtypes = [VP, i, i, i, i, C.POINTER(i)]
    L.svt_aom_fast9_detect.restype = VP
    L.svt_aom_fast9_score.argtypes = [VP, i, VP, i, i]
    L.svt_aom_fast9_score.restype = VP
    L.svt_av1_compute_cross_correlation_c.argtypes = [VP, i, i, i, VP, i, i, i]
    L.svt_av1_compute_cross_correlation_c.restype = C.c_double
    L.svt_av1_determine_correspondence.argtypes = [VP, VP, i, VP, VP, i, i, i, i, i, VP]
    L.svt_av1_determine_correspondence.restype = i
    _prepared.add(id(L))
    return L


def _p(a):
    return a.ctypes.data_as(VP)


def _stride(a):
    assert a.dtype == np.uint8 and a.ndim == 2 and a.strides[1] == 1
    return a.strides[0]


# ------------------------------------------------------------------------------------------------ the reference
def ref_corners(L, plane, max_points=MAX_CORNERS):
    """svt_av1_fast_corner_detect -> int32 [n][2] x, y"""
    h, w = plane.shape
    out = np.full((min(max_points, w * h), 2), -7, np.int32)
    n = prepare(L).svt_av1_fast_corner_detect(_p(plane), w, h, _stride(plane), _p(out), max_points)
    return out[:n].copy()


def ref_kept(L, plane):
    """how many corners the suppression keeps before svt_av1_fast_corner_detect truncates the list"""
    return len(ref_corners(L, plane, plane.shape[0] * plane.shape[1]))


def ref_raw_corners(L, plane, barrier=18):
    """svt_aom_fast9_detect + svt_aom_fast9_score -> (int32 [n][2] x, y in raster order, int32 [n] scores)"""
    h, w = plane.shape
    n = C.c_int(0)
    pc = prepare(L).svt_aom_fast9_detect(_p(plane), w, h, _stride(plane), barrier, C.byref(n))
    xy = np.ctypeslib.as_array(C.cast(pc, C.POINTER(C.c_int32)), (n.value, 2)).copy() if n.value else np.zeros((0, 2), np.int32)
    ps = L.svt_aom_fast9_score(_p(plane), _stride(plane), pc, n.value, barrier)
    sc = np.ctypeslib.as_array(C.cast(ps, C.POINTER(C.c_int32)), (n.value,)).copy() if n.value else np.zeros(0, np.int32)
    _libc.free(pc); _libc.free(ps)
    return xy, sc


def ref_cross_correlation(L, im1, im2, pairs):
    """svt_av1_compute_cross_correlation_c of every x1, y1, x2, y2 -> float64 [n]"""
    f = prepare(L).svt_av1_compute_cross_correlation_c
    p1, s1, p2, s2 = _p(im1), _stride(im1), _p(im2), _stride(im2)
    return np.array([f(p1, s1, int(a), int(b), p2, s2, int(c), int(d)) for a, b, c, d in pairs], np.float64)


def ref_correspondences(L, src, src_points, rf, ref_points):
    """svt_av1_determine_correspondence (both planes at the source's size) -> int32 [n][4] x, y, rx, ry"""
    h, w = src.shape
    assert rf.shape[0] >= h and rf.shape[1] >= w
    sp = np.ascontiguousarray(src_points, np.int32).reshape(-1, 2)
    rp = np.ascontiguousarray(ref_points, np.int32).reshape(-1, 2)
    out = np.full((max(len(sp), 1), 4), -7, np.int32)
    n = prepare(L).svt_av1_determine_correspondence(_p(src), _p(sp), len(sp), _p(rf), _p(rp), len(rp), w, h, _stride(src), _stride(rf), _p(out))
    return out[:n].copy()


# ------------------------------------------------------------------------------------------------ FAST-9, closed form
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def closed_form_scores(plane, barrier=18):
    """int [h][w]: max(B, D) - 1 where that is >= barrier, else 0; B = max over the 16 arcs of 9 ring pixels of min(ring - p), D the same of p - ring"""
    a = plane.astype(np.int32)
    h, w = a.shape
    out = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return out
    p = a[3:h - 3, 3:w - 3]
    d = np.stack([a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - p for dx, dy in RING])
    best = np.full(p.shape, -256, np.int32)
    for s in range(16):
        arc = d[[(s + k) & 15 for k in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))
    sc = best - 1
    out[3:h - 3, 3:w - 3] = np.where(sc >= barrier, sc, 0)
    return out


# ------------------------------------------------------------------------------------------------ pictures
def _frozen(a):
    a = np.ascontiguousarray(a, np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def tex(seed, w, h, dx=0, dy=0, passes=3):
    """a w x h crop of a low-pass noise texture; (dx, dy) moves the crop's origin, so two crops of one seed are the same picture shifted"""
    m = 16
    t = g.texture(seed, h + 2 * m, w + 2 * m, passes)
    return _frozen(np.clip(np.floor(t[m + dy:m + dy + h, m + dx:m + dx + w] + 0.5), 0, 255))


@functools.lru_cache(maxsize=None)
def noise(seed, w, h):
    return _frozen(np.random.default_rng(seed).integers(0, 256, (h, w)))


@functools.lru_cache(maxsize=None)
def spikes(w, h, inverse=False):
    """isolated 255 samples on 0 (or 0 on 255), 9 apart, one of them at (3, 3) and one at (w - 4, h - 4): the first and last pixels that can be corners"""
    a = np.zeros((h, w), np.uint8)
    a[3::9, 3::9] = 255
    a[h - 4, w - 4] = 255
    return _frozen(255 - a if inverse else a)


@functools.lru_cache(maxsize=None)
def blocks(w=40, h=30):
    """a 2x2 block and a 1x3 bar of 200 on 0: neighbouring corners of equal score remove each other"""
    a = np.zeros((h, w), np.uint8)
    a[10:12, 10:12] = 200
    a[20, 25:28] = 200
    return _frozen(a)


@functools.lru_cache(maxsize=None)
def flat(w, h, v=128):
    return _frozen(np.full((h, w), v))


@functools.lru_cache(maxsize=None)
def tiled(seed, w, h, period):
    """noise of the given period in both directions: patches a period apart are identical, their correlations tie exactly"""
    t = np.random.default_rng(seed).integers(0, 256, (period, period))
    return _frozen(np.tile(t, (h // period + 1, w // period + 1))[:h, :w])


@functools.lru_cache(maxsize=None)
def rot_pair(seed, w, h):
    s, r = g.picture_pair(seed, w, h, g.ROT)
    return _frozen(s), _frozen(r)


def corner_pictures():
    """name -> plane, the pictures of the corner tests"""
    return dict(tex_96x80=tex(21, 96, 80), tex_100x76_p1=tex(22, 100, 76, passes=1), noise_90x50=noise(23, 90, 50), noise_352x288=noise(24, 352, 288),
                spikes=spikes(40, 31), spikes_inverse=spikes(40, 31, True), blocks=blocks(), flat=flat(33, 20), tiny_8x8=noise(25, 8, 8),
                tiny_8x8_spike=_frozen(np.pad(np.array([[255, 0], [0, 0]], np.uint8), 3)))


# ------------------------------------------------------------------------------------------------ correspondence cases
def border_points(w, h):
    """points within 6 of every border, on both sides of each eligibility bound, negative and beyond-picture coordinates, and a few well inside"""
    xs = [-(1 << 30), -7, -1, 0, 5, 6, 7, w // 2, w - 8, w - 7, w - 6, w - 1, w, w + 6, 1 << 30]
    ys = [-(1 << 30), -1, 0, 5, 6, h // 2, h - 7, h - 6, h, 1 << 30]
    return np.array([(x, y) for y in ys for x in xs], np.int64).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(L, name):
    """-> (src, ref, src_points, ref_points); L = the reference (its corners are the lists of most cases)"""
    c = lambda a: ref_corners(L, a)
    rng = np.random.default_rng(31)
    if name == "shifted_96x80":
        s, r = tex(21, 96, 80), tex(21, 96, 80, dx=-3, dy=2)
        return s, r, c(s), c(r)
    if name == "rot_96x80":
        s, r = rot_pair(32, 96, 80)
        return s, r, c(s), c(r)
    if name == "rot_352x288":
        s, r = rot_pair(33, 352, 288)
        return s, r, c(s), c(r)
    if name == "identical":
        s = tex(21, 96, 80)
        return s, s, c(s), c(s)
    if name == "same_corner_twice":   # reference corner 5 again at the end and corner 40 again at index 0
        s, r = tex(21, 96, 80), tex(21, 96, 80, dx=-3, dy=2)
        rp = c(r)
        return s, r, c(s), np.concatenate([rp[40:41], rp, rp[5:6]])
    if name == "periodic_ties":        # period 8 against a distance threshold of 11: up to 9 candidates with the identical patch per source corner
        s = tiled(34, 176, 144, 8)
        pts = c(s)
        return s, s, pts, pts[::-1].copy()
    if name == "periodic_ties_raster":   # the same points, the reference list in the other order: other winners
        s = tiled(34, 176, 144, 8)
        return s, s, c(s), c(s)
    if name == "borders":
        s, r = tex(21, 96, 80), tex(21, 96, 80, dx=-3, dy=2)
        b = border_points(96, 80)
        return s, r, np.concatenate([b, c(s)[:40]]), np.concatenate([c(r)[:40], b[::-1]])
    if name == "nothing_near":
        s, r = tex(21, 96, 80), tex(21, 96, 80, dx=-3, dy=2)
        sp, rp = c(s), c(r)
        return s, r, sp[sp[:, 0] < 40], rp[rp[:, 0] > 50]
    if name == "random_points":
        s, r = rot_pair(32, 96, 80)
        return s, r, rng.integers(0, [96, 80], (300, 2)).astype(np.int32), rng.integers(-2, [98, 82], (500, 2)).astype(np.int32)
    if name == "flat_pair":
        s = flat(96, 80)
        pts = rng.integers(6, [90, 74], (60, 2)).astype(np.int32)
        return s, s, pts, pts
    if name == "flat_reference":       # a textured source against a flat reference: every correlation is 0 / 0
        s = tex(21, 96, 80)
        return s, flat(96, 80), c(s), c(s)
    if name == "empty_source":
        s = tex(21, 96, 80)
        return s, s, np.zeros((0, 2), np.int32), c(s)
    if name == "empty_reference":
        s = tex(21, 96, 80)
        return s, s, c(s), np.zeros((0, 2), np.int32)
    if name == "empty_both":
        s = tex(21, 96, 80)
        return s, s, np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32)
    raise KeyError(name)


CASES = ["shifted_96x80", "rot_96x80", "rot_352x288", "identical", "same_corner_twice", "periodic_ties", "periodic_ties_raster", "borders", "nothing_near", "random_points", "flat_pair",
         "flat_reference", "empty_source", "empty_reference", "empty_both"]


def case(L, name):
    return _case(L, name)


@functools.lru_cache(maxsize=None)
def case_reference(L, name):
    s, r, sp, rp = _case(L, name)
    out = ref_correspondences(L, s, sp, r, rp)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ cross-correlation inputs
@functools.lru_cache(maxsize=None)
def correlation_inputs():
    """name -> (im1, im2, pairs [n][4]); every window lies inside"""
    rng = np.random.default_rng(41)

    def inside(n, w, h):
        return np.concatenate([rng.integers(6, [w - 6, h - 6], (n, 2)), rng.integers(6, [w - 6, h - 6], (n, 2))], 1).astype(np.int32)

    s, r = rot_pair(32, 96, 80)
    half = np.array(r)                     # the right half flat: a second window there gives 0 / 0
    half[:, 48:] = 77
    chk = _frozen(((np.indices((30, 30)).sum(0) & 1) * 255))
    per = tiled(34, 64, 48, 8)
    corners = np.array([(6, 6, 6, 6), (89, 73, 89, 73), (6, 73, 89, 6), (89, 6, 6, 73)], np.int32)
    return dict(texture=(s, r, np.concatenate([inside(20000, 96, 80), corners])),
                flat_second=(s, _frozen(half), inside(400, 96, 80)),
                zero_against_255=(flat(30, 30, 0), flat(30, 30, 255), inside(20, 30, 30)),
                against_255_zero=(flat(30, 30, 255), flat(30, 30, 0), inside(20, 30, 30)),
                checker=(chk, chk, inside(200, 30, 30)),
                checker_texture=(chk, tex(21, 30, 30), inside(200, 30, 30)),
                periodic=(per, per, np.array([(20, 20, 20 + 8 * i, 20 + 8 * j) for j in (-1, 0, 1) for i in (-1, 0, 1, 2)], np.int32)))


@functools.lru_cache(maxsize=None)
def correlation_reference(L, name):
    a, b, pairs = correlation_inputs()[name]
    return ref_cross_correlation(L, a, b, pairs)
