"""Shared helpers for the CDEF tests: synthetic frames, the direction-chart frames (every direction, flat blocks, exact cost ties, saturated
samples), skip maps, and drivers that run the REAL reference per-filter-block functions (svt_cdef_filter_fb + compute_cdef_dist*) the way
cdef_seg_search does (/root/reference/Source/Lib/Encoder/Codec/EbCdefProcess.c:168-273) and the way svt_av1_cdef_frame does
(Encoder/Codec/EbEncCdef.c:292-661)."""
import ctypes as C

import numpy as np

from conftest import ptr

BSTRIDE, VB, HB, VERY_LARGE = 144, 3, 8, 16384


class CdefList(C.Structure):
    _fields_ = [("by", C.c_uint8), ("bx", C.c_uint8), ("skip", C.c_uint8)]


def make_frame(w, h, bd, seed, smooth=True, dtype=None):
    """dtype: the sample type of the planes (default: uint8 at bd 8, uint16 above); np.uint16 at bd 8 = 8-bit samples in 16-bit planes"""
    rng = np.random.default_rng(seed)
    planes_src, planes_rec = [], []
    for pli in range(3):
        pw, ph = (w, h) if pli == 0 else (w // 2, h // 2)
        yy, xx = np.mgrid[0:ph, 0:pw]
        base = 90 + 50 * np.sin(xx / 9.0 + pli) * np.cos(yy / 7.0) + 0.1 * xx
        edge = 40 * (((xx + 2 * yy) // 12) % 2)
        s = (base + edge + (0 if smooth else rng.normal(0, 20, (ph, pw)))) * (1 << (bd - 8))
        src = np.clip(s, 0, (1 << bd) - 1)
        rec = np.clip(src + rng.normal(0, 6 * (1 << (bd - 8)), (ph, pw)), 0, (1 << bd) - 1)
        dt = dtype or (np.uint8 if bd == 8 else np.uint16)
        planes_src.append(np.ascontiguousarray(src.astype(dt))); planes_rec.append(np.ascontiguousarray(rec.astype(dt)))
    skip8 = (rng.random((h // 8, w // 8)) < 0.3).astype(np.uint8)
    return planes_src, planes_rec, skip8


# ---------------------------------------------------------------------------------------------------------------- direction chart
def chart_lines():
    """[8][8][8] line index of sample (I, J) for the eight directions of svt_cdef_find_dir_c (Common/Codec/EbCdef.c:132-196)."""
    I, J = np.mgrid[0:8, 0:8]
    return np.stack([I + J, I + J // 2, I, 3 + I - J // 2, 7 + I - J, 3 - I // 2 + J, J, I // 2 + J])


_DIV = [0, 840, 420, 280, 210, 168, 140, 120, 105]
_W_DIAG = [_DIV[i + 1] for i in range(7)] + [_DIV[8]] + [_DIV[7 - i] for i in range(7)]
_W_ODD = [420, 210, 140, 105, 105, 105, 105, 105, 140, 210, 420, 0, 0, 0, 0]
_W_AXIS = [105] * 8 + [0] * 7
CHART_WEIGHTS = np.array([_W_DIAG, _W_ODD, _W_AXIS, _W_ODD, _W_DIAG, _W_ODD, _W_AXIS, _W_ODD], np.int64)


def find_dir_costs(blocks, cs):
    """The eight direction costs of svt_cdef_find_dir_c stated with numpy: blocks [N][8][8] samples -> cost [N][8] (int64), direction [N]
    (first maximum) and var [N] = (best - cost[(best + 4) & 7]) >> 10.  A line sum weighs 840 / (samples on the line)."""
    x = (np.asarray(blocks, np.int64) >> cs) - 128
    n = x.shape[0]
    lines = chart_lines()
    cost = np.zeros((n, 8), np.int64)
    for d in range(8):
        onehot = (lines[d].reshape(64, 1) == np.arange(15)).astype(np.int64)
        partial = x.reshape(n, 64) @ onehot
        cost[:, d] = (partial * partial * CHART_WEIGHTS[d]).sum(axis=1)
    best = cost.argmax(axis=1)                       # first maximum; all zero -> 0, as `cost > best_cost` from best_cost = 0
    rows = np.arange(n)
    var = (cost[rows, best] - cost[rows, (best + 4) & 7]) >> 10
    return cost, best, var


def luma_blocks(plane):
    """[h/8][w/8][8][8] view of a luma plane's 8x8 blocks."""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)


def strength_i(var):
    """The `i` of adjust_strength (Common/Codec/EbCdef.c:112-116) for var != 0."""
    v = np.asarray(var, np.int64) >> 6
    return np.where(v > 0, np.minimum(np.floor(np.log2(np.maximum(v, 1))).astype(np.int64), 12), 0)


CHART_SEED, CHART_SIZES = 7, ((208, 144), (200, 136), (72, 72))   # the frames the GPU chart tests run on; test_cdef_chart_cpu.py checks what they cover
_AMPS = (1, 2, 4, 8, 16, 32, 64, 127)
# one cell of every kind (the per-call tests take exactly these) ...
CHART_KINDS = [("bin", d) for d in range(8)] + [("lvl", d) for d in range(8)] + [("tie", d) for d in (1, 2, 3)] + \
              [("flat", k) for k in range(3)] + [("chk", k) for k in range(2)] + [("imp", k) for k in range(2)]
# ... and the cycle a chart plane walks through: levels and ties twice (their amplitude is drawn per cell), two more flat cells, noise
CHART_CYCLE = CHART_KINDS + [("lvl", d) for d in range(8)] + [("tie", d) for d in (1, 2, 3)] + [("flat", 2), ("flat", 2), ("noise", 0)]


def chart_cell(kind, bd, rng):
    """One 8x8 cell (int64) of the direction chart.
      bin d   full-range binary stripes (0 / max), two lines wide, constant along direction d
      lvl d   random levels of amplitude {1 .. 127} << (bd - 8) around a random centre, constant along direction d
      tie d   A + A.T with A (random levels) constant along d = 1, 2, 3: the costs of d and 8 - d are equal, the lower index has to win
      flat k  0, max, a random level: the eight costs are equal -> direction 0, var 0
      chk k   checkerboard: full range, 1 LSB on a mid-grey
      imp k   one-sample impulse: max on 0, 0 on max
      noise   uniform noise"""
    name, k = kind
    cs, mx = bd - 8, (1 << bd) - 1
    lines = chart_lines()
    if name == "bin":
        return (((lines[k] + int(rng.integers(0, 4))) // 2) % 2) * mx
    if name == "lvl":
        amp = int(rng.choice(_AMPS))
        centre = int(rng.integers(amp << cs, mx - (amp << cs) + 1))
        return centre + (rng.integers(-amp, amp + 1, 15)[lines[k]] << cs)
    if name == "tie":
        amp = min(int(rng.choice(_AMPS)), 63)          # A around a quarter of the range: A + A.T around mid-grey, where the costs carry no DC term
        a = (64 << cs) + int(rng.integers(0, 1 << cs)) + (rng.integers(-amp, amp + 1, 15)[lines[k]] << cs)
        return a + a.T
    if name == "flat":
        return np.full((8, 8), (0, mx, int(rng.integers(1, mx)))[k], np.int64)
    I, J = np.mgrid[0:8, 0:8]
    if name == "chk":
        return ((I + J) % 2) * mx if k == 0 else (128 << cs) + ((I + J) % 2)
    if name == "imp":
        c = np.full((8, 8), mx if k else 0, np.int64)
        c[int(rng.integers(0, 8)), int(rng.integers(0, 8))] = 0 if k else mx
        return c
    return rng.integers(0, mx + 1, (8, 8))


def chart_kind_cells(bd):
    """One cell of every kind of CHART_KINDS, the same at every call: what the per-call tests place in their staging image."""
    rng = np.random.default_rng(760 + bd)   # (a draw at which every tie cell's maximum is the tied pair: test_cdef_chart_cpu.py)
    return [(kind, chart_cell(kind, bd, rng)) for kind in CHART_KINDS]


def _chart_plane(pw, ph, bd, rng, shift):
    """A plane of chart cells whose kind cycles with the cell index; `shift` = (dy, dx) moves the cell grid off the block grid.  The four
    picture corners are full-range checkerboards: 0 and max sit next to the CDEF_VERY_LARGE surround on every edge."""
    ncy, ncx = (ph + shift[0] + 7) // 8, (pw + shift[1] + 7) // 8
    grid = np.zeros((ncy * 8, ncx * 8), np.int64)
    for cy in range(ncy):
        for cx in range(ncx):
            grid[8 * cy:8 * cy + 8, 8 * cx:8 * cx + 8] = chart_cell(CHART_CYCLE[(cy * ncx + cx) % len(CHART_CYCLE)], bd, rng)
    p = grid[shift[0]:shift[0] + ph, shift[1]:shift[1] + pw].copy()
    chk = chart_cell(("chk", 0), bd, rng)
    for ys in (slice(0, 8), slice(ph - 8, ph)):
        for xs in (slice(0, 8), slice(pw - 8, pw)):
            p[ys, xs] = chk
    return p


def make_chart_frame(w, h, bd, seed, dtype=None):
    """(src, rec, skip8) like make_frame (4:2:0, dtype as there), rec a direction chart (see chart_cell).
    src = rec + noise of +-9 << (bd - 8), except: its first third by first third is max - rec (anti-correlated: the largest squared errors and
    a negative covariance in the luma metric), and rows [h/3, 2h/3) x columns [2w/3, w) equal rec (zero distortion).
    skip8 is random at 25 %, except: filter block (0, 1) is skipped entirely (pictures of >= 3 filter-block columns; in a narrower picture
    every filter block holds a corner), the bottom-left filter block keeps exactly one live block (the corner), the four corner blocks are live."""
    cs, mx = bd - 8, (1 << bd) - 1
    dt = dtype or (np.uint8 if bd == 8 else np.uint16)
    planes_src, planes_rec = [], []
    for pli in range(3):
        rng = np.random.default_rng([seed, pli])
        pw, ph = (w, h) if pli == 0 else (w // 2, h // 2)
        rec = _chart_plane(pw, ph, bd, rng, ((0, 0), (3, 5), (6, 2))[pli])
        src = np.clip(rec + (rng.integers(-9, 10, (ph, pw)) << cs), 0, mx)
        src[:ph // 3, :pw // 3] = mx - rec[:ph // 3, :pw // 3]
        src[ph // 3:2 * ph // 3, 2 * pw // 3:] = rec[ph // 3:2 * ph // 3, 2 * pw // 3:]
        planes_src.append(np.ascontiguousarray(src.astype(dt))); planes_rec.append(np.ascontiguousarray(rec.astype(dt)))
    rng = np.random.default_rng([seed, 3])
    r8, c8 = h // 8, w // 8
    skip8 = (rng.random((r8, c8)) < 0.25).astype(np.uint8)
    if (w + 63) // 64 >= 3:
        skip8[0:8, 8:16] = 1
    skip8[8 * ((r8 - 1) // 8):, 0:8] = 1
    skip8[0, 0] = skip8[0, c8 - 1] = skip8[r8 - 1, 0] = skip8[r8 - 1, c8 - 1] = 0
    return planes_src, planes_rec, skip8


def all_skip_fbs(skip8):
    """Raster indices of the filter blocks without a live block."""
    r8, c8 = skip8.shape
    nh = (c8 + 7) // 8
    return [fb for fb in range(((r8 + 7) // 8) * nh) if skip8[8 * (fb // nh):8 * (fb // nh) + 8, 8 * (fb % nh):8 * (fb % nh) + 8].all()]


# the frame-header strengths (pri * 4 + sec index) of the apply tests, one per filter block in turn: unfiltered, luma off / chroma on,
# chroma off / luma on, the maximum, secondary index 3 (= strength 4) without and with a primary, odd and even primaries
APPLY_STRENGTHS = [(0, 0), (0, 37), (22, 0), (63, 63), (3, 3), (7, 11), (60, 2), (13, 50), (1, 1), (33, 62), (18, 7), (47, 29)]


def chart_strengths(nfb, rot):
    ys = np.array([APPLY_STRENGTHS[(fb + rot) % len(APPLY_STRENGTHS)][0] for fb in range(nfb)], np.uint8)
    uvs = np.array([APPLY_STRENGTHS[(fb + rot) % len(APPLY_STRENGTHS)][1] for fb in range(nfb)], np.uint8)
    return ys, uvs


def orc_find_dir_frame(orc, luma, bd):
    """(dir, var) [h/8][w/8] of every 8x8 luma block by orc_cdef_find_dir."""
    blk = np.ascontiguousarray(luma_blocks(luma).astype(np.uint16))
    r8, c8 = blk.shape[:2]
    d = np.zeros((r8, c8), np.int32); v = np.zeros((r8, c8), np.int32)
    for by in range(r8):
        for bx in range(c8):
            var = C.c_int32(0)
            d[by, bx] = orc.orc_cdef_find_dir(ptr(blk[by, bx]), 8, C.byref(var), bd - 8)
            v[by, bx] = var.value
    return d, v


def orc_apply(orc, rec, bd, skip8, ys, uvs, damping):
    h, w = rec[0].shape
    P3 = C.c_void_p * 3; I3 = C.c_int * 3
    out = [p.copy() for p in rec]
    orc.orc_cdef_apply_frame(P3(*[p.ctypes.data for p in rec]), P3(*[p.ctypes.data for p in out]), I3(*[p.shape[1] for p in rec]),
                             rec[0].itemsize, w, h, ptr(skip8), ptr(ys), ptr(uvs), damping, bd)
    return out


def _fb_list(skip8, fbr, fbc, h, w):
    """The reference's list of live 8x8 blocks of one filter block (svt_sb_compute_cdef_list, EbEncCdef.c:239-290)."""
    nb_y, nb_x = min(8, h // 8 - 8 * fbr), min(8, w // 8 - 8 * fbc)
    dl = (CdefList * 64)(); count = 0
    for by in range(nb_y):
        for bx in range(nb_x):
            if not skip8[8 * fbr + by, 8 * fbc + bx]:
                dl[count] = CdefList(by, bx, 0); count += 1
    return dl, count, nb_y, nb_x


def _stage_fb(plane, dec, fbr, fbc, nvfb, nhfb, nb_y, nb_x):
    """The reference's 16-bit staging buffer of one filter block of one plane: 3 rows / 8 columns of neighbours, CDEF_VERY_LARGE outside the
    picture.  Returns (buffer, pointer to the filter block's first sample)."""
    p = plane.astype(np.uint16)
    inbuf = np.full(BSTRIDE * (128 + 2 * VB), VERY_LARGE, np.uint16)
    yoff, xoff = VB * (fbr != 0), HB * (fbc != 0)
    ysize = ((nb_y * 8) >> dec) + VB * (fbr + 1 < nvfb) + yoff
    xsize = ((nb_x * 8) >> dec) + HB * (fbc + 1 < nhfb) + xoff
    y0, x0 = ((64 * fbr) >> dec) - yoff, ((64 * fbc) >> dec) - xoff
    view = inbuf.reshape(-1, BSTRIDE)
    view[VB - yoff:VB - yoff + ysize, HB - xoff:HB - xoff + xsize] = p[y0:y0 + ysize, x0:x0 + xsize]
    return inbuf, C.c_void_p(inbuf.ctypes.data + 2 * (VB * BSTRIDE + HB))


def ref_search_fb(ref, rec, src, bd, skip8, fbr, fbc, pri_damping, ngi=64):
    """mse[2][64] of one filter block via the reference's own functions."""
    cs = bd - 8
    h, w = rec[0].shape
    nvfb, nhfb = (h + 63) // 64, (w + 63) // 64
    dl, count, nb_y, nb_x = _fb_list(skip8, fbr, fbc, h, w)
    mse = np.zeros((2, 64), np.uint64)
    if count == 0:
        return None
    dirs = ((C.c_int32 * 16) * 16)(); var = ((C.c_int32 * 16) * 16)(); dirinit = C.c_int32(0)
    for pli in range(3):
        dec = 1 if pli else 0
        inbuf, in_ptr = _stage_fb(rec[pli], dec, fbr, fbc, nvfb, nhfb, nb_y, nb_x)
        bsize = 0 if dec else 3  # BLOCK_4X4 / BLOCK_8X8
        s = src[pli]
        sp = C.c_void_p(s.ctypes.data + s.itemsize * (((64 * fbr) >> dec) * s.shape[1] + ((64 * fbc) >> dec)))
        for gi in range(ngi):
            pri, sec = gi // 4, gi % 4
            if rec[pli].dtype == np.uint8:      # 16-bit planes take the 16-bit output and distortion functions at any depth (coeff_shift = bd - 8)
                tmp = np.zeros(1 << 14, np.uint8)
                ref.svt_cdef_filter_fb(ptr(tmp), None, BSTRIDE, in_ptr, dec, dec, dirs, C.byref(dirinit), var, pli, dl, count,
                                       pri, sec + (sec == 3), pri_damping, pri_damping, cs)
                f = ref.compute_cdef_dist_8bit_c; f.restype = C.c_uint64
                d = f(sp, s.shape[1], ptr(tmp), dl, count, bsize, cs, pli)
            else:
                tmp = np.zeros(1 << 14, np.uint16)
                ref.svt_cdef_filter_fb(None, ptr(tmp), BSTRIDE, in_ptr, dec, dec, dirs, C.byref(dirinit), var, pli, dl, count,
                                       pri, sec + (sec == 3), pri_damping, pri_damping, cs)
                f = ref.compute_cdef_dist_c; f.restype = C.c_uint64
                d = f(sp, s.shape[1], ptr(tmp), dl, count, bsize, cs, pli)
            mse[0 if pli == 0 else 1, gi] += np.uint64(d)
    return mse


def ref_apply_fb(ref, rec, out, bd, skip8, fbr, fbc, y_strength, uv_strength, damping):
    """One filter block of svt_av1_cdef_frame (EbEncCdef.c:292-661) via svt_cdef_filter_fb with dirinit = NULL: written in plane layout with the
    plane's stride into out[] (which starts as a copy of rec[]); planes go 0, 1, 2 and share dir / var; a filter block whose four strengths are
    zero, or without a live block, is left alone (:434-441)."""
    cs = bd - 8
    h, w = rec[0].shape
    nvfb, nhfb = (h + 63) // 64, (w + 63) // 64
    dl, count, nb_y, nb_x = _fb_list(skip8, fbr, fbc, h, w)
    lv = (y_strength // 4, uv_strength // 4); sc = [y_strength % 4, uv_strength % 4]
    sc = [s + (s == 3) for s in sc]
    if count == 0 or (lv[0] == 0 and sc[0] == 0 and lv[1] == 0 and sc[1] == 0):
        return
    dirs = ((C.c_int32 * 16) * 16)(); var = ((C.c_int32 * 16) * 16)()
    for pli in range(3):
        dec = 1 if pli else 0
        inbuf, in_ptr = _stage_fb(rec[pli], dec, fbr, fbc, nvfb, nhfb, nb_y, nb_x)
        o = out[pli]
        dst = C.c_void_p(o.ctypes.data + o.itemsize * (((64 * fbr) >> dec) * o.shape[1] + ((64 * fbc) >> dec)))
        lbd = o.dtype == np.uint8
        ref.svt_cdef_filter_fb(dst if lbd else None, None if lbd else dst, o.shape[1], in_ptr, dec, dec, dirs, None, var, pli, dl, count,
                               lv[pli != 0], sc[pli != 0], damping, damping, cs)


def orc_search(orc, rec, src, bd, skip8, pri_damping, pick=0, fb_begin=0, fb_end=None):
    h, w = rec[0].shape
    nfb = ((h + 63) // 64) * ((w + 63) // 64)
    fb_end = nfb if fb_end is None else fb_end
    mse = np.zeros((2, nfb, 64), np.uint64)
    P3 = C.c_void_p * 3; I3 = C.c_int * 3
    orc.orc_cdef_search_frame(P3(*[r.ctypes.data for r in rec]), I3(*[r.shape[1] for r in rec]), P3(*[s.ctypes.data for s in src]),
                              I3(*[s.shape[1] for s in src]), rec[0].itemsize, w, h, ptr(skip8), pri_damping, bd, pick, ptr(mse),
                              fb_begin, fb_end)
    return mse
