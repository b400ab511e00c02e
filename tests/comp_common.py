"""Shared definitions for the compound-prediction, OBMC, blend and warp tests: the block records of the C ABI, the random block lists of the first tests, and
(second half) deterministic lists over the full cross products with a numpy restatement and closed forms per operation."""
import ctypes as C

import numpy as np

from conftest import load_package

_pkg = load_package()
CompBlk, WarpBlk, WarpCompBlk, BlendBlk, ObmcBlk = _pkg.CompBlk, _pkg.WarpBlk, _pkg.WarpCompBlk, _pkg.BlendBlk, _pkg.ObmcBlk   # the block records of the C ABI
assert C.sizeof(CompBlk) == 48
SIZES = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (4, 8), (8, 4), (16, 8), (8, 16), (32, 16), (16, 32), (64, 32), (32, 64), (128, 64), (64, 128), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]
# quant_dist_lookup_table[order_idx][..] pairs the encoder uses for COMPOUND_DISTANCE (fwd + bck = 16)
DIST_PAIRS = [(9, 7), (11, 5), (12, 4), (13, 3), (7, 9), (5, 11), (4, 12), (3, 13)]


def make_blocks(rng, W, H, n, mask_bytes):
    """n random compound blocks tiling nothing in particular: destinations are disjoint cells of a 128-pixel grid.  Returns (array, mask buffer)."""
    cols = W // 128
    assert n <= cols * (H // 128)
    blks = (CompBlk * n)()
    masks = rng.integers(0, 65, mask_bytes).astype(np.uint8)
    off = 0
    for i in range(n):
        w, h = SIZES[i % len(SIZES)]
        cx, cy = (i % cols) * 128, (i // cols) * 128
        b = blks[i]
        b.dst_x, b.dst_y, b.w, b.h = cx, cy, w, h
        b.src0_x, b.src0_y = cx + int(rng.integers(-6, 7)), cy + int(rng.integers(-6, 7))
        b.src1_x, b.src1_y = cx + int(rng.integers(-6, 7)), cy + int(rng.integers(-6, 7))
        b.bank_x = b.bank_y = int(rng.integers(0, 4)) if w > 4 and h > 4 else int(rng.integers(4, 6))
        if i % 7 == 3: b.bank_y = int(rng.integers(0, 3))          # dual filters
        sp = [int(rng.integers(0, 16)) for _ in range(4)]
        if i % 5 == 0: sp[0] = 0
        if i % 5 == 1: sp[1] = 0
        if i % 11 == 2: sp = [0, 0, sp[2], 0]
        b.subpel0_x, b.subpel0_y, b.subpel1_x, b.subpel1_y = sp
        b.type = i % 4
        b.fwd_offset, b.bck_offset = DIST_PAIRS[i % len(DIST_PAIRS)]
        b.mask_type = (i // 4) & 1
        b.mask_sub = 0
        b.mask_off, b.mask_stride = -1, 0
        if b.type == 2 and i % 8 != 2:
            b.mask_off = off; off += w * h
        if b.type == 3:
            b.mask_sub = (i // 4) % 2 if max(w, h) <= 64 else 0
            ms = (2 * w if b.mask_sub else w) + int(rng.integers(0, 9))
            b.mask_off, b.mask_stride = off, ms
            off += ms * (2 * h if b.mask_sub else h)
        assert off <= mask_bytes
    return blks, masks


# ---------------------------------------------------------------- warped prediction
assert C.sizeof(WarpBlk) == 44
WARP_SIZES = [(8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (8, 16), (16, 8), (32, 16), (16, 32), (64, 32), (32, 64), (128, 64), (64, 128), (8, 32), (32, 8), (16, 64), (64, 16)]


def warp_model(rng, extreme=False):
    """A model in the style of /root/reference/test/warp_filter_test_util.cc:47-110: random matrix around identity, shear parameters rounded to
    multiples of 64 and inside is_affine_shear_allowed's bounds (4|a| + 7|b| < 2^16, 4|g| + 4|d| < 2^16)."""
    while True:
        lim = (1 << 13) - 64 if not extreme else 1 << 13
        a, b, g, d = [int(rng.integers(-lim, lim + 1)) // 64 * 64 for _ in range(4)]
        if extreme: a, b, g, d = [int(v) for v in rng.choice([-8192, 8192, -4096, 0, 4032], 4)]
        if 4 * abs(a) + 7 * abs(b) >= (1 << 16) or 4 * abs(g) + 4 * abs(d) >= (1 << 16): continue
        m2 = (1 << 16) + a; m3 = b
        m4 = (g * m2) >> 16
        m5 = (1 << 16) + d + (m3 * m4) // m2
        m0, m1 = int(rng.integers(-(1 << 21), 1 << 21)), int(rng.integers(-(1 << 21), 1 << 21))
        return [m0, m1, m2, m3, m4, m5], a, b, g, d


def warp_blocks(rng, W, H, n):
    cols = W // 128
    assert n <= cols * (H // 128)
    blks = (WarpBlk * n)()
    for i in range(n):
        mat, a, b, g, d = warp_model(rng, extreme=(i % 9 == 4))
        if i % 7 == 0: mat[0] += 500 << 16        # far outside the plane: every sample clamps to the right edge
        if i % 7 == 1: mat[1] -= 400 << 16        # ... to the top edge
        w, h = WARP_SIZES[i % len(WARP_SIZES)]
        bl = blks[i]
        for k in range(6): bl.mat[k] = mat[k]
        bl.alpha, bl.beta, bl.gamma, bl.delta = a, b, g, d
        bl.p_col, bl.p_row, bl.p_width, bl.p_height = (i % cols) * 128, (i // cols) * 128, w, h
    return blks


# ---------------------------------------------------------------- pixel-domain mask blends
assert C.sizeof(BlendBlk) == 40
BLEND_SIZES = [(1, 1), (2, 2), (4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (2, 8), (8, 2), (4, 16), (16, 4), (64, 8), (8, 64), (128, 32), (32, 128), (1, 16), (16, 1)]


def blend_blocks(rng, W, H, n, mask_bytes):
    cols = W // 128
    assert n <= cols * (H // 128)
    blks = (BlendBlk * n)()
    masks = rng.integers(0, 65, mask_bytes).astype(np.uint8)
    masks[:300] = 64; masks[300:600] = 0
    off = 0
    for i in range(n):
        w, h = BLEND_SIZES[i % len(BLEND_SIZES)]
        b = blks[i]
        cx, cy = (i % cols) * 128, (i // cols) * 128
        b.dst_x, b.dst_y, b.w, b.h = cx, cy, w, h
        b.src0_x, b.src0_y = (cx, cy) if i % 4 == 0 else (int(rng.integers(0, W - 128)), int(rng.integers(0, H - 128)))    # i % 4 == 0: in place (dst == src0)
        b.src1_x, b.src1_y = int(rng.integers(0, W - 128)), int(rng.integers(0, H - 128))
        b.mode = i % 3
        b.subw, b.subh = ((i // 3) & 1, (i // 6) & 1) if b.mode == 0 and max(w, h) <= 64 else (0, 0)
        if b.mode == 0:
            b.mask_stride = (w << b.subw) + int(rng.integers(0, 5))
            need = b.mask_stride * (h << b.subh)
        else:
            b.mask_stride, need = 0, (w if b.mode == 1 else h)
        b.mask_off = off; off += need
        assert off <= mask_bytes
    return blks, masks


# ================================================================ deterministic case lists, numpy restatements and closed forms
# The lists below are built with nested loops over the cross products the kernels can tell apart; whatever is not part of a product cycles on a counter whose
# period is coprime to the product's sizes (or drifts by one per group), so no two properties move in step.  Every builder returns the records and, per record,
# a plain description that tests/test_comp_ref_cpu.py counts.  Built once per format and shared: nothing here is written to after it is returned.
import functools
import os
import re
from types import SimpleNamespace as NS

FLAVOURS = ("copy", "x", "y", "2d")          # per reference: (subpel_x != 0) + 2 * (subpel_y != 0)
CONTENTS = ("random", "max_on_0", "0_on_max", "checker", "binary")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vp(a): return a.ctypes.data_as(C.c_void_p)


def dtype_of(bd, dt=None): return dt if dt is not None else (np.uint8 if bd == 8 else np.uint16)


def interp_taps(orc):
    """the six 16 x 8 interpolation banks (tests/test_oracle_vs_ref.py pins them to the reference's tables)"""
    return np.ctypeslib.as_array((C.c_int16 * 8 * 16 * 6).in_dll(orc, "orc_interp_kernels")).astype(np.int64)


def zero_outer_taps(taps):
    """the deliberately wrong banks of the sensitivity test: taps 0 and 7 dropped"""
    t = taps.copy(); t[:, :, 0] = 0; t[:, :, 7] = 0
    return t


@functools.lru_cache(maxsize=None)
def warped_filters():
    """Warped_Filters [193][8] from the oracle's generated header (pinned to the reference's table by test_warp_filter_table_headers)"""
    txt = open(os.path.join(ROOT, "oracle", "warp_filter_table.h")).read()
    v = [int(x) for x in re.findall(r"-?\d+", txt[txt.index("#define SVT_WARPED_FILTER_TABLE"):])]
    return np.array(v, np.int64).reshape(193, 8)


def rp2(v, n):
    """ROUND_POWER_OF_TWO on int64 arrays or ints"""
    return v if n == 0 else (v + (1 << (n - 1))) >> n


class Shelf:
    """packs rectangles left to right, top to bottom, touching: the tight, disjoint destinations of a list"""
    def __init__(self, width, x0=0, y0=0): self.W, self.x0, self.x, self.y, self.hh = width, x0, x0, y0, 0

    def put(self, w, h):
        if self.x + w > self.W: self.x, self.y, self.hh = self.x0, self.y + self.hh, 0
        x, y = self.x, self.y
        self.x += w; self.hh = max(self.hh, h)
        return x, y

    @property
    def height(self): return self.y + self.hh


def pattern(shape, dt, lo=1, span=251):
    """the non-zero pre-fill of everything a kernel writes: lo + (7 x + 13 y) % span (a stray store of any constant shows)"""
    if len(shape) == 1: return (lo + (np.arange(shape[0]) * 7) % span).astype(dt)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return (lo + (7 * xx + 13 * yy) % span).astype(dt)


def cover(shape, rects):
    m = np.zeros(shape, bool)
    for x, y, w, h in rects: m[y:y + h, x:x + w] = True
    return m


def content_regions(bd, dt, rng, region, cols, rows, second):
    """a plane of cols x rows square regions, region k holding CONTENTS[k % 5]; second = the plane of reference 1 (max_on_0 / 0_on_max swap sides)"""
    mx = (1 << bd) - 1
    p = rng.integers(0, mx + 1, (rows * region, cols * region)).astype(dt)
    yy, xx = np.mgrid[0:region, 0:region]
    for k in range(cols * rows):
        v = p[(k // cols) * region:(k // cols + 1) * region, (k % cols) * region:(k % cols + 1) * region]
        kind = CONTENTS[k % 5]
        if kind == "max_on_0": v[:] = 0 if second else mx
        elif kind == "0_on_max": v[:] = mx if second else 0
        elif kind == "checker": v[:] = ((yy + xx + second) & 1) * mx
        elif kind == "binary": v[:] = rng.integers(0, 2, (region, region)) * mx
    return p


# ---------------------------------------------------------------- compound prediction
REGION = 160                                   # a 128 x 128 block's 135 x 135 footprint fits with 26 positions to spare


def footprint(x, y, w, h):
    """what compound_predict_kernel reads for a block at (x, y): 23 x 23 per 16 x 16 tile whatever the block's width -> (x0, y0, x1, y1), inclusive"""
    return x - 3, y - 3, x + 16 * ((w + 15) // 16) + 3, y + 16 * ((h + 15) // 16) + 3


@functools.lru_cache(maxsize=None)
def compound_cases(bd, dt=None):
    """22 sizes x 4 types x 16 (flavour of reference 0, flavour of reference 1) = 1408 blocks -> NS(blks, desc, ref0, ref1, masks, dst_w, dst_h)"""
    dt = dtype_of(bd, dt)
    rng = np.random.default_rng(4100 + bd)
    ref0 = content_regions(bd, dt, rng, REGION, 3, 2, 0); ref1 = content_regions(bd, dt, rng, REGION, 3, 2, 1)
    n = len(SIZES) * 4 * 16
    blks = (CompBlk * n)(); desc = []
    shelf = Shelf(1024)
    c = cx = cy = k1 = k2 = k3 = moff = 0
    for si, (w, h) in enumerate(SIZES):
        for typ in range(4):
            for f0 in range(4):
                for f1 in range(4):
                    b = blks[c]
                    b.w, b.h, b.type = w, h, typ
                    b.dst_x, b.dst_y = shelf.put(w, h)
                    content = c % 5                                                    # period 5 against 16 per (size, type): every content, every (size, type)
                    rx, ry = (content % 3) * REGION, (content // 3) * REGION
                    fw, fh = 16 * ((w + 15) // 16) + 7, 16 * ((h + 15) // 16) + 7
                    b.src0_x, b.src0_y = rx + 3 + (3 * c) % (REGION - fw + 1), ry + 3 + (7 * c) % (REGION - fh + 1)
                    b.src1_x, b.src1_y = rx + 3 + (5 * c + 1) % (REGION - fw + 1), ry + 3 + (11 * c + 2) % (REGION - fh + 1)
                    b.bank_x = b.bank_y = (c + c // 16) % 6                            # drifts by one per (size, type) group: no parity shared with the flavours
                    if c % 7 == 3: b.bank_y = (b.bank_x + 1 + (c // 7) % 5) % 6        # dual filters
                    sp = [0, 0, 0, 0]
                    for r, f in enumerate((f0, f1)):
                        if f & 1: sp[2 * r] = 1 + (7 * cx + cx // 15) % 15; cx += 1
                        if f & 2: sp[2 * r + 1] = 1 + (4 * cy + cy // 15) % 15; cy += 1
                    b.subpel0_x, b.subpel0_y, b.subpel1_x, b.subpel1_y = sp
                    b.fwd_offset, b.bck_offset = DIST_PAIRS[(3 * k1 + k1 // 16) % 8]
                    b.mask_off, b.mask_stride = -1, 0
                    if typ == 1: k1 += 1
                    if typ == 2:
                        b.mask_type = (k2 + k2 // 16) & 1
                        if 4 * f0 + f1 != (5 * si) % 16:                               # once per size: no mask stored
                            moff += (1, 2, 3, 0, 5)[k2 % 5]
                            b.mask_off = moff; moff += w * h
                        k2 += 1
                    if typ == 3:
                        b.mask_sub = (k3 + k3 // 16) & 1 if max(w, h) <= 64 else 0
                        moff += (1, 2, 3, 0, 5)[k3 % 5]
                        b.mask_stride = (w << b.mask_sub) + (0, 5, 0, 9, 16)[(k3 + k3 // 5) % 5]
                        b.mask_off = moff; moff += b.mask_stride * (h << b.mask_sub)
                        k3 += 1
                    desc.append(dict(size=(w, h), type=typ, f0=f0, f1=f1, content=CONTENTS[content], banks=(int(b.bank_x), int(b.bank_y)), subpel=tuple(sp),
                                     dist=(int(b.fwd_offset), int(b.bck_offset)), mask_type=int(b.mask_type), mask_sub=int(b.mask_sub), mask_off=int(b.mask_off),
                                     mask_stride=int(b.mask_stride)))
                    c += 1
    masks = np.random.default_rng(4200).integers(0, 65, moff + 8).astype(np.uint8)
    return NS(blks=blks, desc=desc, ref0=ref0, ref1=ref1, masks=masks, dst_w=1024, dst_h=shelf.height, bd=bd, dt=dt, n=n)


def mask_pattern(masks, blks):
    """the mask buffer a launch starts from: the supplied masks where a type-3 record reads them, a pattern above 64 (no mask value) everywhere else"""
    m = (65 + (np.arange(masks.size) * 7) % 190).astype(np.uint8)
    for b in blks:
        if b.type == 3:
            e = b.mask_off + b.mask_stride * (b.h << b.mask_sub)
            m[b.mask_off:e] = masks[b.mask_off:e]
    return m


def numpy_d16(plane, x, y, w, h, taps, bank_x, bank_y, sx, sy, bd):
    """the 16-bit compound intermediate of one reference: copy, one 8-tap pass, or two with the 16-bit value in between"""
    r0, r1 = (5 if bd == 12 else 3), 7
    ob = bd + 14 - r0
    ro = (1 << (ob - r1)) + (1 << (ob - r1 - 1))
    P = plane.astype(np.int64)
    if not sx and not sy: return (P[y:y + h, x:x + w] << (14 - r1 - r0)) + ro
    xf, yf = taps[bank_x][sx], taps[bank_y][sy]
    if not sy: return rp2(sum(int(xf[k]) * P[y:y + h, x - 3 + k:x - 3 + k + w] for k in range(8)), r0) * (1 << (7 - r1)) + ro
    if not sx: return rp2(sum(int(yf[k]) * P[y - 3 + k:y - 3 + k + h, x:x + w] for k in range(8)) * (1 << (7 - r0)), r1) + ro
    im = rp2((1 << (bd + 6)) + sum(int(xf[k]) * P[y - 3:y + h + 4, x - 3 + k:x - 3 + k + w] for k in range(8)), r0)
    im = ((im + (1 << 15)) & 0xffff) - (1 << 15)                                       # kept as int16
    return rp2((1 << ob) + sum(int(yf[k]) * im[k:k + h] for k in range(8)), r1) & 0xffff


def numpy_compound_block(b, ref0, ref1, masks, bd, taps, same_flavour=False, wrong_type=False):
    """-> (samples [h][w], the DIFFWTD mask or None).  same_flavour / wrong_type: the wrong variants of the sensitivity tests (reference 1 filtered with
    reference 0's phases; a type handled as its neighbour of the other parity)"""
    w, h = b.w, b.h
    r0, r1 = (5 if bd == 12 else 3), 7
    ob, bits = bd + 14 - r0, 14 - r0 - r1
    ro = (1 << (ob - r1)) + (1 << (ob - r1 - 1))
    s1 = (b.subpel0_x, b.subpel0_y) if same_flavour else (b.subpel1_x, b.subpel1_y)
    d0 = numpy_d16(ref0, b.src0_x, b.src0_y, w, h, taps, b.bank_x, b.bank_y, b.subpel0_x, b.subpel0_y, bd)
    d1 = numpy_d16(ref1, b.src1_x, b.src1_y, w, h, taps, b.bank_x, b.bank_y, s1[0], s1[1], bd)
    typ, seg = (b.type ^ 1 if wrong_type else b.type), None
    if typ == 0: t = (d0 + d1) >> 1
    elif typ == 1: t = (d0 * b.fwd_offset + d1 * b.bck_offset) >> 4
    else:
        if typ == 2:
            m = np.minimum(38 + (rp2(np.abs(d0 - d1), bits + bd - 8) >> 4), 64)
            if b.mask_type: m = 64 - m
            seg = m.astype(np.uint8)
        else:
            sub, off, ms = (int(b.mask_sub), b.mask_off, b.mask_stride) if b.type == 3 else (0, max(b.mask_off, 0), w)      # else: only under wrong_type
            M = masks[off:off + ms * (h << sub)].astype(np.int64).reshape(h << sub, ms)
            m = rp2(M[0:2 * h:2, 0:2 * w:2] + M[1:2 * h:2, 0:2 * w:2] + M[0:2 * h:2, 1:2 * w:2] + M[1:2 * h:2, 1:2 * w:2], 2) if sub else M[:h, :w]
        t = (m * d0 + (64 - m) * d1) >> 6
    return np.clip(rp2(t - ro, bits), 0, (1 << bd) - 1), seg


# all max against all 0 (reference 0 holds the max), every flavour pair: the filters sum to 128, so every flavour gives max << (7 - round_0) exactly
CLOSED_COMPOUND = {"average": {8: 128, 10: 512, 12: 2048}, "distance_13_3": {8: 207, 10: 831, 12: 3327},
                   "diffwtd_38_mask": {8: 53, 10: 54, 12: 54}, "diffwtd_38_sample": {8: 211, 10: 863, 12: 3455}}


def closed_compound(d, bd):
    """(sample, mask or None) a record of saturated content must give, from three lines of arithmetic on flat planes; None where there is no closed form"""
    if d["content"] not in ("max_on_0", "0_on_max") or d["type"] == 3: return None
    bits = 14 - 7 - (5 if bd == 12 else 3)
    a, b = (((1 << bd) - 1) << bits, 0) if d["content"] == "max_on_0" else (0, ((1 << bd) - 1) << bits)
    if d["type"] == 0: return rp2((a + b) >> 1, bits), None
    if d["type"] == 1: return rp2((a * d["dist"][0] + b * d["dist"][1]) >> 4, bits), None
    m = min(38 + (rp2(abs(a - b), bits + bd - 8) >> 4), 64)
    if d["mask_type"]: m = 64 - m
    return rp2((m * a + (64 - m) * b) >> 6, bits), m


@functools.lru_cache(maxsize=None)
def compound_expected(orc, bd, dt=None):
    """the oracle's destination plane and mask buffer for compound_cases(bd, dt), from the pre-fill patterns -> (dst0, masks0, exp, m_exp)"""
    c = compound_cases(bd, dt)
    dst0, m0 = pattern((c.dst_h, c.dst_w), c.dt), mask_pattern(c.masks, c.blks)
    exp, m_exp = dst0.copy(), m0.copy()
    orc.orc_compound_predict_batch(c.ref0.itemsize, bd, _vp(c.ref0), c.ref0.shape[1], _vp(c.ref1), c.ref1.shape[1], _vp(exp), c.dst_w, _vp(m_exp), c.blks, 0, c.n)
    return dst0, m0, exp, m_exp


# ---------------------------------------------------------------- pixel-domain blends
MASK_CLASSES = ("random", "all_64", "all_0")


@functools.lru_cache(maxsize=None)
def blend_cases(in_place):
    """18 sizes x {mode 0 with each (subw, subh) up to 64 x 64, with (0, 0) above; mode 1; mode 2} x three masks.  in_place: dst is src0's plane at src0's
    position; otherwise a plane of its own (so every source is disjoint from every destination) -> NS(blks, desc, masks, w, h): all three planes are w x h"""
    combos = lambda w, h: [(0, sw, sh) for sw in (0, 1) for sh in (0, 1) if (sw, sh) == (0, 0) or max(w, h) <= 64] + [(1, 0, 0), (2, 0, 0)]
    n = sum(len(combos(w, h)) for w, h in BLEND_SIZES) * 3
    blks = (BlendBlk * n)(); desc = []
    W = 512
    shelf = Shelf(W, 3, 2)
    rng = np.random.default_rng(4300)
    mparts = []; moff = c = 0
    for (w, h) in BLEND_SIZES:
        for (mode, sw, sh) in combos(w, h):
            for mc, mclass in enumerate(MASK_CLASSES):
                b = blks[c]
                b.w, b.h, b.mode, b.subw, b.subh = w, h, mode, sw, sh
                b.dst_x, b.dst_y = shelf.put(w, h)
                b.mask_stride = (w << sw) + (0, 3, 0, 7, 1)[c % 5] if mode == 0 else 0
                need = b.mask_stride * (h << sh) if mode == 0 else (w if mode == 1 else h)
                pad = (1, 0, 3, 2, 5)[(c + c // 5) % 5]
                mparts.append(rng.integers(0, 65, pad).astype(np.uint8))
                mparts.append(rng.integers(0, 65, need).astype(np.uint8) if mclass == "random" else np.full(need, 64 if mclass == "all_64" else 0, np.uint8))
                b.mask_off = moff + pad; moff += pad + need
                desc.append(dict(size=(w, h), mode=mode, sub=(sw, sh), mask=mclass))
                c += 1
    H = shelf.height + 2
    for c, b in enumerate(blks):
        b.src0_x, b.src0_y = (b.dst_x, b.dst_y) if in_place else ((11 * c) % (W - b.w + 1), (5 * c) % (H - b.h + 1))
        b.src1_x, b.src1_y = (7 * c + 1) % (W - b.w + 1), (3 * c + 2) % (H - b.h + 1)
    return NS(blks=blks, desc=desc, masks=np.concatenate(mparts), w=W, h=H, n=n, in_place=in_place)


def blend_planes(c, dt):
    """(src0, src1, dst pre-fill) of a blend list: samples up to 255 / 4095, both ends planted; in place the destination is src0 itself"""
    rng = np.random.default_rng(4400 + np.dtype(dt).itemsize)
    mx = 255 if dt == np.uint8 else 4095
    a = rng.integers(0, mx + 1, (c.h, c.w)).astype(dt); b = rng.integers(0, mx + 1, (c.h, c.w)).astype(dt)
    a[::7, ::5] = mx; b[::5, ::7] = mx; a[3::7, 1::5] = 0; b[2::5, 3::7] = 0
    return a, b, (a.copy() if c.in_place else pattern((c.h, c.w), dt))


def numpy_blend_block(b, s0, s1, masks, ignore_subh=False):
    """s0 / s1: the block's two h x w sources"""
    w, h, sw, sh = b.w, b.h, int(b.subw), int(b.subh)
    M = masks[b.mask_off:].astype(np.int64)
    if b.mode == 1: m = M[:w][None, :]
    elif b.mode == 2: m = M[:h][:, None]
    else:
        if ignore_subh: sh = 0
        M = M[:b.mask_stride * (h << sh)].reshape(h << sh, b.mask_stride)
        cols = (M[:, 0:2 * w:2] + M[:, 1:2 * w:2]) if sw else M[:, :w]
        m = rp2(cols[0::2] + cols[1::2], sw + 1) if sh else rp2(cols, sw)
    return rp2(m * s0.astype(np.int64) + (64 - m) * s1.astype(np.int64), 6)


# ---------------------------------------------------------------- OBMC costs
assert C.sizeof(ObmcBlk) == 16
OBMC_CONTENTS = ("random", "pre_max", "pre_0", "halves")
OBMC_OFFSETS = ((0, 0), (1, 0), (0, 1), (1, 1))


@functools.lru_cache(maxsize=None)
def obmc_cases():
    """22 sizes x the four offset classes x four contents, each content in the block's own (w + 1) x (h + 1) predictor rectangle and wm_off range
    -> NS(blks, desc, pre, wsrc, mask)"""
    n = len(SIZES) * 16
    blks = (ObmcBlk * n)(); desc = []
    W = 1024
    shelf = Shelf(W, 1, 1)
    for (w, h) in SIZES:
        for _ in range(16): shelf.put(w + 1, h + 1)
    rng = np.random.default_rng(4500)
    pre = rng.integers(0, 256, (shelf.height + 1, W)).astype(np.uint8)
    total = sum(w * h for w, h in SIZES) * 16
    wsrc = rng.integers(0, 255 * 4096 + 1, total).astype(np.int32); mask = rng.integers(0, 4097, total).astype(np.int32)
    shelf = Shelf(W, 1, 1)
    c = off = ex = ey = 0
    for (w, h) in SIZES:
        for (ox, oy) in OBMC_OFFSETS:
            for content in OBMC_CONTENTS:
                x, y = shelf.put(w + 1, h + 1)
                xo = yo = 0
                if ox: xo = 1 + ex % 7; ex += 1
                if oy: yo = 1 + (3 * ey) % 7; ey += 1
                blks[c] = ObmcBlk(x, y, w, h, xo, yo, off)
                P = pre[y:y + h + 1, x:x + w + 1]; Ws = wsrc[off:off + w * h].reshape(h, w); Mk = mask[off:off + w * h].reshape(h, w)
                if content == "pre_max": P[:] = 255; Ws[:] = 0; Mk[:] = 4096
                elif content == "pre_0": P[:] = 0; Ws[:] = 255 * 4096
                elif content == "halves":
                    P[:, :w // 2] = 255; Ws[:, :w // 2] = 0; P[:, w // 2:] = 0; Ws[:, w // 2:] = 255 * 4096; Mk[:] = 4096
                desc.append(dict(size=(w, h), offsets=(ox, oy), eighths=(xo, yo), content=content))
                off += w * h; c += 1
    return NS(blks=blks, desc=desc, pre=pre, wsrc=wsrc, mask=mask, n=n)


def numpy_obmc_block(b, pre, wsrc, mask, narrow_square=False):
    """{sad, sse, variance} of one block; narrow_square: the wrong variant whose sum * sum is a 32-bit product"""
    w, h = b.w, b.h
    P = pre[b.pre_y:b.pre_y + h + 1, b.pre_x:b.pre_x + w + 1].astype(np.int64)
    Ws = wsrc[b.wm_off:b.wm_off + w * h].astype(np.int64).reshape(h, w); Mk = mask[b.wm_off:b.wm_off + w * h].astype(np.int64).reshape(h, w)
    sad = int(rp2(np.abs(Ws - P[:h, :w] * Mk), 12).sum())
    f1 = rp2(P[:, :w] * (128 - 16 * b.xoffset) + P[:, 1:] * (16 * b.xoffset), 7)
    pf = rp2(f1[:h] * (128 - 16 * b.yoffset) + f1[1:] * (16 * b.yoffset), 7) & 0xff
    v = Ws - pf * Mk
    d = np.sign(v) * rp2(np.abs(v), 12)
    sm, sse = int(d.sum()), int((d * d).sum())
    sq = sm * sm
    if narrow_square: sq = ((sq + (1 << 31)) % (1 << 32)) - (1 << 31)
    q = abs(sq) // (w * h) * (1 if sq >= 0 else -1)                                    # C division truncates towards 0
    return sad % (1 << 32), sse % (1 << 32), (sse - q) % (1 << 32)


def closed_obmc(d):
    """(sad, sse, variance) where the content fixes them: predictor 255 on wsrc 0 under the full mask at any offsets (a flat plane filters to itself), and the
    half-and-half block at offset (0, 0), whose differences are +255 and -255 in equal number"""
    w, h = d["size"]
    if d["content"] == "pre_max": return 255 * w * h, 65025 * w * h, 0
    if d["content"] == "halves" and d["offsets"] == (0, 0): return 255 * w * h, 65025 * w * h, 65025 * w * h
    return None


@functools.lru_cache(maxsize=None)
def obmc_expected(orc):
    c = obmc_cases()
    exp = np.zeros((c.n, 3), np.uint32)
    orc.orc_obmc_batch(_vp(c.pre), c.pre.shape[1], _vp(c.wsrc), _vp(c.mask), c.blks, c.n, _vp(exp))
    return exp


# ---------------------------------------------------------------- warped prediction
# the reference's functions take any p_width / p_height: the last cell of a row or column is cut by AOMMIN(4, p_col + p_width - j - 4), which is how a 4-wide
# chroma block of an 8 x 8 luma block is predicted; and any plane from 1 x 1 up, since every row and column index is clamped
WARP_ALL_SIZES = WARP_SIZES + [(4, 4), (4, 8), (8, 4), (4, 16)]
WARP_SS = ((0, 0), (1, 1), (1, 0))
WARP_CLASSES = ("random", "extreme", "left", "right", "above", "below", "astride_left", "astride_right", "astride_top", "astride_bottom", "corner")
WARP_PLANE = (192, 144, 208)                   # width, height, stride of the main reference plane
WARP_SMALL = (6, 5, 16)                        # narrower than a filter's 8 taps and lower than a cell's 15 rows: both clamps bind inside one filter


def warp_plane(bd, dt, which=0, small=False):
    """the reference plane: four regions of random / max / 0 / checker-and-binary content; the samples between width and stride are never read"""
    w, h, stride = WARP_SMALL if small else WARP_PLANE
    rng = np.random.default_rng(4600 + bd + 10 * which + small)
    mx = (1 << bd) - 1
    p = rng.integers(0, mx + 1, (h, stride)).astype(dt)
    if small: p[0, 0] = mx; p[h - 1, w - 1] = 0; p[2, :w] = (np.arange(w) & 1) * mx
    else:
        yy, xx = np.mgrid[0:h // 2, 0:w // 2]
        p[:h // 2, w // 2:w] = 0 if which else mx; p[h // 2:, :w // 2] = mx if which else 0
        p[h // 2:, w // 2:w] = np.where(xx < w // 4, ((yy + xx) & 1) * mx, rng.integers(0, 2, (h // 2, w // 2)) * mx)
    return p


def _aim(mat, ss, px, py, tx, ty):
    """set the translation so that the block sample (px, py) lands on plane sample (tx, ty), plus the model's own fraction of a sample"""
    sx, sy = px << ss[0], py << ss[1]
    mat[0] = ((tx << ss[0]) << 16) - (mat[2] * sx + mat[3] * sy) + (mat[0] & 0xffff)
    mat[1] = ((ty << ss[1]) << 16) - (mat[4] * sx + mat[5] * sy) + (mat[1] & 0xffff)


def _warp_record(bl, rng, cls, k, ss, x, y, w, h, plane):
    """one record of class cls for the w x h block at (x, y) of the destination plane; k picks the corner, the fraction and where along the edge"""
    PW, PH, _ = plane
    if cls in ("random", "extreme"):
        mat, a, b, g, d = warp_model(rng, extreme=(cls == "extreme"))
        _aim(mat, ss, x + w // 2, y + h // 2, PW // 4 + (37 * k) % (PW // 2), PH // 4 + (23 * k) % (PH // 2))
    else:
        mat, a, b, g, d = [(k * 9973) & 0xffff, (k * 7919) & 0xffff, 1 << 16, 0, 0, 1 << 16], 0, 0, 0, 0
        inx, iny = 8 + (13 * k) % max(1, PW - w - 16), 8 + (11 * k) % max(1, PH - h - 16)
        tx, ty = {"left": (-(w + 12), iny), "right": (PW + 12, iny), "above": (inx, -(h + 12)), "below": (inx, PH + 12),
                  "astride_left": (-3, iny), "astride_right": (PW + 3 - w, iny), "astride_top": (inx, -3), "astride_bottom": (inx, PH + 3 - h),
                  "corner": ((-3, PW + 3 - w)[k & 1], (-3, PH + 3 - h)[(k >> 1) & 1])}[cls]
        _aim(mat, ss, x, y, tx, ty)
    _fill(bl, mat, (a, b, g, d), x, y, w, h)


def _fill(bl, mat, shear, x, y, w, h):
    for i in range(6): bl.mat[i] = mat[i]
    bl.alpha, bl.beta, bl.gamma, bl.delta = shear
    bl.p_col, bl.p_row, bl.p_width, bl.p_height = x, y, w, h


def warp_cells(b, ss):
    """(j, i, ix4, iy4, sx4, sy4) of every 8 x 8 cell of a record: where its filters sit in the reference plane"""
    out = []
    m = [int(v) for v in b.mat]
    for i in range(b.p_row, b.p_row + b.p_height, 8):
        for j in range(b.p_col, b.p_col + b.p_width, 8):
            sx, sy = (j + 4) << ss[0], (i + 4) << ss[1]
            x4, y4 = (m[2] * sx + m[3] * sy + m[0]) >> ss[0], (m[4] * sx + m[5] * sy + m[1]) >> ss[1]
            assert -(1 << 31) <= m[2] * sx + m[3] * sy + m[0] < (1 << 31) and -(1 << 31) <= m[4] * sx + m[5] * sy + m[1] < (1 << 31)
            out.append((j, i, x4 >> 16, y4 >> 16, ((x4 & 0xffff) - 4 * (b.alpha + b.beta)) & ~63, ((y4 & 0xffff) - 4 * (b.gamma + b.delta)) & ~63))
    return out


def warp_edge_classes(b, ss, width, height):
    """what the record's cells do at the plane's edges, from their footprints (columns ix4 - 7 .. ix4 + 7, rows iy4 - 7 .. iy4 + 7), not from its label"""
    cells = warp_cells(b, ss)
    got = set()
    lo_x, hi_x = min(c[2] for c in cells) - 7, max(c[2] for c in cells) + 7
    lo_y, hi_y = min(c[3] for c in cells) - 7, max(c[3] for c in cells) + 7
    if hi_x <= 0: got.add("left")
    if lo_x >= width - 1: got.add("right")
    if hi_y <= 0: got.add("above")
    if lo_y >= height - 1: got.add("below")
    for (_, _, ix, iy, _, _) in cells:
        L, R, T, B = ix - 7 < 0 < ix + 7, ix - 7 < width - 1 < ix + 7, iy - 7 < 0 < iy + 7, iy - 7 < height - 1 < iy + 7
        if L: got.add("astride_left")
        if R: got.add("astride_right")
        if T: got.add("astride_top")
        if B: got.add("astride_bottom")
        if (L or R) and (T or B): got.add("corner")
        if any(ix + l - 3 < 0 and ix + l + 4 > width - 1 for l in range(-4, 4)): got.add("row_both_clamps")
        if iy - 7 < 0 and iy + 7 > height - 1: got.add("column_both_clamps")
    if not got: got.add("inside")
    return got


@functools.lru_cache(maxsize=None)
def warp_cases(ss):
    """per sub-sampling (ss_x, ss_y): a list on the main plane (21 sizes x 3, the eleven classes cycling: 63 blocks) and a list on the small plane (21 blocks)
    -> [NS(name, plane = (width, height, stride), small, blks, desc, dst_w, dst_h)]"""
    out = []
    for small in (False, True):
        rounds = 1 if small else 3
        n = len(WARP_ALL_SIZES) * rounds
        blks = (WarpBlk * n)(); desc = []
        rng = np.random.default_rng(4700 + 2 * WARP_SS.index(ss) + small)
        shelf = Shelf(512, 2, 1)
        plane = WARP_SMALL if small else WARP_PLANE
        c = 0
        for (w, h) in WARP_ALL_SIZES:
            for _ in range(rounds):
                x, y = shelf.put(w, h)
                cls = ("random", "extreme", "astride_left", "corner", "random")[c % 5] if small else WARP_CLASSES[c % 11]      # 5 and 11 against 21 x 3
                if small:
                    mat, a, b, g, d = warp_model(rng, extreme=(cls == "extreme")) if cls in ("random", "extreme") else ([c * 9973 & 0xffff, c * 7919 & 0xffff, 1 << 16, 0, 0, 1 << 16], 0, 0, 0, 0)
                    _aim(mat, ss, x + (w // 2 if c % 3 else 0), y + (h // 2 if c % 3 else 0), (2, 3, -2)[c % 3], (2, 1, -1)[c % 3])
                    _fill(blks[c], mat, (a, b, g, d), x, y, w, h)
                else: _warp_record(blks[c], rng, cls, c, ss, x, y, w, h, plane)
                desc.append(dict(size=(w, h), cls=cls, edges=warp_edge_classes(blks[c], ss, plane[0], plane[1])))
                c += 1
        out.append(NS(name="small" if small else "main", plane=plane, small=small, blks=blks, desc=desc, dst_w=512, dst_h=shelf.height + 1, n=n))
    return out


def numpy_warp_block(b, plane, width, height, ss, bd, comp=None, convbuf=None, no_left_clamp=False):
    """one record, every 8 x 8 cell in turn: 15 x 8 horizontally filtered samples with a filter per sample, then 8 x 8 (or what the block leaves of it) vertical
    sums.  -> samples [h][w]; with comp = (do_average, use_jnt_comp_avg, fwd, bck) the compound tail: the 16-bit values when do_average is 0, otherwise pixels
    from them and convbuf [h][w].  plane is indexed [row][column] (its stride is its second dimension).  no_left_clamp: the wrong variant (columns left of the
    plane wrap to its right end)"""
    F = warped_filters()
    P = plane.astype(np.int64)
    hbd = plane.dtype.itemsize == 2
    r0, r1 = (5 if bd == 12 else 3), 7
    rbh = r0 + max(bd + 7 - r0 - 14, 0) if hbd else r0
    rbv, obh, obv = (r1 if comp else 14 - rbh), bd + 6, bd + 14 - rbh
    out = np.zeros((b.p_height, b.p_width), np.int64)
    kk, ll, mm = np.arange(-7, 8)[:, None, None], np.arange(-4, 4)[None, :, None], np.arange(8)[None, None, :]
    for (j, i, ix4, iy4, sx4, sy4) in warp_cells(b, ss):
        rows = np.clip(iy4 + kk, 0, height - 1)
        cols = ix4 + ll - 3 + mm
        cols = np.where(cols < 0, cols % width, np.minimum(cols, width - 1)) if no_left_clamp else np.clip(cols, 0, width - 1)
        fh = F[rp2(sx4 + b.beta * (kk + 4) + b.alpha * (ll + 4), 10) + 64]                 # [15][8][1][8 taps]
        tmp = rp2((1 << obh) + (P[rows, cols] * fh[:, :, 0, :]).sum(-1), rbh)             # [15][8]
        k2, l2 = np.arange(-4, 4)[:, None], np.arange(-4, 4)[None, :]
        fv = F[rp2(sy4 + b.delta * (k2 + 4) + b.gamma * (l2 + 4), 10) + 64]               # [8][8][8 taps]
        win = np.stack([tmp[m:m + 8] for m in range(8)], -1)                              # [8][8][8]: rows k + m + 4 of column l
        s = rp2((1 << obv) + (win * fv).sum(-1), rbv)
        y0, x0 = i - b.p_row, j - b.p_col
        ch, cw = min(8, b.p_height - y0), min(8, b.p_width - x0)
        out[y0:y0 + ch, x0:x0 + cw] = s[:ch, :cw]
    if comp is None: return np.clip(out - (1 << (bd - 1)) - (1 << bd), 0, (1 << bd) - 1)
    do_average, jnt, fwd, bck = comp
    if not do_average: return out & 0xffff
    ob = bd + 14 - r0
    t = (convbuf.astype(np.int64) * fwd + out * bck) >> 4 if jnt else (convbuf.astype(np.int64) + out) >> 1
    return np.clip(rp2(t - (1 << (ob - r1)) - (1 << (ob - r1 - 1)), 14 - r0 - r1), 0, (1 << bd) - 1)


def warp_expected(orc, lst, ss, bd, dt):
    """(reference plane, patterned destination plane, the oracle's result on it) of one list of warp_cases(ss)"""
    plane = warp_plane(bd, dt, 0, lst.small)
    w, h, stride = lst.plane
    dst0 = pattern((lst.dst_h, lst.dst_w), dt)
    exp = dst0.copy()
    orc.orc_warp_predict_batch(plane.itemsize, bd, _vp(plane), w, h, stride, _vp(exp), lst.dst_w, ss[0], ss[1], lst.blks, lst.n)
    return plane, dst0, exp


assert C.sizeof(WarpCompBlk) == 56
WARP_COMP_SIZES = [(8, 8), (128, 128), (4, 8), (16, 32), (64, 16), (8, 4), (32, 32), (4, 16)]


@functools.lru_cache(maxsize=None)
def warp_comp_cases(ss=(0, 0)):
    """the launches of a compound warp over one compound buffer and one destination plane, in order:
      first      do_average 0, every block its own cb_off and a cb_stride wider than the block          (reference plane 0)
      second     do_average 1 over the same buffer, plain average and several DIST_PAIRS in turn         (reference plane 1)
      mixed      new first-pass blocks (fresh buffer ranges) among second passes over `first`'s ranges, at new destinations
      null_dst   a first pass with no destination plane at all
    -> NS(lists = [NS(name, which, blks, desc, null_dst)], cb_len, dst_w, dst_h)"""
    rng = np.random.default_rng(4800 + WARP_SS.index(ss))
    shelf = Shelf(256, 1, 1)
    cb = [3]                                                                               # running compound-buffer offset

    def record(bl, k, w, h, x, y, off, stride, avg, jnt, pair):
        _warp_record(bl.blk, rng, ("random", "astride_left", "extreme", "corner", "random", "astride_bottom", "random")[k % 7], k, ss, x, y, w, h, WARP_PLANE)
        bl.cb_off, bl.cb_stride, bl.do_average, bl.use_jnt_comp_avg = off, stride, avg, jnt
        bl.fwd_offset, bl.bck_offset = pair if jnt else (0, 0)
        return dict(size=(w, h), do_average=avg, jnt=jnt, dist=(int(bl.fwd_offset), int(bl.bck_offset)), cb_off=off, cb_stride=stride)

    def fresh(w, h, k):
        off, stride = cb[0], w + (1, 6, 3, 11)[k % 4]
        cb[0] += stride * h + (1, 2, 5)[k % 3]
        return off, stride

    n = len(WARP_COMP_SIZES)
    first, second = (WarpCompBlk * n)(), (WarpCompBlk * n)()
    d1, d2 = [], []
    for k, (w, h) in enumerate(WARP_COMP_SIZES):
        x, y = shelf.put(w, h)
        off, stride = fresh(w, h, k)
        d1.append(record(first[k], k, w, h, x, y, off, stride, 0, 0, None))
        d2.append(record(second[k], k + 3, w, h, x, y, off, stride, 1, k % 3 != 0, DIST_PAIRS[(3 * k) % 8]))
    mixed = (WarpCompBlk * n)(); d3 = []
    for k, (w, h) in enumerate(WARP_COMP_SIZES):
        x, y = shelf.put(w, h)
        if k % 2: d3.append(record(mixed[k], k + 5, w, h, x, y, *fresh(w, h, k + 1), 0, 0, None))
        else: d3.append(record(mixed[k], k + 6, w, h, x, y, first[k].cb_off, first[k].cb_stride, 1, k % 4 == 0, DIST_PAIRS[(5 * k + 3) % 8]))
    m = 3
    nulld = (WarpCompBlk * m)(); d4 = []
    for k, (w, h) in enumerate(WARP_COMP_SIZES[:m]):
        d4.append(record(nulld[k], k + 9, w, h, 8 * k, 4 * k, *fresh(w, h, k + 2), 0, 0, None))
    lists = [NS(name="first", which=0, blks=first, desc=d1, null_dst=False), NS(name="second", which=1, blks=second, desc=d2, null_dst=False),
             NS(name="mixed", which=1, blks=mixed, desc=d3, null_dst=False), NS(name="null_dst", which=0, blks=nulld, desc=d4, null_dst=True)]
    return NS(lists=lists, cb_len=cb[0] + 5, dst_w=256, dst_h=shelf.height + 1, ss=ss)


def warp_comp_expected(orc, c, bd, dt):
    """the four launches in order on one compound buffer and one destination plane -> per launch (buffer after, plane after), from patterned starts"""
    w, h, stride = WARP_PLANE
    planes = [warp_plane(bd, dt, 0), warp_plane(bd, dt, 1)]
    cb = pattern((c.cb_len,), np.uint16, 40000, 1021); dst = pattern((c.dst_h, c.dst_w), dt)
    steps = [(cb.copy(), dst.copy())]
    for l in c.lists:
        orc.orc_warp_compound_batch(planes[0].itemsize, bd, _vp(planes[l.which]), w, h, stride, None if l.null_dst else _vp(dst), c.dst_w, c.ss[0], c.ss[1],
                                    _vp(cb), l.blks, len(l.blks))
        steps.append((cb.copy(), dst.copy()))
    return planes, steps
