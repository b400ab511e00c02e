"""Shared by the mode-decision precompute tests: the 85 square PUs of a 64x64 superblock in the order of the open-loop ME results (64x64, 32x32 x 4, 16x16 x 16,
8x8 x 64: EbMeTierZeroPu, Encoder/Codec/EbMotionEstimationLcuResults.h) — any order works for the entry point, which takes the list as an argument — and a
synthetic picture with its reference planes and a vector table."""
import ctypes as C
import functools

import numpy as np


def square_pus():
    pus = [(0, 0, 64, 64)]
    for s, n in ((32, 2), (16, 4), (8, 8)):
        pus += [(x * s, y * s, s, s) for y in range(n) for x in range(n)]
    return pus


def make_case(rng, w, h, n_refs, pad=40, mv_range=24, frac_none=0.1):
    """source + n_refs padded reference planes of a w x h picture, and [n_sb][85][n_refs] vectors (whole samples) some of which are 'none' and some of which
    point outside the reference's allocation"""
    sb_cols, sb_rows = (w + 63) // 64, (h + 63) // 64
    n_sb = sb_cols * sb_rows
    base = rng.integers(0, 256, (h + 2 * pad + 64, w + 2 * pad + 64)).astype(np.uint8)
    src = np.ascontiguousarray(base[pad:pad + h, pad:pad + w])
    refs = []
    for r in range(n_refs):
        dx, dy = int(rng.integers(-6, 7)), int(rng.integers(-6, 7))
        p = base[pad + dy - pad:pad + dy + h + pad, pad + dx - pad:pad + dx + w + pad].astype(np.int16) if min(pad + dy - pad, pad + dx - pad) >= 0 else None
        if p is None:
            p = rng.integers(0, 256, (h + 2 * pad, w + 2 * pad)).astype(np.int16)
        p = np.clip(p + rng.integers(-3, 4, p.shape), 0, 255).astype(np.uint8)
        if r == 1: p[:] = 255   # saturated differences
        refs.append(np.ascontiguousarray(p))
    pus = square_pus()
    mvx = rng.integers(-mv_range, mv_range + 1, (n_sb, len(pus), n_refs)).astype(np.int16)
    mvy = rng.integers(-mv_range, mv_range + 1, (n_sb, len(pus), n_refs)).astype(np.int16)
    far = rng.random(mvx.shape) < 0.03
    mvx[far] = rng.integers(-3 * pad, 3 * pad, int(far.sum())).astype(np.int16)   # some of these leave the allocation
    mvx[rng.random(mvx.shape) < frac_none] = -32768
    mv = (mvx.astype(np.uint16).astype(np.uint32)) | (mvy.astype(np.uint16).astype(np.uint32) << 16)
    return src, refs, pus, np.ascontiguousarray(mv), sb_cols, n_sb, pad


def oracle_table(orc, src, refs, pus, mv, sb_cols, n_sb, pad, pic_w, pic_h):
    n_refs = len(refs)
    pu4 = np.array(pus, np.uint8)
    planes = (C.c_void_p * n_refs)(*[r.ctypes.data + pad * r.shape[1] + pad for r in refs])
    strides = (C.c_int * n_refs)(*[r.shape[1] for r in refs])
    box = np.array([[-pad, -pad, r.shape[1] - pad, r.shape[0] - pad] for r in refs], np.int32)
    out = np.zeros(mv.shape, np.uint32)
    orc.orc_md_fullpel_sad_picture(src.ctypes.data_as(C.c_void_p), src.shape[1], pic_w, pic_h, sb_cols, n_sb, len(pus), pu4.ctypes.data_as(C.c_void_p), n_refs, planes, strides,
                                   box.ctypes.data_as(C.c_void_p), mv.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def oracle_grid(orc, src, refs, pus, mv, sb_cols, n_sb, pad, pic_w, pic_h, bank):
    """the 7 x 7 sub-pel grid table of svt_hip_md_subpel_grid_picture_dev by the oracle: [n_sb][n_pus][n_refs][49][2]"""
    n_refs = len(refs)
    pu4 = np.array(pus, np.uint8)
    planes = (C.c_void_p * n_refs)(*[r.ctypes.data + pad * r.shape[1] + pad for r in refs])
    strides = (C.c_int * n_refs)(*[r.shape[1] for r in refs])
    box = np.array([[-pad, -pad, r.shape[1] - pad, r.shape[0] - pad] for r in refs], np.int32)
    out = np.zeros(mv.shape + (49, 2), np.uint32)
    orc.orc_md_subpel_grid_picture(src.ctypes.data_as(C.c_void_p), src.shape[1], pic_w, pic_h, sb_cols, n_sb, len(pus), pu4.ctypes.data_as(C.c_void_p), n_refs, planes, strides,
                                   box.ctypes.data_as(C.c_void_p), mv.ctypes.data_as(C.c_void_p), bank, out.ctypes.data_as(C.c_void_p))
    return out


def oracle_avg_table(orc, src, refs, pus, mv, sb_cols, n_sb, pad, pic_w, pic_h, pairs):
    """the compound-average table of svt_hip_md_fullpel_avg_sad_picture_dev by the oracle: [n_sb][n_pus][n_pairs]"""
    n_refs = len(refs)
    pu4 = np.array(pus, np.uint8)
    planes = (C.c_void_p * n_refs)(*[r.ctypes.data + pad * r.shape[1] + pad for r in refs])
    strides = (C.c_int * n_refs)(*[r.shape[1] for r in refs])
    box = np.array([[-pad, -pad, r.shape[1] - pad, r.shape[0] - pad] for r in refs], np.int32)
    pr = np.array(pairs, np.uint8)
    out = np.zeros(mv.shape[:2] + (len(pairs),), np.uint32)
    orc.orc_md_fullpel_avg_sad_picture(src.ctypes.data_as(C.c_void_p), src.shape[1], pic_w, pic_h, sb_cols, n_sb, len(pus), pu4.ctypes.data_as(C.c_void_p), n_refs, planes, strides,
                                       box.ctypes.data_as(C.c_void_p), mv.ctypes.data_as(C.c_void_p), len(pairs), pr.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


# ------------------------------------------------------------------------------------------------ case builders shared by tests/test_md_ref_cpu.py and tests/test_md_pre_gpu.py
# Every builder returns the inputs and the expected table(s), and asserts on the way that the oracle's table equals a plain numpy statement (int64) of the same operation on
# every slot.  No case invites a wrong bounds check into a bad read: the boxes handed to the entry points lie MARGIN samples inside the real allocation on every side, and so
# does the source, so a wrong check shows as a wrong number.
MARGIN = 16
NO_MV = -32768
NOT_COMPUTED = 0xffffffff
SENTINEL = 0xa5a5a5a5          # what the device tests fill a table with before the launch: a slot nobody wrote is seen
GRID_OFF = ((-1, 2), (-1, 4), (-1, 6), (0, 0), (0, 2), (0, 4), (0, 6))   # grid offset -6 .. 6 eighth-samples = (whole samples, phase in eighths)
SIDES = ("left", "top", "right", "bottom")


class Plane:
    """A plane as an entry point sees it: sample (0, 0) is buf[oy, ox] of a larger C-contiguous buffer, `box` = (x_min, y_min, x_max, y_max) is what the caller declares of it
    (a reference's allocation box; the picture for a source).  The box lies MARGIN samples inside the buffer on every side."""

    def __init__(self, box, dtype, rng=None, hi=256, stride=None, shift=0):
        x0, y0, x1, y1 = box
        cols = stride if stride is not None else x1 - x0 + 2 * MARGIN + shift
        rows = y1 - y0 + 2 * MARGIN
        self.buf = (rng.integers(0, hi, (rows, cols)) if rng is not None else np.zeros((rows, cols))).astype(dtype)
        self.box, self.ox, self.oy, self.stride = tuple(box), MARGIN + shift - x0, MARGIN - y0, cols
        self.off = self.oy * cols + self.ox                    # of sample (0, 0), in samples from the start of the buffer
        assert self.ox + x0 >= MARGIN and self.ox + x1 + MARGIN <= cols and self.oy + y0 >= MARGIN and self.oy + y1 + MARGIN <= rows

    def view(self, x, y, w, h):
        r0, c0 = self.oy + y, self.ox + x
        assert 0 <= r0 and r0 + h <= self.buf.shape[0] and 0 <= c0 and c0 + w <= self.buf.shape[1], (x, y, w, h)
        return self.buf[r0:r0 + h, c0:c0 + w]

    def block(self, x, y, w, h):
        return self.view(x, y, w, h).astype(np.int64)

    def freeze(self):
        self.buf.setflags(write=False)
        return self

    @property
    def host(self):
        return C.c_void_p(self.buf.ctypes.data + self.off * self.buf.itemsize)

    def align(self, x=0, y=0):
        """address & 3 of sample (x, y) on the device, where the buffer starts at an allocation's (256-byte aligned) address"""
        return ((self.off + y * self.stride + x) * self.buf.itemsize) & 3


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def sb_cols(self): return (self.pic_w + 63) // 64

    @property
    def n_sb(self): return self.sb_cols * ((self.pic_h + 63) // 64)

    def slots(self):
        """(sb, pu, x, y, w, h) of every (superblock, PU), picture coordinates"""
        for sb in range(self.n_sb):
            for p, (px, py, w, h) in enumerate(self.pus):
                yield sb, p, (sb % self.sb_cols) * 64 + px, (sb // self.sb_cols) * 64 + py, w, h


def mv_words(mx, my):
    return np.ascontiguousarray(np.asarray(mx).astype(np.int16).astype(np.uint16).astype(np.uint32) | (np.asarray(my).astype(np.int16).astype(np.uint16).astype(np.uint32) << 16))


def mv_xy(word):
    word = int(word)
    lo, hi = word & 0xffff, word >> 16
    return lo - 65536 if lo >= 32768 else lo, hi - 65536 if hi >= 32768 else hi


def sad_extent(w, h):
    """what a full-pel candidate needs of its reference, relative to the block's origin there: [0, w + 4) x [0, h) — rows are read as whole dwords"""
    return 0, 0, w + 4, h


def grid_extent(s):
    """what the 7 x 7 grid needs: the 8-tap window [-4, s + 4) both ways, and 4 more columns for the dwords"""
    return -4, -4, s + 8, s + 4


def computed(c, ref, x, y, w, h, mx, my, extent):
    """the "not computed" rule of include/svt_hip.h: a vector, the PU inside the picture, what the kernel reads of the reference inside its box"""
    lx, ty, rx, by = extent
    x_min, y_min, x_max, y_max = ref.box
    return mx != NO_MV and x + w <= c.pic_w and y + h <= c.pic_h and x + mx + lx >= x_min and y + my + ty >= y_min and x + mx + rx <= x_max and y + my + by <= y_max


def numpy_sad(a, b):
    return int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum())


def numpy_avg_sad(s, a, b):
    return int(np.abs(s.astype(np.int64) - ((a.astype(np.int64) + b.astype(np.int64) + 1) >> 1)).sum())


def interp_taps(orc):
    """the oracle's interpolation kernels [bank][sixteenth-sample phase][tap] (pinned to the reference by tests/test_oracle_vs_ref.py::test_interp_kernels_and_convolve_sr)"""
    return np.ctypeslib.as_array((C.c_int16 * 8 * 16 * 6).in_dll(orc, "orc_interp_kernels")).astype(np.int64)


def numpy_grid(src, ref, x, y, s, mx, my, bank, taps, probe=None):
    """(variance, sse) [49][2] of the s x s PU at (x, y) of Plane `src` against the 49 quarter-pel positions around vector (mx, my) into Plane `ref`: a horizontal 8-tap pass
    over the window, clip((sum + 64) >> 7, 0, 255), a vertical pass the same way, then the statistics — phase 0 included (its tap is 128).  taps = interp_taps(orc), or a
    changed copy; probe (a dict) collects whether either clip of either pass was ever needed."""
    S = src.block(x, y, s, s)
    W = ref.block(x + mx - 4, y + my - 4, s + 8, s + 8)
    H = np.zeros((7, s + 8, s), np.int64)
    seen = dict(h_lo=False, h_hi=False, v_lo=False, v_hi=False)
    for a, (ix, fx) in enumerate(GRID_OFF):
        k = taps[bank][2 * fx]
        pre = (sum(int(k[t]) * W[:, ix + 1 + t:ix + 1 + t + s] for t in range(8)) + 64) >> 7
        seen["h_lo"] |= bool((pre < 0).any()); seen["h_hi"] |= bool((pre > 255).any())
        H[a] = np.clip(pre, 0, 255)
    out = np.zeros((49, 2), np.uint32)
    for b, (iy, fy) in enumerate(GRID_OFF):
        k = taps[bank][2 * fy]
        pre = (sum(int(k[t]) * H[:, iy + 1 + t:iy + 1 + t + s, :] for t in range(8)) + 64) >> 7
        seen["v_lo"] |= bool((pre < 0).any()); seen["v_hi"] |= bool((pre > 255).any())
        d = np.clip(pre, 0, 255) - S
        for a in range(7):
            sse, sm = int((d[a] * d[a]).sum()), int(d[a].sum())
            out[7 * b + a] = ((sse - sm * sm // (s * s)) % (1 << 32), sse)
    if probe is not None:
        for name, v in seen.items(): probe[name] = probe.get(name, False) or v
    return out


def numpy_sad_table(c):
    out = np.full(c.mv.shape, NOT_COMPUTED, np.uint32)
    for sb, p, x, y, w, h in c.slots():
        for r, ref in enumerate(c.refs):
            mx, my = mv_xy(c.mv[sb, p, r])
            if computed(c, ref, x, y, w, h, mx, my, sad_extent(w, h)):
                out[sb, p, r] = numpy_sad(c.src.block(x, y, w, h), ref.block(x + mx, y + my, w, h))
    return out


def numpy_avg_table(c):
    out = np.full(c.mv.shape[:2] + (len(c.pairs),), NOT_COMPUTED, np.uint32)
    for sb, p, x, y, w, h in c.slots():
        for q, (c0, c1) in enumerate(c.pairs):
            (mx0, my0), (mx1, my1) = mv_xy(c.mv[sb, p, c0]), mv_xy(c.mv[sb, p, c1])
            if computed(c, c.refs[c0], x, y, w, h, mx0, my0, sad_extent(w, h)) and computed(c, c.refs[c1], x, y, w, h, mx1, my1, sad_extent(w, h)):
                out[sb, p, q] = numpy_avg_sad(c.src.block(x, y, w, h), c.refs[c0].block(x + mx0, y + my0, w, h), c.refs[c1].block(x + mx1, y + my1, w, h))
    return out


def numpy_grid_table(c, taps, probe=None):
    out = np.full(c.mv.shape + (49, 2), NOT_COMPUTED, np.uint32)
    for sb, p, x, y, w, h in c.slots():
        for r, ref in enumerate(c.refs):
            mx, my = mv_xy(c.mv[sb, p, r])
            if w == h and w in (8, 16, 32, 64) and computed(c, ref, x, y, w, h, mx, my, grid_extent(w)):
                out[sb, p, r] = numpy_grid(c.src, ref, x, y, w, mx, my, c.bank, taps, probe)
    return out


def halfpel_of(grid):
    """the 3 x 3 half-pel table [...][9][2] = positions (1, 3, 5) x (1, 3, 5) of the 7 x 7 table [...][49][2]"""
    return np.ascontiguousarray(grid.reshape(grid.shape[:-2] + (7, 7, 2))[..., 1::2, 1::2, :]).reshape(grid.shape[:-2] + (9, 2))


def _orc_args(c):
    """the arguments the oracle's three picture functions share (the ctypes pointers keep their arrays alive)"""
    n = len(c.refs)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    pu4, box = np.array(c.pus, np.uint8), np.array([r.box for r in c.refs], np.int32)
    return vp, (c.src.host, c.src.stride, c.pic_w, c.pic_h, c.sb_cols, c.n_sb, len(c.pus), vp(pu4), n, (C.c_void_p * n)(*[r.host for r in c.refs]),
                (C.c_int * n)(*[r.stride for r in c.refs]), vp(box), vp(c.mv))


def oracle_sad_table(orc, c):
    vp, args = _orc_args(c)
    out = np.zeros(c.mv.shape, np.uint32)
    (orc.orc_md_fullpel_sad_picture if c.src.buf.itemsize == 1 else orc.orc_md_fullpel_sad_picture16)(*args, vp(out))
    return out


def oracle_avg_sad_table(orc, c):
    vp, args = _orc_args(c)
    pr = np.array(c.pairs, np.uint8)
    out = np.zeros(c.mv.shape[:2] + (len(c.pairs),), np.uint32)
    if c.src.buf.itemsize == 1: orc.orc_md_fullpel_avg_sad_picture(*args, len(c.pairs), vp(pr), vp(out))
    else: orc.orc_md_fullpel_avg_sad_picture16(*args, len(c.pairs), vp(pr), 10, vp(out))
    return out


def oracle_grid_table(orc, c):
    vp, args = _orc_args(c)
    out = np.zeros(c.mv.shape + (49, 2), np.uint32)
    orc.orc_md_subpel_grid_picture(*args, c.bank, vp(out))
    return out


def _frozen(a):
    a.setflags(write=False)
    return a


def _expect(c, orc, sad=False, avg=False, grid=False, probe=None):
    """fills c.exp_sad / c.exp_avg / c.exp_grid (+ c.exp_half) with the oracle's tables after checking them against numpy's, slot by slot"""
    c.src.freeze()
    for r in c.refs: r.freeze()
    c.mv = _frozen(np.ascontiguousarray(c.mv, np.uint32))
    for on, name, o_fn, n_fn in ((sad, "exp_sad", lambda: oracle_sad_table(orc, c), lambda: numpy_sad_table(c)),
                                 (avg, "exp_avg", lambda: oracle_avg_sad_table(orc, c), lambda: numpy_avg_table(c)),
                                 (grid, "exp_grid", lambda: oracle_grid_table(orc, c), lambda: numpy_grid_table(c, interp_taps(orc), probe))):
        if on:
            o, n = o_fn(), n_fn()
            assert np.array_equal(o, n), (name, np.argwhere(o != n)[:5])
            setattr(c, name, _frozen(o))
    if grid: c.exp_half = _frozen(halfpel_of(c.exp_grid))
    return c


def _dtype_max(bits):
    return (np.uint8, 255) if bits == 8 else (np.uint16, 1023)     # the 16-bit planes are a 10-bit encode's


# ---- (a) every width x the heights at which the kernels' row loop turns over
# the widths whose w / 4 does not divide 64, and the first height at which a wave that lets its lanes past the last whole row add counts a row twice
FIRST_WRONG_H = {12: 22, 20: 13, 24: 11, 28: 10, 36: 8, 40: 7, 44: 6, 48: 6, 52: 5, 56: 5, 60: 5}
WIDTHS_PAIRS = ((0, 1), (1, 0), (1, 1), (0, 0))


def width_height_pus():
    pus = []
    for w in range(4, 65, 4):
        rows = 64 // (w // 4)                                    # rows a wave covers in one step
        for h in sorted({min(max(v, 1), 64) for v in (1, rows, rows + 1, 2 * rows + 1, 4 * rows, 4 * rows + 1, 64)}):
            k = len(pus) % 4                                       # against alternating corners of the superblock
            pus.append(((64 - w) * (k & 1), (64 - h) * (k >> 1), w, h))
    return pus


@functools.lru_cache(maxsize=None)
def widths_case(orc, bits):
    """128 x 64, 2 references, vectors within +-8; superblock 1 of the source is all 0 and reference 1 all max"""
    dt, mx_val = _dtype_max(bits)
    rng = np.random.default_rng(100 + bits)
    pus = width_height_pus()
    assert len(pus) <= 128 and {p[2] for p in pus} == set(range(4, 65, 4))
    for w, first in FIRST_WRONG_H.items():
        assert any(p[2] == w and p[3] >= first for p in pus), w
    assert all(p[0] + p[2] <= 64 and p[1] + p[3] <= 64 for p in pus) and len({(p[0] > 0, p[1] > 0) for p in pus}) == 4
    pic_w, pic_h, pad = 128, 64, 24
    src = Plane((0, 0, pic_w, pic_h), dt, rng, mx_val + 1)
    src.view(64, 0, 64, 64)[:] = 0
    box = (-pad, -pad, pic_w + pad, pic_h + pad)
    refs = [Plane(box, dt, rng, mx_val + 1), Plane(box, dt, rng, mx_val + 1, shift=2)]
    refs[1].view(-pad, -pad, pic_w + 2 * pad, pic_h + 2 * pad)[:] = mx_val
    mvx, mvy = rng.integers(-8, 9, (2, len(pus), 2)), rng.integers(-8, 9, (2, len(pus), 2))
    assert (mvx % 2 == 1).any() and (mvy % 2 == 1).any() and (mvx % 2 == 0).any() and abs(mvx).max() <= 8 and abs(mvy).max() <= 8
    c = _expect(Case(src=src, refs=refs, pus=pus, mv=mv_words(mvx, mvy), pic_w=pic_w, pic_h=pic_h, pairs=WIDTHS_PAIRS, max=mx_val), orc, sad=True, avg=True)
    assert (c.exp_sad != NOT_COMPUTED).all() and (c.exp_avg != NOT_COMPUTED).all()
    area = np.array([p[2] * p[3] for p in pus], np.int64)
    assert np.array_equal(c.exp_sad[1, :, 1], area * mx_val) and np.array_equal(c.exp_avg[1, :, 2], area * mx_val)    # all max against all 0
    return c


# ---- (b) blocks flush with each side of a reference's box, and one sample past it
EDGE_SAD_BLOCKS = ((4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (64, 16), (12, 24))
EDGE_GRID_SIZES = (8, 16, 32, 64)
EDGE_PAIRS = ((0, 2), (2, 0), (1, 2), (2, 1))      # column 2 always holds a vector well inside: each edge vector is the first and the second of a pair in turn


def edge_slot(sb, p, r):
    """(side, past) of the vector in column r < 2 of PU p of superblock sb: the four superblocks take the four sides, the two columns flush / one past"""
    return SIDES[sb], (r ^ p) & 1


@functools.lru_cache(maxsize=None)
def edges_case(orc, bits, grid):
    """128 x 128 (four superblocks), three references with boxes of their own; grid: the PUs of the sub-pel grid (8 bits, bank 2) instead of the SAD blocks"""
    dt, mx_val = _dtype_max(bits)
    rng = np.random.default_rng(200 + bits + grid)
    pic_w = pic_h = 128
    if grid: pus = [(56, 48, 8, 8), (16, 32, 16, 16), (32, 0, 32, 32), (0, 0, 64, 64)]
    else: pus = [((64 - w) * (i & 1), (64 - h) * ((i >> 1) & 1), w, h) for i, (w, h) in enumerate(EDGE_SAD_BLOCKS)]
    assert [p[2:] for p in pus] == ([(s, s) for s in EDGE_GRID_SIZES] if grid else list(EDGE_SAD_BLOCKS))
    src = Plane((0, 0, pic_w, pic_h), dt, rng, mx_val + 1)
    boxes = [(-40, -36, pic_w + 44, pic_h + 40), (-33, -41, pic_w + 37, pic_h + 35), (-32, -32, pic_w + 32, pic_h + 32)]
    refs = [Plane(b, dt, rng, mx_val + 1, shift=i) for i, b in enumerate(boxes)]
    mvx, mvy = np.zeros((4, len(pus), 3), np.int64), np.zeros((4, len(pus), 3), np.int64)
    c = Case(src=src, refs=refs, pus=pus, pic_w=pic_w, pic_h=pic_h, pairs=EDGE_PAIRS, bank=2)
    for sb, p, x, y, w, h in c.slots():
        lx, ty, rx, by = grid_extent(w) if grid else sad_extent(w, h)
        for r in range(2):
            x_min, y_min, x_max, y_max = boxes[r]
            side, past = edge_slot(sb, p, r)
            ax, ay = int(rng.integers(-5, 6)), int(rng.integers(-5, 6))             # the other coordinate: anywhere well inside
            if side == "left": ax = x_min - lx - x - past
            elif side == "right": ax = x_max - rx - x + past
            elif side == "top": ay = y_min - ty - y - past
            else: ay = y_max - by - y + past
            mvx[sb, p, r], mvy[sb, p, r] = ax, ay
        mvx[sb, p, 2], mvy[sb, p, 2] = rng.integers(-6, 7, 2)
    c.mv = mv_words(mvx, mvy)
    _expect(c, orc, sad=not grid, avg=not grid, grid=bool(grid))
    done = (c.exp_grid[..., 0, 1] if grid else c.exp_sad) != NOT_COMPUTED
    for p in range(len(pus)):
        for sb in range(4):
            kinds = {edge_slot(sb, p, r)[1]: bool(done[sb, p, r]) for r in range(2)}
            assert kinds == {0: True, 1: False}, (p, SIDES[sb])                     # flush: computed; one past: not
            if not grid:   # pairs (r, 2) and (2, r): not computed exactly when the edge vector is one past, whichever of the two it is
                for q, (c0, c1) in enumerate(EDGE_PAIRS):
                    assert bool(c.exp_avg[sb, p, q] != NOT_COMPUTED) == kinds[edge_slot(sb, p, min(c0, c1))[1]]
        assert done[:, p, 2].all()
        assert {edge_slot(sb, p, r) for sb in range(4) for r in range(2)} == {(s, k) for s in SIDES for k in (0, 1)}
    return c


# ---- (c) planes at every alignment
UNALIGNED = ((8, 1), (8, 2), (8, 3), (16, 1))       # (bits, samples the source pointer is off a dword)
UNALIGNED_PAIRS = ((0, 1), (1, 0))
UNALIGNED_EXTRA_PUS = ((4, 1, 8, 8), (12, 2, 16, 16), (20, 3, 32, 32), (5, 7, 8, 8), (27, 13, 16, 16))   # origins off the 8-sample lattice of the square PUs


@functools.lru_cache(maxsize=None)
def unaligned_case(orc, bits, shift):
    """128 x 64, the 85 square PUs and five at odd origins, 2 references; source stride 203 and the source pointer `shift` samples off a dword, odd reference strides, sample (0, 0) of a reference
    at an odd sample; grid tables (8 bits only) with bank 2"""
    dt, mx_val = _dtype_max(bits)
    rng = np.random.default_rng(300 + bits + shift)
    pic_w, pic_h, pad = 128, 64, 48
    src = Plane((0, 0, pic_w, pic_h), dt, rng, mx_val + 1, stride=203, shift=shift)
    box = (-pad, -pad, pic_w + pad, pic_h + pad)
    refs = [Plane(box, dt, rng, mx_val + 1, shift=1), Plane(box, dt, rng, mx_val + 1, shift=3)]
    assert src.stride == 203 and src.off % 4 == shift and all(r.stride % 2 == 1 and r.off % 2 == 1 for r in refs)
    pus = square_pus() + list(UNALIGNED_EXTRA_PUS)
    mvx, mvy = rng.integers(-20, 21, (2, len(pus), 2)), rng.integers(-20, 21, (2, len(pus), 2))
    mvx[rng.random(mvx.shape) < 0.05] = NO_MV
    c = Case(src=src, refs=refs, pus=pus, mv=mv_words(mvx, mvy), pic_w=pic_w, pic_h=pic_h, pairs=UNALIGNED_PAIRS, bank=2)
    _expect(c, orc, sad=True, avg=True, grid=bits == 8)
    assert src.align() == (shift * src.buf.itemsize) & 3
    want = {0, 1, 2, 3} if bits == 8 else {0, 2}
    assert {src.align(x, y) for _, _, x, y, _, _ in c.slots()} == want                       # the source side of the loads sees every alignment
    for r, ref in enumerate(refs):
        assert {ref.align(x + mv_xy(c.mv[sb, p, r])[0], y + mv_xy(c.mv[sb, p, r])[1]) for sb, p, x, y, _, _ in c.slots() if c.exp_sad[sb, p, r] != NOT_COMPUTED} == want
    assert (c.exp_sad != NOT_COMPUTED).sum() > 250 and (c.exp_sad == NOT_COMPUTED).any()
    return c


# ---- (d) all six interpolation banks on content that reaches the outer taps and both clips
def zero_outer_taps(taps, bank):
    """a copy of the kernels in which the two outermost non-zero taps of every non-zero phase of `bank` are 0"""
    t = taps.copy()
    for ph in range(1, 16):
        nz = np.flatnonzero(t[bank][ph])
        t[bank][ph][[nz[0], nz[-1]]] = 0
    return t


@functools.lru_cache(maxsize=None)
def banks_case(orc, bank):
    """128 x 64, 2 references, pad 48, the 85 square PUs: reference 0 is 0 / 255 noise, reference 1 flat 255 / 0 halves whose edges run through PUs of every size"""
    rng = np.random.default_rng(400)                                # the same picture for every bank
    pic_w, pic_h, pad = 128, 64, 48
    src = Plane((0, 0, pic_w, pic_h), np.uint8, rng)
    box = (-pad, -pad, pic_w + pad, pic_h + pad)
    refs = [Plane(box, np.uint8, rng), Plane(box, np.uint8, rng, shift=3)]
    refs[0].view(-pad, -pad, pic_w + 2 * pad, pic_h + 2 * pad)[:] = np.where(rng.random((pic_h + 2 * pad, pic_w + 2 * pad)) < 0.5, 0, 255)
    yy, xx = np.mgrid[-pad:pic_h + pad, -pad:pic_w + pad]
    refs[1].view(-pad, -pad, pic_w + 2 * pad, pic_h + 2 * pad)[:] = np.where((xx >= 53) ^ (yy >= 29) ^ (xx >= 85), 255, 0)
    pus = square_pus()
    mvx, mvy = rng.integers(-20, 21, (2, len(pus), 2)), rng.integers(-20, 21, (2, len(pus), 2))
    c = Case(src=src, refs=refs, pus=pus, mv=mv_words(mvx, mvy), pic_w=pic_w, pic_h=pic_h, bank=bank, clips={})
    _expect(c, orc, grid=True, probe=c.clips)
    assert (c.exp_grid != NOT_COMPUTED).all()
    return c


def banks_case_sensitive(orc, c):
    """the sizes s for which zeroing the bank's two outermost non-zero taps changes a (variance, sse) pair of an s x s PU on reference 0"""
    taps = zero_outer_taps(interp_taps(orc), c.bank)
    hit = set()
    for sb, p, x, y, w, _ in c.slots():
        if w not in hit and not np.array_equal(numpy_grid(c.src, c.refs[0], x, y, w, *mv_xy(c.mv[sb, p, 0]), c.bank, taps), c.exp_grid[sb, p, 0]): hit.add(w)
    return hit


# ---- (e) closed forms: one 64 x 64 superblock, zero vectors, a PU of every size
CLOSED_PUS = ((0, 0, 64, 64), (32, 16, 32, 32), (16, 40, 16, 16), (8, 48, 8, 8))
CLOSED_KINDS = ("max_on_0", "0_on_max", "same", "flat_100")


@functools.lru_cache(maxsize=None)
def closed_case(orc, kind, bank):
    rng = np.random.default_rng(500)
    pad = 24
    src = Plane((0, 0, 64, 64), np.uint8, rng)
    ref = Plane((-pad, -pad, 64 + pad, 64 + pad), np.uint8, rng, shift=1)
    inside = ref.view(-pad, -pad, 64 + 2 * pad, 64 + 2 * pad)
    if kind == "max_on_0": src.view(0, 0, 64, 64)[:] = 0; inside[:] = 255
    elif kind == "0_on_max": src.view(0, 0, 64, 64)[:] = 255; inside[:] = 0
    elif kind == "same": ref.view(0, 0, 64, 64)[:] = src.view(0, 0, 64, 64)
    else: src.view(0, 0, 64, 64)[:] = 100; inside[:] = 100
    c = _expect(Case(src=src, refs=[ref], pus=list(CLOSED_PUS), mv=np.zeros((1, len(CLOSED_PUS), 1), np.uint32), pic_w=64, pic_h=64, bank=bank, kind=kind), orc, grid=True)
    for p, (_, _, s, _) in enumerate(CLOSED_PUS):
        g = c.exp_grid[0, p, 0]
        if kind in ("max_on_0", "0_on_max"): assert (g == (0, s * s * 65025)).all(), (kind, bank, s)      # the largest sse a uint32 statistic holds at s = 64
        elif kind == "same": assert tuple(g[24]) == (0, 0) and (np.delete(g[:, 1], 24) > 0).all(), (kind, bank, s)   # the centre alone reads 0
        else: assert (g == 0).all(), (kind, bank, s)
    return c


# ---- (f) other PU lists for the grid: the launcher's one-wave and four-wave launches with one side empty, and with PUs the kernel declines on both sides
GRID_LISTS = {
    "small_only": [(0, 0, 8, 8)],
    "large_only": [(0, 0, 64, 64)],
    "mixed": [(0, 0, 32, 16), (48, 8, 8, 8), (0, 0, 4, 4), (32, 32, 32, 32), (8, 8, 12, 12), (0, 0, 64, 64), (16, 48, 16, 16), (0, 0, 16, 32), (40, 24, 8, 8), (0, 32, 32, 32),
              (32, 0, 16, 16)],
}
GRID_DECLINED = ((0, 0, 4, 4), (8, 8, 12, 12), (0, 0, 16, 32), (0, 0, 32, 16))


@functools.lru_cache(maxsize=None)
def grid_list_case(orc, name):
    rng = np.random.default_rng(600)
    pic_w, pic_h, pad = 128, 64, 48
    src = Plane((0, 0, pic_w, pic_h), np.uint8, rng)
    box = (-pad, -pad, pic_w + pad, pic_h + pad)
    refs = [Plane(box, np.uint8, rng), Plane(box, np.uint8, rng, shift=1)]
    pus = GRID_LISTS[name]
    mvx, mvy = rng.integers(-20, 21, (2, len(pus), 2)), rng.integers(-20, 21, (2, len(pus), 2))
    c = _expect(Case(src=src, refs=refs, pus=pus, mv=mv_words(mvx, mvy), pic_w=pic_w, pic_h=pic_h, bank=2), orc, grid=True)
    for p, pu in enumerate(pus):
        assert (c.exp_grid[:, p] == NOT_COMPUTED).all() if pu in GRID_DECLINED else (c.exp_grid[:, p, :, :, 1] != NOT_COMPUTED).all(), pu
    return c
