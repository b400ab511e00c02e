"""Shared helpers for the ME parity tests (oracle side + HIP side)."""
import ctypes as C

import numpy as np

from conftest import load_package, ptr

pkg = load_package()
synth = __import__("importlib").import_module("svt_av1_amd.synth")


class OrcSbSearch(C.Structure):
    _fields_ = [("sb_x", C.c_int32), ("sb_y", C.c_int32), ("x_origin", C.c_int16), ("y_origin", C.c_int16),
                ("width", C.c_int16), ("height", C.c_int16)]


class OrcSearchWindow(C.Structure):
    _fields_ = [("x_origin", C.c_int16), ("y_origin", C.c_int16), ("width", C.c_int16), ("height", C.c_int16)]


def windows(orc, width, height, sa_w, sa_h, centers=None):
    """Per-SB search windows through the oracle's restatement of integer_search_sb's clamp."""
    orc.orc_me_search_window.restype = OrcSearchWindow
    orc.orc_me_search_window.argtypes = [C.c_int] * 8
    sbs = synth.sb_grid(width, height)
    arr = (OrcSbSearch * len(sbs))()
    for i, (x, y) in enumerate(sbs):
        cx, cy = centers[i] if centers is not None else (0, 0)
        v = orc.orc_me_search_window(x, y, int(cx), int(cy), sa_w, sa_h, width, height)
        arr[i] = OrcSbSearch(x, y, v.x_origin, v.y_origin, v.width, v.height)
    return arr


def windows_product(L, width, height, sa_w, sa_h, centers=None):
    """The same windows through the product's own host function (svt_hip_me_search_window, include/svt_hip.h): what a caller of the ABI uses."""
    sbs = synth.sb_grid(width, height)
    arr = (OrcSbSearch * len(sbs))()      # same record layout as SvtHipSbSearch
    for i, (x, y) in enumerate(sbs):
        cx, cy = centers[i] if centers is not None else (0, 0)
        v = L.svt_hip_me_search_window(x, y, int(cx), int(cy), sa_w, sa_h, width, height)
        arr[i] = OrcSbSearch(x, y, v.x_origin, v.y_origin, v.width, v.height)
    return arr


def oracle_frame(orc, cur_p, ref_p, stride, pad, sbs, sub_sad, begin=0, end=None):
    n = len(sbs)
    end = n if end is None else end
    sad = np.zeros((n, 85), np.uint32)
    mv = np.zeros((n, 85), np.uint32)
    orc.orc_me_fullpel_frame(ptr(cur_p), ptr(ref_p), stride, pad, pad, sbs, n, sub_sad, ptr(sad), ptr(mv), begin, end)
    return sad, mv


def hip_frame(hip, cur_p, ref_p, stride, pad, sbs, sub_sad):
    n = len(sbs)
    sad = np.zeros((n, 85), np.uint32)
    mv = np.zeros((n, 85), np.uint32)
    hip.check(hip.L.svt_hip_me_fullpel_frame(hip.h, ptr(cur_p), ptr(ref_p), stride, cur_p.shape[0], pad, pad,
                                            C.cast(sbs, C.c_void_p), n, sub_sad, ptr(sad), ptr(mv)), "me_fullpel_frame")
    return sad, mv


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# Saturated content for the 85-PU integer search: source all 0 against a window all 255 (polarity 0) or the mirror image (polarity 1), so that every packed
# 16-bit partial sum of me_fullpel_85pu_kernel reaches its largest value (a 16x16 PU: 256 * 255 = 0xFF00, key 0xFF00xxxx under the initial 0xFFFFFFFF).
# The GPU test and tests/test_reducers_ref_cpu.py build their inputs here.
PU_AREA = np.array([4096] + [1024] * 4 + [256] * 16 + [64] * 64, np.int64)
PU_LAST = (0, 4, 20, 84)                       # the PUs that hold the superblock's bottom-right sample: 64x64, the last 32x32, 16x16 and 8x8
# 8x8, 8x1: one group of 8 candidates; 16x24; 64x64: one full tile; 72x40: several tiles with ragged last ones; 4x4, 5x3: the narrow kernel
SATURATED_WINDOWS = ((8, 8), (8, 1), (16, 24), (64, 64), (72, 40), (4, 4), (5, 3))
SATURATED_STRIP_WINDOW = (336, 200)            # 67 200 candidates: the strip-walking instance


def mv_word(x, y):
    """MV word of the candidate at displacement (x, y): quarter-pel int16 halves, y << 16 | x"""
    return (((y * 4) & 0xFFFF) << 16) | ((x * 4) & 0xFFFF)


def saturated_case(orc, window, variant, pol, sub, strip=False):
    """-> padded planes cur_p / ref_p, stride, the SvtHipSbSearch records, closed-form (sad [n][85], mv [n][85]) and the list of records they hold for.
    Ordinary windows: a 192 x 192 picture, its interior superblock (64, 64) first, then the two corner ones; the strip window: the 384 x 320 picture of
    test_search_area_above_65536_candidates, its inner superblock 8.  Variants: 0 nothing planted (every candidate ties at 255 * area -- SUB: half the rows,
    doubled -- and the window's first candidate wins); 1 a whole matching superblock at the first record's last candidate (64x64 PU: unique 0 there, the
    oracle decides the rest); 2 one matching sample at the bottom-right corner of the first record's window region (SUB: on its last sampled row), which
    only the last candidate's PUs 0, 4, 20, 84 read: 255 * (area - 1) (SUB: area - 2) there, every other PU still tied at the first candidate."""
    pad = synth.PAD
    (w, h), pick = ((384, 320), [8]) if strip else ((192, 192), [4, 0, 8])
    lo, hi = (0, 255) if pol == 0 else (255, 0)
    cur_p = np.full((h + 2 * pad, w + 2 * pad), lo, np.uint8); ref_p = np.full_like(cur_p, hi)
    allw = windows(orc, w, h, window[0], window[1])
    sbs = (OrcSbSearch * len(pick))(*[allw[i] for i in pick])
    d = sbs[0]
    assert (d.width, d.height) == tuple(window)                      # the clamp left the whole window
    y0, x0 = pad + d.sb_y + d.y_origin, pad + d.sb_x + d.x_origin    # the first record's window region in ref_p: rows y0 .. y0 + height + 62
    n = len(pick)
    sad = np.tile(255 * PU_AREA, (n, 1)).astype(np.uint32)
    mv = np.array([[mv_word(s.x_origin, s.y_origin)] * 85 for s in sbs], np.uint32)
    closed_for = list(range(n))
    if variant == 1:
        ref_p[y0 + d.height - 1:y0 + d.height + 63, x0 + d.width - 1:x0 + d.width + 63] = lo
        closed_for = []
    elif variant == 2:
        ref_p[y0 + d.height - 1 + (62 if sub else 63), x0 + d.width - 1 + 63] = lo
        for pu in PU_LAST:
            sad[0, pu] = 255 * (PU_AREA[pu] - (2 if sub else 1))
            mv[0, pu] = mv_word(d.x_origin + d.width - 1, d.y_origin + d.height - 1)
        closed_for = [0]
    return cur_p, ref_p, cur_p.shape[1], sbs, (sad, mv), closed_for


_saturated_oracle = {}


def saturated_oracle(orc, window, variant, pol, sub, strip=False):
    """the oracle's (sad, mv) of saturated_case, computed once per case (the wave-count variants of the GPU test share it)"""
    key = (tuple(window), variant, pol, sub, strip)
    if key not in _saturated_oracle:
        cur_p, ref_p, stride, sbs, _, _ = saturated_case(orc, window, variant, pol, sub, strip)
        _saturated_oracle[key] = oracle_frame(orc, cur_p, ref_p, stride, synth.PAD, sbs, sub)
    return _saturated_oracle[key]


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# The same for the 16-bit windowed search (sad_loop16_lds_kernel / sad_loop16_generic): block all 0 against a window all mx (1023, 4095) and the mirror image.
# The reference's initial best is 0xffffff; a 12-bit 64 x 64 block gives 0xfff000, 4095 short of it.  (bw, bh, sa_w, sa_h, row_step, odd source column)
SAD16_LDS_SHAPES = [(bw, bh, saw, sah, 1, odd) for (bw, bh) in ((16, 16), (32, 32), (48, 17), (64, 64)) for (saw, sah) in ((8, 1), (64, 64), (24, 40)) for odd in (0, 1)]
SAD16_GENERIC_SHAPES = [(64, 64, 16, 16, 2, 0), (32, 32, 8, 8, 2, 1), (16, 16, 9, 9, 1, 0), (32, 32, 5, 40, 1, 0), (8, 8, 16, 16, 1, 0), (64, 64, 72, 8, 1, 0)]
SAD16_SHAPES = SAD16_LDS_SHAPES + SAD16_GENERIC_SHAPES
SAD16_SW, SAD16_RW = 72, 140                   # plane strides in samples (even: a block at an even column is dword-aligned in every row)


def sad16_takes_lds_form(bw, bh, saw, sah, rs):
    """the shape test of sad_loop16_lds_kernel"""
    return rs == 1 and 16 <= bw <= 64 and bw % 16 == 0 and 1 <= bh <= 64 and 8 <= saw <= 64 and saw % 8 == 0 and 1 <= sah <= 64


def saturated_sad16(mx, pol):
    """-> src, ref (uint16 planes, random outside the jobs' own regions), the SvtHipSadLoop jobs (three variants per shape of SAD16_SHAPES) and their closed
    forms [(sad, x, y)]: 0 nothing planted: mx * bw * rows at (0, 0); 1 a whole matching block at candidate (sa_w - 2, sa_h - 2): 0 there; 2 one matching
    sample that only the last candidate reads: mx * (bw * rows - 1) at (sa_w - 1, sa_h - 1)."""
    rng = np.random.default_rng(16 + mx)
    n = 3 * len(SAD16_SHAPES)
    src = rng.integers(0, mx + 1, (n * 66, SAD16_SW)).astype(np.uint16); ref = rng.integers(0, mx + 1, (n * 137, SAD16_RW)).astype(np.uint16)
    lo, hi = (0, mx) if pol == 0 else (mx, 0)
    jobs, closed = [], []
    for si, (bw, bh, saw, sah, rs, odd) in enumerate(SAD16_SHAPES):
        rows = bh // rs
        for variant in range(3):
            k = 3 * si + variant
            sx, sy, rx, ry = 2 + odd, 66 * k + 1, 1 + k % 4, 137 * k + 2
            assert sx + bw <= SAD16_SW and rx + saw + bw - 1 <= SAD16_RW and bh <= 65 and sah + bh - 1 <= 135
            src[sy:sy + bh, sx:sx + bw] = lo
            win = ref[ry:ry + sah + bh - 1, rx:rx + saw + bw - 1]
            win[:] = hi
            cx, cy = max(saw - 2, 0), max(sah - 2, 0)
            if variant == 1:
                win[cy:cy + bh, cx:cx + bw] = lo
            elif variant == 2:
                win[sah - 1 + (rows - 1) * rs, saw + bw - 2] = lo
            jobs.append(pkg.SadLoop(sx, sy, rx, ry, bw, bh, saw, sah, rs, 0))
            closed.append((mx * bw * rows, 0, 0) if variant == 0 else (0, cx, cy) if variant == 1 else (mx * (bw * rows - 1), saw - 1, sah - 1))
    return src, ref, (pkg.SadLoop * n)(*jobs), closed


def oracle_sad16(orc, src, ref, S):
    n = len(S)
    e_sad, e_xy = np.zeros(n, np.uint32), np.full((n, 2), -7, np.int16)
    orc.orc_sad_loop16_batch(ptr(src), src.shape[1], ptr(ref), ref.shape[1], S, 0, n, ptr(e_sad), ptr(e_xy))
    return e_sad, e_xy
