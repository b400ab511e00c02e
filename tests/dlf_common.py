"""Synthetic mode-info grids and edge descriptors for the deblocking tests / bench (SURVEY.md 8(d),
config 3 (iii)): per 64x64 SB a square transform size from {4,8,16,32,64}, skip flag p = 0.3,
filter levels (Y v/h, U, V) = (20, 20, 12, 12)."""
import ctypes as C

import numpy as np

from conftest import load_package, ptr

pkg = load_package()


def make_mode_info(width, height, seed=15, levels=(20, 20, 12, 12), varied=False):
    rng = np.random.default_rng(seed)
    cols, rows = (width + 3) // 4, (height + 3) // 4
    mi = (pkg.DlfModeInfo * (cols * rows))()
    for sy in range(0, rows, 16):
        for sx in range(0, cols, 16):
            tl = int(rng.integers(2, 7))              # tx log2 for this SB
            bl = max(tl, int(rng.integers(2, 7)))     # prediction block >= tx block
            for by in range(sy, min(sy + 16, rows), 1 << (bl - 2)):
                for bx in range(sx, min(sx + 16, cols), 1 << (bl - 2)):
                    skip = 1 if rng.random() < 0.3 else 0
                    lv = levels if not varied else tuple(int(v) for v in rng.integers(0, 64, 4))
                    for y in range(by, min(by + (1 << (bl - 2)), rows)):
                        for x in range(bx, min(bx + (1 << (bl - 2)), cols)):
                            m = mi[y * cols + x]
                            m.tx_w_log2 = m.tx_h_log2 = tl
                            m.uv_tx_w_log2 = m.uv_tx_h_log2 = min(max(tl - 1, 2), 5)
                            m.bw_log2 = m.bh_log2 = bl
                            m.skip_inter = skip
                            m.level[0][0], m.level[0][1] = lv[0], lv[1]
                            m.level[1][0] = m.level[1][1] = lv[2]
                            m.level[2][0] = m.level[2][1] = lv[3]
    return mi, cols, rows


_orc = None


def oracle():
    """oracle/liboracle.so — the checker; the expectations of the deblocking tests come from its restatement of set_lpf_parameters (pinned to the reference's frame loop by
    tests/test_oracle_vs_ref.py::test_deblocking_edges_of_a_frame), never from the product's own builders"""
    global _orc
    if _orc is None:
        import os
        import subprocess
        from conftest import ROOT
        path = os.path.join(ROOT, "oracle", "liboracle.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])
        _orc = C.CDLL(path)
    return _orc


def records(mi, cols, rows):
    """the grid as the 13-byte records both the product's builders and the oracle read"""
    raw = np.frombuffer(mi, np.uint8) if not isinstance(mi, np.ndarray) else mi
    assert raw.size == 13 * cols * rows
    return np.ascontiguousarray(raw.reshape(-1, 13))


def build_edges(mi, cols, rows, plane, pw, ph, filt_w=None, filt_h=None):
    """edge planes of one plane by the ORACLE (orc_dlf_build_edges); filt_w / filt_h: the units the frame loop visits (default: all)"""
    ss = 0 if plane == 0 else 1
    uw, uh = (pw + 3) // 4, (ph + 3) // 4
    ev = np.zeros((uh, uw), np.uint16); eh = np.zeros((uh, uw), np.uint16)
    raw = records(mi, cols, rows)
    oracle().orc_dlf_build_edges(ptr(raw), cols, rows, plane, ss, ss, pw, ph, uw if filt_w is None else filt_w, uh if filt_h is None else filt_h, ptr(ev), ptr(eh))
    return ev, eh


def product_host_edges(mi, cols, rows, plane, pw, ph, filt_w=None, filt_h=None):
    """the same planes by the PRODUCT's host builder (svt_hip_dlf_build_edges[_crop], svt-av1_amd/csrc/svt_hip_host.cpp): what the tests compare with the oracle"""
    ss = 0 if plane == 0 else 1
    uw, uh = (pw + 3) // 4, (ph + 3) // 4
    ev = np.zeros((uh, uw), np.uint16); eh = np.zeros((uh, uw), np.uint16)
    raw = records(mi, cols, rows)
    L = pkg.lib()
    assert L.svt_hip_dlf_build_edges_crop(ptr(raw), cols, rows, plane, ss, ss, pw, ph, uw if filt_w is None else filt_w, uh if filt_h is None else filt_h, ptr(ev), ptr(eh)) == 0
    return ev, eh


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# The reference's own mode-info fields per 4x4 unit (E2 pin): random AV1 partitions of every superblock, a transform depth, inter / intra, skip and a
# prediction mode per block.  BlockSize enum order (Common/Codec/EbDefinitions.h).
BS_DIMS = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64), (64, 128), (128, 64), (128, 128),
           (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]
BS_INDEX = {d: i for i, d in enumerate(BS_DIMS)}


def _partition(rng, x, y, n, out, depth_bias):
    """blocks (x, y, w, h) of a square node of size n, AV1 partition types"""
    kinds = ["none", "split", "horz", "vert"] + (["horz4", "vert4"] if 16 <= n <= 64 else []) + (["horz_a", "vert_a"] if n >= 16 else [])
    if n == 128: kinds = ["none", "split", "split", "horz", "vert"]
    k = kinds[int(rng.integers(0, len(kinds)))] if rng.random() > depth_bias or n <= 8 else "split"
    h2 = n // 2
    if k == "none": out.append((x, y, n, n))
    elif k == "horz": out += [(x, y, n, h2), (x, y + h2, n, h2)]
    elif k == "vert": out += [(x, y, h2, n), (x + h2, y, h2, n)]
    elif k == "horz4": out += [(x, y + i * n // 4, n, n // 4) for i in range(4)]
    elif k == "vert4": out += [(x + i * n // 4, y, n // 4, n) for i in range(4)]
    elif k == "horz_a": out += [(x, y, h2, h2), (x + h2, y, h2, h2), (x, y + h2, n, h2)]
    elif k == "vert_a": out += [(x, y, h2, h2), (x, y + h2, h2, h2), (x + h2, y, h2, n)]
    else:
        if n == 8: out += [(x + dx, y + dy, 4, 4) for dy in (0, 4) for dx in (0, 4)]
        else:
            for dy in (0, h2):
                for dx in (0, h2): _partition(rng, x + dx, y + dy, h2, out, depth_bias * 0.6)


def make_reference_mode_info(rng, w, h, sb_size, p_skip=0.4, p_inter=0.7):
    """-> dict of [h / 4][w / 4] uint8 arrays: sb_type, tx_depth, ref_frame0 (0 = intra, 1..7), skip, mode (intra 0..12, inter 13..24, a few INTRA_MODE_4x4 = 25)"""
    cols, rows = w // 4, h // 4
    f = {k: np.zeros((rows, cols), np.uint8) for k in ("sb_type", "tx_depth", "ref_frame0", "skip", "mode")}
    for sy in range(0, h, sb_size):
        for sx in range(0, w, sb_size):
            blocks = []
            _partition(rng, sx, sy, sb_size, blocks, 0.5)
            for (x, y, bw, bh) in blocks:
                if x >= w or y >= h: continue
                inter = rng.random() < p_inter
                vals = dict(sb_type=BS_INDEX[(bw, bh)], tx_depth=int(rng.integers(0, 3)), ref_frame0=int(rng.integers(1, 8)) if inter else 0,
                            skip=int(rng.random() < p_skip), mode=int(rng.integers(13, 25)) if inter else (25 if rng.random() < 0.05 else int(rng.integers(0, 13))))
                for k, v in vals.items():
                    f[k][y // 4:min(y + bh, h) // 4, x // 4:min(x + bw, w) // 4] = v
    return f


def oracle_edges(orc, f, w, h, lf, pad_right=0, pad_bottom=0, sb_size=64):
    """summary grid (the product's SvtHipDlfModeInfo records, 13 bytes each), the oracle's edge planes [plane] = (edges_v, edges_h) and the level table"""
    cols, rows = w // 4, h // 4
    lfa = np.array(lf, np.int32)
    lvl = np.zeros((3, 2, 8, 2), np.uint8)
    orc.orc_dlf_level_table(ptr(lfa), ptr(lvl))
    summ = np.zeros((rows * cols, 13), np.uint8)
    orc.orc_dlf_mode_info_summary(rows * cols, ptr(f["sb_type"]), ptr(f["tx_depth"]), ptr(f["ref_frame0"]), ptr(f["skip"]), ptr(f["mode"]), ptr(lvl), ptr(summ))
    edges = []
    for plane in range(3):
        ss = int(plane > 0)
        pw, ph = w >> ss, h >> ss
        fw = orc.orc_dlf_filtered_units(w, pad_right, sb_size, ss); fh = orc.orc_dlf_filtered_units(h, pad_bottom, sb_size, ss)
        ev = np.zeros(((ph + 3) // 4, (pw + 3) // 4), np.uint16); eh = np.zeros_like(ev)
        orc.orc_dlf_build_edges(ptr(summ), cols, rows, plane, ss, ss, pw, ph, fw, fh, ptr(ev), ptr(eh))
        edges.append((ev, eh))
    return summ, edges, lvl


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# Inputs of the pixel-domain SSE / SAD / variance reducers at the edges of their forms (block_sse_kernel, block_sse_rows_kernel, plane_sse_kernel, the
# block SAD / variance kernels).  The GPU tests and tests/test_reducers_ref_cpu.py build their inputs from these functions, so what the CPU test proves
# about the inputs holds for the GPU runs.
SSE_LIST_THRESHOLD = 2048      # svt_hip_launch_block_sse: lists of up to this many pairs take the row-sliced form, longer ones one wave per pair
SSE_SMALL_W, SSE_SMALL_H = (1, 4, 7, 8, 33, 64, 128), (1, 4, 5, 16, 128)
SSE_A_SHAPE, SSE_B_SHAPE = (800, 840), (810, 900)
# restoration-unit rectangles as the loop-filter bridge builds them (up to 1.5 x a 256-sample unit, the 8-row stripe offset on top): (a_x, a_y, b_x, b_y, w, h).
# Heights above 256 take the rows form's second trip, widths above 64 its lane loop; 257 / 300 / 33 / 41 are no multiple of a wave's 8 rows; odd columns.
SSE_RECTS = [(17, 200, 40, 150, 384, 392), (401, 3, 333, 500, 320, 257), (455, 300, 601, 100, 70, 300), (839, 400, 0, 0, 1, 300), (3, 700, 811, 9, 65, 33),
             (451, 750, 515, 760, 384, 41)]
SSE_RECT_IDENTICAL = (600, 320, 701, 405, 70, 300)      # b holds a copy of a here: SSE 0
SSE_RECT_SATURATED = (0, 0, 1, 8, 384, 392)             # a all 0, b all max: SSE w * h * max^2 > 2^32 at every depth


def numpy_sse(a, b, pairs):
    """sum (a - b)^2 of every pair in int64: the plain restatement next to the oracle's orc_plane_sse"""
    return np.array([int(((a[ay:ay + h, ax:ax + w].astype(np.int64) - b[by:by + h, bx:bx + w].astype(np.int64)) ** 2).sum()) for (ax, ay, bx, by, w, h) in pairs], np.uint64)


def oracle_sse(a, b, pairs):
    orc = oracle()
    orc.orc_plane_sse.restype = C.c_uint64
    sa, sb = a.shape[1], b.shape[1]
    return np.array([orc.orc_plane_sse(a.itemsize, C.c_void_p(a.ctypes.data + (ay * sa + ax) * a.itemsize), sa, C.c_void_p(b.ctypes.data + (by * sb + bx) * b.itemsize), sb, w, h)
                     for (ax, ay, bx, by, w, h) in pairs], np.uint64)


_sse_cases = {}


def sse_case(bd):
    """-> dict: planes a / b (bd 8: uint8; 10, 12: uint16 holding bd-bit values), and the pair lists of tests/test_distortion_gpu.py with their expected sums
    (`exp_*`, the oracle's, asserted equal to numpy's):
      small       2051 small blocks (just above the threshold, not a multiple of 4: the list form's last workgroup holds three pairs)
      rects       the restoration-unit rectangles + the identical pair + the saturated pair (8 pairs: the rows form)
      long        the rectangles inside the small blocks (2059 pairs: the list form on 150 000-sample blocks)
    Built once per depth and shared; nobody writes to it."""
    if bd in _sse_cases: return _sse_cases[bd]
    rng = np.random.default_rng(220 + bd)
    mx = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    a = rng.integers(0, mx + 1, SSE_A_SHAPE).astype(dt); b = rng.integers(0, mx + 1, SSE_B_SHAPE).astype(dt)
    ax, ay, bx, by, w, h = SSE_RECT_SATURATED
    a[ay:ay + h, ax:ax + w] = 0; b[by:by + h, bx:bx + w] = mx
    ax, ay, bx, by, w, h = SSE_RECT_IDENTICAL
    b[by:by + h, bx:bx + w] = a[ay:ay + h, ax:ax + w]
    small = []
    for i in range(SSE_LIST_THRESHOLD + 3):
        w = SSE_SMALL_W[i % len(SSE_SMALL_W)] if i < 35 else int(rng.choice(SSE_SMALL_W))       # every width x height at least once
        h = SSE_SMALL_H[i // len(SSE_SMALL_W)] if i < 35 else int(rng.choice(SSE_SMALL_H))
        small.append((int(rng.integers(0, a.shape[1] - w + 1)), int(rng.integers(0, a.shape[0] - h + 1)),
                      int(rng.integers(0, b.shape[1] - w + 1)), int(rng.integers(0, b.shape[0] - h + 1)), w, h))
    rects = SSE_RECTS[:3] + [SSE_RECT_IDENTICAL] + SSE_RECTS[3:] + [SSE_RECT_SATURATED]
    long_ = small[:1000] + rects + small[1000:]
    case = dict(bd=bd, max=mx, a=a, b=b, small=small, rects=rects, long=long_, rects_at=1000)
    for name in ("small", "rects", "long"):
        for (ax, ay, bx, by, w, h) in case[name]:      # the kernels check no bounds: the lists must stay inside the planes
            assert 0 <= ax and ax + w <= a.shape[1] and 0 <= ay and ay + h <= a.shape[0] and 0 <= bx and bx + w <= b.shape[1] and 0 <= by and by + h <= b.shape[0]
        exp = oracle_sse(a, b, case[name])
        assert np.array_equal(exp, numpy_sse(a, b, case[name])), name
        case["exp_" + name] = exp
    for v in case.values():
        if isinstance(v, np.ndarray): v.setflags(write=False)
    _sse_cases[bd] = case
    return case


def blk_pairs(pairs):
    """the list as the bytes of an SvtHipBlkPair array"""
    P = (pkg.BlkPair * len(pairs))(*[pkg.BlkPair(*p) for p in pairs])
    return np.frombuffer(bytes(P), np.uint8)


PLANE_SSE_SATURATED_SIZES = ((333, 77), (1030, 17))    # 1030: two column groups of 1024, the second 6 samples wide; 77 / 17 rows: a ragged last group of 8


def saturated_planes(mx, w, h):
    """test_plane_sse's planes (offset origins (3, 2) / (5, 1), random surroundings) with the compared w x h region all 0 in a and all mx in b
    -> a, b, the closed form w * h * mx^2.  A lane of plane_sse_kernel then sums 8 * 4 * mx^2 (2^29 at 12 bits) into its u32 partial."""
    rng = np.random.default_rng(mx + w)
    dt = np.uint8 if mx < 256 else np.uint16
    a = rng.integers(0, mx + 1, (h + 5, w + 9)).astype(dt); b = rng.integers(0, mx + 1, (h + 3, w + 20)).astype(dt)
    a[2:2 + h, 3:3 + w] = 0; b[1:1 + h, 5:5 + w] = mx
    return a, b, w * h * mx * mx


def saturated_block_pair(bd):
    """test_block_sad_and_variance's extra pair: a 128 x 128 block lying wholly on all-max (plane a, 256 x 320) against all-0 (plane b, 256 x 352) content
    -> (rows, columns) of the region in a and in b, the pair, closed forms (sad, variance, sse).  The 10-bit sse is svt_aom_highbd_10_variance's
    ROUND_POWER_OF_TWO(sse, 4)."""
    mx = (1 << bd) - 1
    sse = mx * mx * 16384
    return (slice(128, 256), slice(192, 320)), (slice(128, 256), slice(224, 352)), (192, 128, 224, 128, 128, 128), (mx * 16384, 0, sse if bd == 8 else (sse + 8) >> 4)
