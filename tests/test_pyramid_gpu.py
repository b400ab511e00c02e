"""GPU parity: HME pyramids (decimation / 2x2 down-sampling), per-SB variance pyramid and the HME
exhaustive search (svt_sad_loop_kernel semantics incl. first-minimum tie break and sub-SAD rows),
HIP through the C ABI vs the oracle.  Mirrors /root/reference/test/SadTest.cc:611-785 (sad_LoopTest)
and compute_mean_test.cc."""
import ctypes as C

import numpy as np
import pytest

from conftest import ptr

pytestmark = pytest.mark.gpu


def test_downsample_and_variance_pyramid(hip, orc):
    rng = np.random.default_rng(2)
    W, H = 448, 256
    img = rng.integers(0, 256, (H + 64, W + 64), dtype=np.uint8)
    img[:64, :64] = 255; img[64:128, :64] = 0
    d_img = hip.to_device(img)
    for step in (2, 4):
        for filt in (0, 1):
            exp = np.zeros((H // step, W // step + 8), np.uint8)
            orc.orc_downsample_2d(ptr(img), img.shape[1], W, H, ptr(exp), exp.shape[1], step, filt)
            d_out = hip.to_device(np.zeros_like(exp))
            hip.check(hip.L.svt_hip_downsample_2d_dev(hip.h, d_img, img.shape[1], W, H, d_out, exp.shape[1], step, filt))
            assert np.array_equal(hip.to_host(d_out, exp.shape, np.uint8), exp), (step, filt)
            hip.free(d_out)
    cols, n = W // 64, (W // 64) * (H // 64)
    for full in (0, 1):
        e_m = np.zeros((n, 85), np.uint8); e_v = np.zeros((n, 85), np.uint16)
        for sb in range(n):
            p = C.c_void_p(img.ctypes.data + (sb // cols) * 64 * img.shape[1] + (sb % cols) * 64)
            orc.orc_variance_pyramid_sb(p, img.shape[1], full, C.c_void_p(e_m.ctypes.data + sb * 85), C.c_void_p(e_v.ctypes.data + sb * 170))
        d_m, d_v = hip.empty(n * 85), hip.empty(n * 170)
        hip.check(hip.L.svt_hip_variance_pyramid_dev(hip.h, d_img, img.shape[1], cols, n, full, d_m, d_v))
        assert np.array_equal(hip.to_host(d_m, (n, 85), np.uint8), e_m) and np.array_equal(hip.to_host(d_v, (n, 85), np.uint16), e_v), full
        hip.free(d_m, d_v)
    hip.free(d_img)


def test_sad_loop_batch(hip, pkg, orc):
    rng = np.random.default_rng(4)
    src = rng.integers(0, 256, (160, 256), dtype=np.uint8); ref = rng.integers(0, 256, (400, 600), dtype=np.uint8)
    ref[0:120, 0:200] = 7; src[0:64, 0:64] = 9            # all candidates tie -> first wins
    cases = [(16, 16, 32, 9, 1), (32, 32, 16, 7, 1), (64, 64, 8, 5, 1), (16, 16, 48, 3, 2), (16, 16, 240, 60, 1), (32, 32, 16, 16, 2),
             (64, 64, 16, 16, 2), (16, 8, 64, 32, 1), (8, 8, 7, 3, 1)]
    n = len(cases) * 4
    S = (pkg.SadLoop * n)()
    e_sad = np.zeros(n, np.uint32); e_xy = np.zeros((n, 2), np.int16)
    for i in range(n):
        bw, bh, saw, sah, rs = cases[i % len(cases)]
        tie = i < 3
        sx, sy = (0, 0) if tie else (int(rng.integers(0, 256 - bw)), int(rng.integers(0, 160 - bh)))
        rx, ry = (0, 0) if tie else (int(rng.integers(0, 600 - bw - saw)), int(rng.integers(0, 400 - bh - sah)))
        S[i] = pkg.SadLoop(sx, sy, rx, ry, bw, bh, saw, sah, rs, 0)
        best = C.c_uint64(0); xc = C.c_int16(-3); yc = C.c_int16(-4)
        orc.orc_sad_loop(C.c_void_p(src.ctypes.data + sy * 256 + sx), 256 * rs, C.c_void_p(ref.ctypes.data + ry * 600 + rx), 600 * rs, bh // rs, bw,
                         C.byref(best), C.byref(xc), C.byref(yc), 600, C.c_int16(saw), C.c_int16(sah))
        e_sad[i] = best.value; e_xy[i] = (xc.value, yc.value)
    d_src, d_ref, d_S = hip.to_device(src), hip.to_device(ref), hip.to_device(np.frombuffer(bytes(S), np.uint8))
    d_sad, d_xy = hip.empty(n * 4), hip.to_device(np.tile(np.array([-3, -4], np.int16), (n, 1)))
    hip.check(hip.L.svt_hip_sad_loop_batch_dev(hip.h, d_src, 256, d_ref, 600, d_S, n, d_sad, d_xy))
    assert np.array_equal(hip.to_host(d_sad, (n,), np.uint32), e_sad)
    assert np.array_equal(hip.to_host(d_xy, (n, 2), np.int16), e_xy)
    hip.free(d_src, d_ref, d_S, d_sad, d_xy)


# (bw, bh, sa_w, sa_h, row_step): every lane-split factor P of sad_loop_fast (1, 2, 4, 8), both LDS stride choices, multi-tile windows, row_step 2;
# the last two put the un-split 32-wide and a 64-row 16-wide block on a full tile (the longest runs between two flushes of the packed partial sums)
SATURATED_SHAPES = [(16, 16, 16, 16, 1), (16, 16, 64, 64, 1), (32, 32, 16, 16, 1), (32, 32, 40, 24, 2), (64, 64, 8, 5, 1), (64, 64, 64, 64, 1),
                    (64, 64, 16, 16, 2), (16, 16, 240, 60, 1), (32, 32, 64, 64, 1), (16, 64, 64, 64, 1)]


def test_sad_loop_saturated(hip, pkg, orc):
    """Source block all 0 against a window all 255 (and the mirror image): every absolute difference is 255, the largest a packed 16-bit partial SAD
    can meet before it is flushed.  Three searches per shape and polarity: nothing planted (all candidates tie at 255 * bw * bh / row_step, the first
    wins), a whole matching block planted in the last tile of the window (unique minimum 0), one matching sample planted where only the last
    candidate sees it (unique minimum one 255 short of saturation)."""
    rng = np.random.default_rng(9)
    SW, RW = 80, 328                                   # plane strides (multiples of 4: the fast path)
    jobs, e_flat = [], []
    src = [rng.integers(0, 256, (len(SATURATED_SHAPES) * 3 * 72, SW), dtype=np.uint8) for _ in range(2)]
    ref = [rng.integers(0, 256, (len(SATURATED_SHAPES) * 3 * 136, RW), dtype=np.uint8) for _ in range(2)]
    for si, (bw, bh, saw, sah, rs) in enumerate(SATURATED_SHAPES):
        rows = bh // rs
        for variant in range(3):
            k = 3 * si + variant
            sx, sy, rx, ry = 3 + k % 5, 72 * k + 2, 1 + k % 7, 136 * k + 3          # byte-misaligned on both sides
            for pol in (0, 1):                          # 0: source 0 / window 255, 1: the mirror image
                lo, hi = (0, 255) if pol == 0 else (255, 0)
                src[pol][sy:sy + bh, sx:sx + bw] = lo
                win = ref[pol][ry:ry + sah + bh - 1, rx:rx + saw + bw - 1]
                win[:] = hi
                if variant == 1:                        # candidate (cx, cy) in the last 64 x 64 tile, not its last one
                    cx, cy = max(saw - 2, 0), max(sah - 2, 0)
                    win[cy:cy + bh, cx:cx + bw] = lo
                elif variant == 2:                      # the window's last sampled sample: only candidate (saw - 1, sah - 1) reads it
                    win[sah - 1 + (rows - 1) * rs, saw + bw - 2] = lo
            jobs.append(pkg.SadLoop(sx, sy, rx, ry, bw, bh, saw, sah, rs, 0))
            e_flat.append((255 * bw * rows, 0, 0) if variant == 0 else (0, cx, cy) if variant == 1 else (255 * (bw * rows - 1), saw - 1, sah - 1))
    n = len(jobs)
    S = (pkg.SadLoop * n)(*jobs)
    d_S = hip.to_device(np.frombuffer(bytes(S), np.uint8))
    for pol in (0, 1):
        e_sad = np.zeros(n, np.uint32); e_xy = np.zeros((n, 2), np.int16)
        for i, j in enumerate(jobs):
            rs = j.row_step
            best = C.c_uint64(0); xc = C.c_int16(-3); yc = C.c_int16(-4)
            orc.orc_sad_loop(C.c_void_p(src[pol].ctypes.data + j.src_y * SW + j.src_x), SW * rs, C.c_void_p(ref[pol].ctypes.data + j.ref_y * RW + j.ref_x),
                             RW * rs, j.bh // rs, j.bw, C.byref(best), C.byref(xc), C.byref(yc), RW, C.c_int16(j.sa_w), C.c_int16(j.sa_h))
            e_sad[i] = best.value; e_xy[i] = (xc.value, yc.value)
        # the oracle is not the only witness: the planted content fixes every result in closed form
        assert e_sad.tolist() == [e[0] for e in e_flat] and e_xy.tolist() == [[e[1], e[2]] for e in e_flat], pol
        d_src, d_ref = hip.to_device(src[pol]), hip.to_device(ref[pol])
        d_sad, d_xy = hip.empty(n * 4), hip.to_device(np.tile(np.array([-3, -4], np.int16), (n, 1)))
        hip.check(hip.L.svt_hip_sad_loop_batch_dev(hip.h, d_src, SW, d_ref, RW, d_S, n, d_sad, d_xy))
        g_sad, g_xy = hip.to_host(d_sad, (n,), np.uint32), hip.to_host(d_xy, (n, 2), np.int16)
        assert np.array_equal(g_sad, e_sad), (pol, [(SATURATED_SHAPES[i // 3], i % 3, int(g_sad[i]), int(e_sad[i])) for i in np.flatnonzero(g_sad != e_sad)[:6]])
        assert np.array_equal(g_xy, e_xy), (pol, [(SATURATED_SHAPES[i // 3], i % 3, g_xy[i].tolist(), e_xy[i].tolist()) for i in np.flatnonzero((g_xy != e_xy).any(axis=1))[:6]])
        hip.free(d_src, d_ref, d_sad, d_xy)
    hip.free(d_S)
