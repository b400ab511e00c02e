"""GPU parity of the RD-side distortion reductions: coefficient-domain residual / prediction distortion and SATD for
lists of transform blocks, pixel-domain SSE for lists of block pairs (8- and 16-bit) vs the oracle (pinned to
svt_full_distortion_kernel32_bits_c, svt_av1_block_error_c, svt_aom_satd_c, svt_aom_sse_c in tests/test_oracle_vs_ref.py)."""
import ctypes as C

import numpy as np
import pytest

from conftest import ptr
import dlf_common as dc

pytestmark = pytest.mark.gpu


def test_coeff_distortion(hip, orc):
    rng = np.random.default_rng(21)
    for n, nblk in ((16, 1000), (64, 333), (1024, 77), (100, 5)):
        c = rng.integers(-(1 << 20), 1 << 20, (nblk, n)).astype(np.int32)
        r = (c + rng.integers(-5000, 5000, (nblk, n))).astype(np.int32)
        c[0] = np.iinfo(np.int32).max // 2; r[0] = -(np.iinfo(np.int32).max // 2)     # 64-bit range of the squares
        exp = np.zeros((nblk, 3), np.uint64); exp0 = np.zeros((nblk, 3), np.uint64)
        for i in range(nblk):
            orc.orc_coeff_distortion(ptr(c[i]), ptr(r[i]), n, ptr(exp[i]))
            orc.orc_coeff_distortion(ptr(c[i]), None, n, ptr(exp0[i]))
        d_c, d_r, d_o = hip.to_device(c), hip.to_device(r), hip.empty(nblk * 24)
        hip.check(hip.L.svt_hip_coeff_distortion_batch_dev(hip.h, d_c, d_r, n, nblk, d_o))
        assert np.array_equal(hip.to_host(d_o, (nblk, 3), np.uint64), exp)
        hip.check(hip.L.svt_hip_coeff_distortion_batch_dev(hip.h, d_c, None, n, nblk, d_o))
        assert np.array_equal(hip.to_host(d_o, (nblk, 3), np.uint64), exp0)
        hip.free(d_c, d_r, d_o)


@pytest.mark.parametrize("bd", [8, 10])
def test_block_sse(hip, pkg, orc, bd):
    rng = np.random.default_rng(22 + bd)
    dt = np.uint8 if bd == 8 else np.uint16
    a = rng.integers(0, 1 << bd, (300, 420)).astype(dt); b = rng.integers(0, 1 << bd, (310, 400)).astype(dt)
    n = 300
    pairs = []
    for i in range(n):
        w = int(rng.choice([4, 8, 16, 32, 64, 128, 7, 33])); h = int(rng.choice([4, 8, 16, 32, 64, 128, 5]))
        pairs.append((int(rng.integers(0, 420 - w)), int(rng.integers(0, 300 - h)), int(rng.integers(0, 400 - w)), int(rng.integers(0, 310 - h)), w, h))
    P = (pkg.BlkPair * n)(*[pkg.BlkPair(*p) for p in pairs])
    orc.orc_plane_sse.restype = C.c_uint64
    exp = np.array([orc.orc_plane_sse(a.itemsize, C.c_void_p(a.ctypes.data + (ay * 420 + ax) * a.itemsize), 420,
                                      C.c_void_p(b.ctypes.data + (by * 400 + bx) * b.itemsize), 400, w, h) for (ax, ay, bx, by, w, h) in pairs], np.uint64)
    d_a, d_b, d_p, d_o = hip.to_device(a), hip.to_device(b), hip.to_device(np.frombuffer(bytes(P), np.uint8)), hip.empty(n * 8)
    hip.check(hip.L.svt_hip_block_sse_batch_dev(hip.h, a.itemsize, d_a, 420, d_b, 400, d_p, n, d_o))
    assert np.array_equal(hip.to_host(d_o, (n,), np.uint64), exp)
    hip.free(d_a, d_b, d_p, d_o)


def _block_sse(hip, d_a, a, d_b, b, pairs):
    """svt_hip_block_sse_batch_dev on `pairs`, the output buffer pre-filled with 0xA5 bytes (a pair's sum must not depend on what the buffer held)"""
    n = len(pairs)
    d_p, d_o = hip.to_device(dc.blk_pairs(pairs)), hip.to_device(np.full(n * 8, 0xA5, np.uint8))
    hip.check(hip.L.svt_hip_block_sse_batch_dev(hip.h, a.itemsize, d_a, a.shape[1], d_b, b.shape[1], d_p, n, d_o))
    got = hip.to_host(d_o, (n,), np.uint64)
    hip.free(d_p, d_o)
    return got


def _mismatch(got, exp, pairs):
    return [(int(i), pairs[i], int(got[i]), int(exp[i])) for i in np.flatnonzero(got != exp)[:6]]


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_block_sse_both_forms(hip, bd):
    """One list of 2051 small blocks through the list form (block_sse_kernel: one wave per pair, a last workgroup of three pairs) and its first 2048
    entries through the rows form (block_sse_rows_kernel); n = 2049 puts a single pair into the last workgroup.  Every run equals the oracle and numpy,
    the shared entries are identical between the forms."""
    c = dc.sse_case(bd)
    T = dc.SSE_LIST_THRESHOLD
    pairs, exp = c["small"], c["exp_small"]
    assert len(pairs) == T + 3
    d_a, d_b = hip.to_device(c["a"]), hip.to_device(c["b"])
    full = _block_sse(hip, d_a, c["a"], d_b, c["b"], pairs)
    rows = _block_sse(hip, d_a, c["a"], d_b, c["b"], pairs[:T])
    one = _block_sse(hip, d_a, c["a"], d_b, c["b"], pairs[:T + 1])
    hip.free(d_a, d_b)
    assert np.array_equal(full[-3:], exp[-3:]), _mismatch(full[-3:], exp[-3:], pairs[-3:])      # the short final workgroup
    assert np.array_equal(full, exp), _mismatch(full, exp, pairs)
    assert np.array_equal(rows, exp[:T]), _mismatch(rows, exp[:T], pairs)
    assert np.array_equal(one, exp[:T + 1]), _mismatch(one, exp[:T + 1], pairs)
    assert np.array_equal(full[:T], rows) and np.array_equal(one[:T], rows)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_block_sse_restoration_rectangles(hip, bd):
    """Restoration-unit rectangles as the loop-filter bridge passes them (up to 384 x 392, odd columns, heights that are no multiple of 8), as a short list
    (rows form: its second trip of 256 rows, widths above 64) and inside a list of 2059 pairs (list form on 150 000-sample blocks).  The identical pair
    reads 0 although the buffer was pre-filled, the all-0 against all-max pair reads w * h * max^2 > 2^32."""
    c = dc.sse_case(bd)
    d_a, d_b = hip.to_device(c["a"]), hip.to_device(c["b"])
    short = _block_sse(hip, d_a, c["a"], d_b, c["b"], c["rects"])
    long_ = _block_sse(hip, d_a, c["a"], d_b, c["b"], c["long"])
    hip.free(d_a, d_b)
    assert np.array_equal(short, c["exp_rects"]), _mismatch(short, c["exp_rects"], c["rects"])
    assert np.array_equal(long_, c["exp_long"]), _mismatch(long_, c["exp_long"], c["long"])
    zi, si = c["rects"].index(dc.SSE_RECT_IDENTICAL), c["rects"].index(dc.SSE_RECT_SATURATED)
    sat = 384 * 392 * c["max"] ** 2
    assert sat > 1 << 32
    for got in (short, long_[c["rects_at"]:c["rects_at"] + len(c["rects"])]):
        assert int(got[zi]) == 0 and int(got[si]) == sat
