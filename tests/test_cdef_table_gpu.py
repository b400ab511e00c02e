"""The CDEF strength search's table form of constrain() on 8-bit planes (svt-av1_amd/csrc/cdef.hip: build_cdef_tables, sec_entry / pri_entry, unpack_sec).

On `uint8_t` planes the search reads a tap's constrained value from tables the workgroup builds in LDS for the launch's damping: every secondary sum (luma and
chroma) and the chroma primary sums; the luma primary sums (strengths adjusted per block) and everything on `uint16_t` planes stay on the packed arithmetic.
The tables fit at every frame-header damping 3..6, so the choice between the two forms is the sample format's alone: the 8-bit cases below run the table form
at every table size (luma half sizes 16, 32, 64, 128; chroma, one less damping, 16, 16, 32, 64), the 16-bit cases the arithmetic form on the same samples.

GPU cases: both distortion tables, `dir` and `var` bit-equal to the oracle.  The CPU-only cases restate the table entries from constrain() and pin the bounds the
kernel's byte / field packing rests on, and the packed accumulate / unpack against the plain sums."""
import numpy as np
import pytest

import cdef_common as cc
import test_cdef_dir0_gpu as d0
import test_cdef_gpu as tcg

gpu = pytest.mark.gpu
VERY_LARGE = cc.VERY_LARGE


def check(hip, orc, src, rec, skip8, bd, damping):
    """one search at one damping against the oracle; returns the GPU's (tables, dir, var)"""
    e_dir, e_var = tcg.expected_dirs(orc, rec[0], bd, skip8)
    exp = cc.orc_search(orc, rec, src, bd, skip8, damping)
    got, g_dir, g_var = tcg.gpu_search_dirs(hip, rec, src, bd, skip8, damping)
    assert np.array_equal(got[0], exp[0]), ("Y", bd, damping, np.argwhere(got[0] != exp[0])[:5])
    assert np.array_equal(got[1], exp[1]), ("UV", bd, damping, np.argwhere(got[1] != exp[1])[:5])
    assert np.array_equal(g_dir, e_dir), ("dir", bd, damping, np.argwhere(g_dir != e_dir)[:5])
    assert np.array_equal(g_var, e_var), ("var", bd, damping, np.argwhere(g_var != e_var)[:5])
    assert exp[0].any() and exp[1].any()
    return got, g_dir, g_var


# ------------------------------------------------------------------------------------------------------------ direction chart, every damping
@gpu
@pytest.mark.parametrize("damping", (3, 4, 5, 6))
@pytest.mark.parametrize("size", ((200, 136), (208, 144)), ids=("200x136", "208x144"))
def test_chart_every_damping(hip, orc, size, damping):
    """Seed 7: tests/test_cdef_chart_cpu.py asserts its directions, flat blocks, adjust_strength levels and ties.  8-bit planes: the table form, one table size
    per damping (the arithmetic form runs in test_16bit_planes_chart on the same chart)."""
    src, rec, skip8 = cc.make_chart_frame(size[0], size[1], 8, cc.CHART_SEED, np.uint8)
    assert rec[0].dtype == np.uint8
    check(hip, orc, src, rec, skip8, 8, damping)


# ------------------------------------------------------------------------------------------------------------ saturated content
def saturated_frame(kind, seed):
    """72 x 72 (2 x 2 filter blocks, the last ones 8 luma / 4 chroma samples wide): every plane a 0 / 255 pattern.  All kinds put both levels into the outermost
    two rows and columns, so that differences of +-255 (the clamp of the table index) and CDEF_VERY_LARGE taps (the zero end entry; out of the max) meet every
    tap position.  The source is the pattern under +-9 of noise, clipped."""
    rng = np.random.default_rng([seed, len(kind)])
    src, rec = [], []
    for pli in range(3):
        n = 72 >> (pli != 0)
        I, J = np.mgrid[0:n, 0:n]
        p = {"chk": (I + J) % 2, "chk2": (I // 2 + J // 2) % 2, "cols": J % 2, "rows": I % 2, "diag2": ((I + J) // 2) % 2, "anti3": ((I - J) // 3) % 2}[kind] * 255
        if pli == 2: p = 255 - p
        for edge in (p[:2], p[-2:], p[:, :2], p[:, -2:]):
            assert edge.min() == 0 and edge.max() == 255
        rec.append(np.ascontiguousarray(p.astype(np.uint8)))
        src.append(np.ascontiguousarray(np.clip(p + rng.integers(-9, 10, p.shape), 0, 255).astype(np.uint8)))
    skip8 = (rng.random((9, 9)) < 0.2).astype(np.uint8)
    skip8[0, :] = skip8[-1, :] = skip8[:, 0] = skip8[:, -1] = 0    # every picture edge is filtered
    return src, rec, skip8


@gpu
@pytest.mark.parametrize("kind", ("chk", "chk2", "cols", "rows", "diag2", "anti3"))
def test_saturated(hip, orc, kind):
    src, rec, skip8 = saturated_frame(kind, seed=17)
    assert rec[0].shape[1] % 64 == 8
    for damping in (3, 4, 5, 6):
        check(hip, orc, src, rec, skip8, 8, damping)


# ------------------------------------------------------------------------------------------------------------ one-direction frames, mixed chroma passes
@gpu
@pytest.mark.parametrize("damping", (4, 6))
@pytest.mark.parametrize("d", (0, 4, 2))
def test_one_direction(hip, orc, d, damping):
    """200 x 136: directions 0 and 4 take the shortcuts (B = A; secB = secA), direction 2 the whole B part"""
    src, rec, skip8 = d0.one_direction_frame(200, 136, 8, np.uint8, d, seed=11)
    o_dir, _ = cc.orc_find_dir_frame(orc, rec[0], 8)
    live = skip8 == 0
    assert (o_dir[live] == d).sum() >= 0.9 * live.sum(), (d, np.bincount(o_dir[live], minlength=8))
    check(hip, orc, src, rec, skip8, 8, damping)


@gpu
@pytest.mark.parametrize("damping", (4, 6))
def test_mixed_chroma_passes(hip, orc, damping):
    """chroma passes that mix directions and skipped blocks (test_cdef_dir0_gpu.mixed_frame; its own test asserts what the passes hold)"""
    src, rec, skip8, _ = d0.mixed_frame(8, np.uint8, seed=13)
    check(hip, orc, src, rec, skip8, 8, damping)


# ------------------------------------------------------------------------------------------------------------ 16-bit planes: the arithmetic instances
@gpu
@pytest.mark.parametrize("bd", (8, 10))
def test_16bit_planes_chart(hip, orc, bd):
    """200 x 136 chart in uint16_t planes: the arithmetic kernels, equal to the oracle and, at depth 8, to the uint8_t (table) run on the same samples"""
    src, rec, skip8 = cc.make_chart_frame(200, 136, bd, cc.CHART_SEED, np.uint16)
    assert rec[0].dtype == np.uint16
    for damping in (4, 6):
        wide = check(hip, orc, src, rec, skip8, bd, damping)
        if bd == 8:
            narrow = check(hip, orc, [p.astype(np.uint8) for p in src], [p.astype(np.uint8) for p in rec], skip8, 8, damping)
            for a, b in zip(wide, narrow):
                assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------ the tables, restated (no GPU)
def msb(n):
    return int(n).bit_length() - 1


def constrain(d, t, damping):
    """Common/Codec/EbCdef.c:86-93"""
    if t == 0:
        return 0
    a = abs(d)
    v = min(a, max(0, t - (a >> max(0, damping - msb(t)))))
    return -v if d < 0 else v


def tab_half(damping):
    return 256 if damping >= 7 else 16 if damping <= 3 else 2 << damping


def pri_weight(k, t):
    return 3 if t & 1 else (4, 2)[k]


def build_tables(damping):
    """(S [2n + 1] dwords, P [2][2n + 1][16] bytes) as cdef.hip's build_cdef_tables lays them out; entry e holds d = e - n"""
    n = tab_half(damping)
    S = np.zeros(2 * n + 1, np.uint32); P = np.zeros((2, 2 * n + 1, 16), np.uint8)
    for e in range(2 * n + 1):
        d = e - n
        inside = abs(d) < n
        c1, c2, c4 = (constrain(d, t, damping) if inside else 0 for t in (1, 2, 4))
        S[e] = (4 + c2) | (4 + c1) << 8 | (4 + c4) << 16
        for k in range(2):
            for t in range(16):
                P[k, e, t] = 64 + pri_weight(k, t) * (constrain(d, t, damping) if inside else 0)
    return n, S, P


DAMPINGS = (2, 3, 4, 5, 6)   # luma 3..6, chroma one less


@pytest.mark.parametrize("damping", DAMPINGS)
def test_table_entries_vanish_outside(damping):
    """constrain(d, t, D) is zero for |d| >= t << max(0, D - msb(t)): for every t <= 15 that is below 2^(D+1) when D >= 3.  At D = 2 (chroma at the lowest header
    damping) the strengths 9..15 are not shifted at all and reach up to |d| = 14 > 2^3, which is why the table's half size is max(16, 2^(D+1))."""
    n = tab_half(damping)
    assert n == max(16, 2 << damping)
    for t in list(range(16)):
        for a in range(n - 1, 256):          # n - 1 as well: the builder's `|d| < n` keeps no non-zero value out
            assert constrain(a, t, damping) == 0 and constrain(-a, t, damping) == 0, (damping, t, a)
    for t in (1, 2, 4):                       # the secondary strengths vanish from 2^(D+1) at every damping
        for a in range(2 << damping, 256):
            assert constrain(a, t, damping) == 0
    if damping >= 3:
        assert all(constrain(a, t, damping) == 0 for t in range(16) for a in range(2 << damping, 256))
    else:
        assert constrain(14, 15, 2) == 1 and constrain(8, 15, 2) == 7    # the counter-example to "zero from 2^(D+1)" at D = 2


@pytest.mark.parametrize("damping", DAMPINGS)
def test_table_sums_are_carry_free(damping):
    n, S, P = build_tables(damping)
    for e in (0, 2 * n):                      # the end entries: the clamp's targets, CDEF_VERY_LARGE taps among them
        assert S[e] == 0x00040404 and (P[:, e] == 64).all()
    # primary: a byte is 64 +- w * c with |w * c| <= 4 * 14; the two mirrored taps of one distance share an accumulator byte
    for k in range(2):
        for t in range(16):
            col = P[k, :, t].astype(np.int64)
            assert 8 <= col.min() and col.max() <= 120, (damping, k, t, col.min(), col.max())
            assert 2 * col.max() <= 255 and abs(col - 64).max() <= pri_weight(k, t) * t
    # secondary: fields 4 +- c in 0..8; four taps of distance 0 count twice (2 * acc0 + acc1), four of distance 1 once: 48 +- 48
    for sh, t in ((8, 1), (0, 2), (16, 4)):
        f = ((S >> sh) & 0xFF).astype(np.int64)
        assert (S >> 24 == 0).all() and 4 - t <= f.min() and f.max() <= 4 + t
        assert 2 * 4 * f.max() + 4 * f.max() <= 96 <= 255 and 2 * 4 * f.min() + 4 * f.min() >= 0


@pytest.mark.parametrize("damping", DAMPINGS)
def test_packed_sums_equal_plain_sums(damping):
    """the kernel's index rule, dword accumulation and unpacking against sum(w * constrain): random 8-bit taps, +-255 differences, CDEF_VERY_LARGE taps"""
    n, S, P = build_tables(damping)
    P32 = P.view(np.uint32)                  # [2][2n + 1][4] little-endian dwords, as the kernel adds them
    rng = np.random.default_rng(damping)
    for trial in range(400):
        x = int(rng.choice((0, 255, int(rng.integers(0, 256)))))
        spread = int(rng.choice((3, 20, 255)))
        taps = np.clip(x + rng.integers(-spread, spread + 1, 12), 0, 255)
        taps[rng.random(12) < 0.15] = VERY_LARGE
        if trial % 7 == 0: taps[:] = 255 - x if x in (0, 255) else taps
        idx = np.minimum((taps + (n - x)).astype(np.int64) & 0xFFFFFFFF, 2 * n)          # unsigned wrap of a negative sum, then the clamp
        diff = [0 if v == VERY_LARGE else int(v) - x for v in taps]                       # EbCdef.c:87-93 returns 0 for such a tap: its shifted |d| exceeds every t
        # secondary: taps 0..3 distance 0 (weight 2), 4..7 distance 1 (weight 1)
        acc0 = int(S[idx[0:4]].sum()) & 0xFFFFFFFF; acc1 = int(S[idx[4:8]].sum()) & 0xFFFFFFFF
        tot = (2 * acc0 + acc1) & 0xFFFFFFFF
        got = {1: ((tot >> 8) & 0xFF) - 48, 2: (tot & 0xFF) - 48, 4: ((tot >> 16) & 0xFF) - 48}
        for t in (1, 2, 4):
            assert got[t] == sum(2 * constrain(d, t, damping) for d in diff[0:4]) + sum(constrain(d, t, damping) for d in diff[4:8]), (damping, t, x, taps)
        # primary: taps 8, 9 distance 0, taps 10, 11 distance 1
        a0 = (P32[0, idx[8]].astype(np.uint64) + P32[0, idx[9]]) & 0xFFFFFFFF; a1 = (P32[1, idx[10]].astype(np.uint64) + P32[1, idx[11]]) & 0xFFFFFFFF
        for t in range(16):
            s = ((int(a0[t >> 2]) >> (8 * (t & 3))) & 0xFF) + ((int(a1[t >> 2]) >> (8 * (t & 3))) & 0xFF) - 256
            want = sum(pri_weight(0, t) * constrain(d, t, damping) for d in diff[8:10]) + sum(pri_weight(1, t) * constrain(d, t, damping) for d in diff[10:12])
            assert s == want, (damping, t, x, taps)
