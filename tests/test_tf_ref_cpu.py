"""CPU side of the temporal-filter pins (tests/test_tf_gpu.py: test_filter_edge_cases, test_filter_slow_division_instance, test_estimate_noise_edges,
test_subpel_edge_cases): builds every case of tf_common, checks the oracle against the plain restatements there (numpy_filter, numpy_noise, python_subpel), asserts
the closed forms, and asserts that each case contains what the GPU tests say they cover.  Needs no GPU.  The comparisons with the compiled reference at the end
run where oracle/_ref has been built."""
import ctypes as C

import numpy as np
import pytest

from conftest import ptr
import tf_common as T

FILTER_IDS = [T.fmt_id(f) for f in T.FILTER_FMTS]


def planes_equal(case, bufs, arrays):
    return all(np.array_equal(case.view(bufs, p), arrays[p]) for p in range(case.planes()))


def padding_intact(case, bufs):
    return all((bufs[p][:, case.dims[p][1]:] == T.sentinel(case.dt)).all() for p in range(3))


# what the oracle alone produces on each content (read off on the CPU; the same for every format to within the figures below, which are the smallest seen): the number of
# distinct weights strictly between 0 and 1000
WEIGHTS_BETWEEN = {"max_vs_0": 300, "0_vs_max": 487, "checker": 183, "binary": 245, "border": 916, "luma_only": 553, "border_420": 434, "two_columns": 452}


@pytest.mark.parametrize("fmt", T.FILTER_FMTS, ids=FILTER_IDS)
def test_filter_cases_oracle_is_the_restatement(orc, fmt):
    """orc_tf_filter_frame == numpy_filter on every case (planes and both SSE words), out of place and in place; strides all different and the padding untouched; the
    block records hold both split values, the extreme vectors and errors; every content reaches weights 0 and 1000 and a stated number of values between"""
    names = set()
    for c in T.filter_edge_cases(fmt):
        names.add(c.name)
        weights = [set(), set(), set()]
        out, sse = T.numpy_filter(c, weights)
        dst, o_sse = c.oracle(orc)
        assert planes_equal(c, dst, out) and np.array_equal(o_sse, sse), (c.name, o_sse, sse)
        assert padding_intact(c, dst)
        inp, i_sse = c.oracle(orc, in_place=True)
        assert planes_equal(c, inp, out) and np.array_equal(i_sse, sse) and padding_intact(c, inp)
        assert any((c.view(dst, p) != c.view(c.src, p)).any() for p in range(c.planes())) and sse[0] > 0
        seen = set().union(*weights)
        between = len(seen - {0, 1000})
        print(T.fmt_id(fmt), c.name, "weights between 0 and 1000:", between)
        assert 0 in seen and 1000 in seen and between >= WEIGHTS_BETWEEN[c.name], (c.name, between)
        b = np.concatenate(c.blocks)
        assert set(np.unique(b["split"])) == {0, 1}
        assert {0, 1, 15, 1 << 40, 1 << 63} <= set(int(v) for v in np.unique(b["err16"]))
        mv = set(zip(b["mv16_x"].ravel().tolist(), b["mv16_y"].ravel().tolist())) | set(zip(b["mv32_x"].ravel().tolist(), b["mv32_y"].ravel().tolist()))
        assert {(0, 0), (32767, 32767), (32767, -32767), (-32767, 32767), (-32768, -32768)} <= mv
        assert len(c.preds) + 1 <= 4
    assert names == set(WEIGHTS_BETWEEN)
    cs = T.filter_edge_cases(fmt)
    assert {(c.ss_x, c.ss_y) for c in cs} == {(1, 1), (1, 0), (0, 0)} and {c.tf_chroma for c in cs} == {0, 1} and {c.decay for c in cs} == {1, 4}
    assert {c.mfs for c in cs} == {1, 64, 2160} and {c.w for c in cs} == {64, 128}
    assert T.launch_constants((1, 1, 1), 4, 1)[1] == 1.0            # min_frame_size 1: the threshold is clamped to 1


def test_filter_contents_hold_what_they_say():
    for fmt in ((np.uint8, 8), (np.uint16, 12)):
        mx = (1 << fmt[1]) - 1
        cs = {c.name: c for c in T.filter_edge_cases(fmt)}
        s, p = cs["max_vs_0"].view(cs["max_vs_0"].src, 0), cs["max_vs_0"].view(cs["max_vs_0"].preds[0], 0)
        assert (s == mx).all() and (p == 0).all()
        s, p = cs["0_vs_max"].view(cs["0_vs_max"].src, 2), cs["0_vs_max"].view(cs["0_vs_max"].preds[0], 2)
        assert (s == 0).all() and (p == mx).all()
        c = cs["checker"]; s, p = c.view(c.src, 0).astype(int), c.view(c.preds[0], 0).astype(int)
        assert (s + p == mx).all() and (s[::2, ::2] == 0).all() and (s[::2, 1::2] == mx).all() and (s[1::2, ::2] == mx).all()
        c = cs["binary"]; assert set(np.unique(c.view(c.src, 0))) == {0, mx} == set(np.unique(c.view(c.preds[0], 0)))
        for name in ("border", "border_420"):
            c = cs[name]
            for pl in range(3):
                d = c.view(c.src, pl).astype(int) != c.view(c.preds[0], pl).astype(int)
                ch, cw = 32 >> (c.ss_y if pl else 0), 32 >> (c.ss_x if pl else 0)
                for y0 in range(0, d.shape[0], ch):
                    for x0 in range(0, d.shape[1], cw):
                        blk = d[y0:y0 + ch, x0:x0 + cw]
                        assert not blk[2:-2, 2:-2].any() and blk[:2].any() and blk[-2:].any() and blk[:, :2].any() and blk[:, -2:].any()
        c = cs["luma_only"]
        assert (c.view(c.src, 0) != c.view(c.preds[0], 0)).any() and all(np.array_equal(c.view(c.src, p), c.view(c.preds[0], p)) for p in (1, 2))
        # ... and the chroma weights of that predictor still move: they are not all 1000
        w = [set(), set(), set()]
        only = T.FilterCase("x", "luma_only", fmt[0], fmt[1], 64, 64, (1, 0), 1, 1, 64, 0, seed=15, window=("content",))
        only.blocks[0][:] = np.zeros(1, T.BLK_DTYPE)[0]
        T.numpy_filter(only, w)
        assert len(w[1]) > 5 and len(w[2]) > 5
    # 12 bits: the largest chroma window sum, 29 samples of 4095^2, needs more than 28 bits and fits 32
    assert 1 << 28 < 29 * 4095 ** 2 == 486301725 < 1 << 32


def test_filter_widening_holds_with_errors_pre_shifted(orc):
    """the (u16, 8) result is the widened (u8, 8) result once the 8-bit run is given the block errors already divided by 16 (the 16-bit function shifts them at any depth)"""
    for c16, c8 in zip(T.filter_edge_cases((np.uint16, 8)), T.filter_edge_cases((np.uint8, 8))):
        assert all(np.array_equal(c16.view(c16.src, p), c8.view(c8.src, p)) for p in range(3))
        for b in c8.blocks:
            b["err16"] >>= np.uint64(4); b["err32"] >>= np.uint64(4)
        d16, s16 = c16.oracle(orc); d8, s8 = c8.oracle(orc)
        assert all(np.array_equal(c16.view(d16, p), c8.view(d8, p)) for p in range(c16.planes())) and np.array_equal(s16, s8), c16.name


def test_recip_ok_restated():
    assert T.recip_ok(1.0) and T.recip_ok(2 * (4 * (0.7 + np.log1p(1.7))) ** 2) and T.recip_ok(216.0)
    assert not T.recip_ok(float("inf")) and not T.recip_ok(-1.0) and not T.recip_ok(0.0) and not T.recip_ok(float("nan"))
    assert not T.recip_ok(np.nextafter(2.0, 0.0)) and T.recip_ok(np.nextafter(np.nextafter(2.0, 0.0), 0.0))       # all-ones significand
    assert not T.recip_ok(2.0 ** -501) and T.recip_ok(2.0 ** -499) and not T.recip_ok(2.0 ** 501) and T.recip_ok(2.0 ** 499)


@pytest.mark.parametrize("fmt", T.FILTER_FMTS, ids=FILTER_IDS)
def test_slow_division_case(orc, fmt):
    """V noise -1: den[2] = +inf, the only launch constant recip_ok refuses; the oracle handles it without undefined behaviour (x / inf = 0, expf(-0) * 1000 = 1000), so V is the
    rounded mean of the window; Y and U are what the ordinary-noise twin gives"""
    c, twin = T.slow_division_case(fmt), T.slow_division_case(fmt, v_noise=2.4)
    den, thr = T.launch_constants(c.noise, c.decay, c.mfs)
    assert den[2] == float("inf") and [T.recip_ok(v) for v in den + [thr]] == [True, True, False, True]
    assert all(T.recip_ok(v) for v in T.launch_constants(twin.noise, twin.decay, twin.mfs)[0])
    w = [set(), set(), set()]
    out, sse = T.numpy_filter(c, w)
    dst, o_sse = c.oracle(orc)
    assert planes_equal(c, dst, out) and np.array_equal(o_sse, sse) and padding_intact(c, dst)
    assert w[2] == {1000} and len(w[0]) > 40 and len(w[1]) > 40
    mean = T.rounded_mean_of_window(c, 2)
    assert np.array_equal(out[2], mean) and (mean != c.view(c.src, 2)).any()
    t_dst, _ = twin.oracle(orc)
    assert all(np.array_equal(c.view(dst, p), c.view(t_dst, p)) for p in (0, 1)) and not np.array_equal(c.view(dst, 2), c.view(t_dst, 2))


# ------------------------------------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("fmt", T.NOISE_FMTS, ids=[T.fmt_id(f) for f in T.NOISE_FMTS])
def test_noise_cases(orc, fmt):
    orc.orc_tf_estimate_noise.restype = C.c_double
    dt, bd = fmt
    sh = bd - 8 if np.dtype(dt).itemsize == 2 else 0
    got = {}
    for name, buf, w, h, closed in T.noise_edge_cases(fmt):
        assert buf.shape[1] > w and buf.shape[0] == h
        out = np.full(2, -7, np.int64)
        sigma = orc.orc_tf_estimate_noise(ptr(buf), buf.itemsize, bd, w, h, buf.shape[1], ptr(out))
        s, n = T.numpy_noise(buf[:, :w], bd)
        assert (int(out[0]), int(out[1])) == (s, n), (name, out, s, n)
        if closed is not None: assert (s, n) == closed, (name, s, n, closed)
        assert sigma == T.sigma_of(s, n)
        got[name] = (s, n, sigma)
    assert got["rows_past_2048"][1] > 16 and 2100 - 2 > 2048
    # ... and the rows past the first 2048 change the result: a loop without the grid stride would miss them
    name, buf, w, h, _ = T.noise_edge_cases(fmt)[0]
    assert T.numpy_noise(buf[:2050, :w], bd) != got["rows_past_2048"][:2]
    for k in ("2x2", "2x40", "40x2"): assert got[k] == (0, 0, -1.0)
    assert got["3x3"][1] <= 1 and got["3x3"][2] == -1.0
    assert got["flat_17x3"] == (0, 15, -1.0) and got["flat_18x3"] == (0, 16, 0.0)
    assert got["259x5"][1] > 256 * 3 and got["261x5"][1] > 256 * 3            # the column loop's second trip contributes (one and three live lanes)
    assert got["ga_smooth"][1] == 1 and got["ga_edge"][1] == 0
    lo, hi = T.ga_pair(bd, dt)
    rnd = (1 << sh) >> 1
    assert ((2 * lo + rnd) >> sh, (2 * hi + rnd) >> sh) == ((49, 50) if sh else (48, 50))
    assert got["checker"][:2] == ({8: 2040, 10: 2046, 12: 2048}[bd] * 35 * 19, 35 * 19)     # smooth by the Sobel test, Laplacian 8 max per sample


def test_gradient_magnitude_is_even():
    """|gx| + |gy| has the parity of gx + gy = 2 (a - k) + 2 (d - f) + 2 (b - h): the raw magnitudes 49, 197 and 791 cannot occur, which is why the threshold cases
    stand at 48 / 50, 196 / 198 and 790 / 792"""
    rng = np.random.default_rng(0)
    p = rng.integers(0, 4096, (4096, 3, 3))
    a, b, c, d, f, g, h, k = p[:, 0, 0], p[:, 0, 1], p[:, 0, 2], p[:, 1, 0], p[:, 1, 2], p[:, 2, 0], p[:, 2, 1], p[:, 2, 2]
    gx = (a - c) + (g - k) + 2 * (d - f); gy = (a - g) + (c - k) + 2 * (b - h)
    assert ((np.abs(gx) + np.abs(gy)) % 2 == 0).all()


def test_noise_widening(orc):
    for (n16, b16, w, h, _), (n8, b8, _, _, _) in zip(T.noise_edge_cases((np.uint16, 8)), T.noise_edge_cases((np.uint8, 8))):
        assert n16 == n8 and np.array_equal(b16[:, :w], b8[:, :w])
        assert T.numpy_noise(b16[:, :w], 8) == T.numpy_noise(b8[:, :w], 8)


# ------------------------------------------------------------------------------------------------------------------------ sub-pel
def test_variance_closed_forms():
    """flat 0 against flat max: 2^30 / 2^28 at (u16, 10), 2^26 / 2^24 at (u16, 8), 0 at (u8, 8) -- the 16-bit form at depth 8 is not the widened 8-bit form"""
    for (pb, bd), (d32, d16) in T.FLAT_DIST.items():
        mx = (1 << bd) - 1
        for n, want in ((1024, d32), (256, d16)):
            for sign in (1, -1):
                sse, s = n * mx * mx, sign * n * mx
                assert (T.variance_u8(sse, s, n) if pb == 1 else T.variance_u16(sse, s, n)) == want
                assert T.variance_u16(sse, s, n, wide=True) == 0
    assert 46341 ** 2 > 1 << 31 > 46340 ** 2                       # where `sum * sum` first wraps
    # the split decision: err32 = 2^30 with four err16 = 0 is no split when wrapped and split in 64 bits; products overflow from 143 165 577
    assert T.split_flag(1 << 30, [0] * 4) == 0 and T.split_flag(1 << 30, [0] * 4, wide=True) == 1
    assert 143165577 * 15 > (1 << 31) - 1 >= 143165576 * 15


SUBPEL_IDS = [T.fmt_id(f) for f in T.SUBPEL_FMTS]
BLK_FIELDS = ("mv32_x", "mv32_y", "err32", "split", "mv16_x", "mv16_y", "err16")


def same_blocks(a, b):
    return all(np.array_equal(a[k], b[k]) for k in BLK_FIELDS)


@pytest.mark.parametrize("fmt", T.SUBPEL_FMTS, ids=SUBPEL_IDS)
def test_subpel_cases(orc, fmt):
    """orc_tf_subpel_frame == python_subpel on every case (every field of every record, untouched ones included, and the predictor planes whole), and the cases hold
    what they are there for"""
    dt, bd = fmt
    pb = np.dtype(dt).itemsize
    cases = T.subpel_edge_cases(fmt)
    probes = {}
    for name, c in cases.items():
        probes[name] = pr = {}
        blk, pred = T.python_subpel(orc, c, pr)
        o_blk, o_pred = c.oracle(orc)
        assert same_blocks(blk, o_blk), name
        assert all(np.array_equal(a, b) for a, b in zip(pred, o_pred)), name
        used = set(int(i) for i in c.jobs["blk_index"])
        for i in range(c.n_blocks):
            if i not in used: assert o_blk[i].tobytes() == bytes([0x5A]) * 256
        assert len(used) < c.n_blocks
        for p in range(3 if c.tf_chroma else 1):                    # only the job's blocks are written, at the crop's origin
            ox, oy = c.org[p]
            hh, ww = c.h >> (p > 0), c.w >> (p > 0)
            touched = o_pred[p] != T.sentinel(dt)
            outside = touched.copy(); outside[oy:oy + hh, ox:ox + ww] = False
            assert not outside.any() and touched[oy:oy + hh, ox:ox + ww].mean() > 0.9
        assert (c.jobs["dst_x"] != c.jobs["x"]).all() and (c.jobs["dst_y"] != c.jobs["y"]).all() and (c.jobs["dst_x"] != c.jobs["dst_y"]).all()
        if not c.tf_chroma: assert all((o_pred[p] == T.sentinel(dt)).all() for p in (1, 2))
    # ---- ties: nine equal distortions in round 0 of every search, the closed-form distortions and vectors
    for name in ("flat_0_vs_max", "flat_max_vs_0", "flat_0_vs_max_hp0", "flat_max_vs_0_hp0"):
        c, pr = cases[name], probes[name]
        blk, _ = c.oracle(orc)
        e = c.expect
        assert len(pr["round0"]) == 20 * len(c.jobs) and all(len(set(d)) == 1 and len(d) == 9 for _, _, d in pr["round0"])
        assert pr["dist_wide"] == (pb == 2)                        # 64-bit `sum * sum` would change the 16-bit distortions
        T.check_tie_closed_forms(c, blk)
    assert {cases[n].tf_hp for n in ("flat_0_vs_max", "flat_0_vs_max_hp0")} == {0, 1}
    # ---- every row the same: ties in columns of three, columns differ, the winner is the first of its column
    pr = probes["rows_equal"]
    for bs, tag, d in pr["round0"]:
        cols = [d[0:3], d[3:6], d[6:9]]
        assert all(len(set(col)) == 1 for col in cols) and len({col[0] for col in cols}) == 3, (bs, tag, d)
    c = cases["rows_equal"]
    blk, _ = c.oracle(orc)
    B = blk[int(c.jobs["blk_index"][0])]
    for q in range(4):      # the winner of a round is the first candidate of its column: the vertical offset only ever moves up, by -4 and then by -2 and -1 where a later column wins
        assert int(B["mv32_y"][q]) - T.i16(T.i16(int(c.jobs["mv32"][0][q]) >> 16) * 2) in (-4, -5, -6, -7)
    # ---- overshoot: both clamps of all three filtered branches bind (the fourth branch, the full-sample copy, has none)
    assert all(v == [True, True] for v in probes["overshoot"]["clamps"].values()), probes["overshoot"]["clamps"]
    assert probes["overshoot"]["im_max"] > (1 << (bd + 4))
    # ---- the split decision's wrap
    sp = probes["split_wrap"]["split"]
    e32, e16, wrapped, wide = sp[0]
    assert e32 == T.FLAT_DIST[(pb, bd)][0] and e16 == [0, 0, 0, 0]
    if bd == 10: assert (wrapped, wide) == (0, 1) and e32 == 1 << 30
    else: assert wrapped == wide == 1                              # below bit depth 10 the products cannot overflow: the wrap case pins bit depth 10 only
    # ---- the int16 edges
    c = cases["int16_edge"]
    halves = {T.i16(int(w) & 0xffff) for w in c.jobs["mv32"][0]} | {T.i16(int(w) >> 16) for w in c.jobs["mv32"][0]}
    assert {16383, -16383, -16384} <= halves
    blk, _ = c.oracle(orc)
    B = blk[int(c.jobs["blk_index"][0])]
    assert max(abs(int(v)) for v in list(B["mv32_x"]) + list(B["mv32_y"])) >= 32762


@pytest.mark.parametrize("fmt", T.SUBPEL_FMTS, ids=SUBPEL_IDS)
def test_subpel_threshold_equality(orc, fmt):
    c = T.subpel_edge_cases(fmt)["texture"]
    outs = T.threshold_equality_runs(lambda k: k.oracle(orc)[0], c)
    pys = T.threshold_equality_runs(lambda k: T.python_subpel(orc, k)[0], c)
    assert all(same_blocks(a, b) for a, b in zip(outs, pys))


def test_named_mistakes_show_on_the_cases(orc):
    """the mistakes the GPU tests are there to catch, made in the CPU restatements: each changes the result of the case that is named for it.  (64-bit variance
    arithmetic and a 64-bit split decision: the probes of test_subpel_cases; a row loop without the grid stride: test_noise_cases.)"""
    for fmt in T.SUBPEL_FMTS:
        cases = T.subpel_edge_cases(fmt)
        for name in ("flat_0_vs_max", "flat_max_vs_0_hp0", "rows_equal"):     # `<=` in the candidate scan: the last of the tied candidates wins
            blk, pred = T.python_subpel(orc, cases[name], mutate=("scan_le",))
            o_blk, _ = cases[name].oracle(orc)
            assert not np.array_equal(blk["mv32_x"], o_blk["mv32_x"]) or not np.array_equal(blk["mv32_y"], o_blk["mv32_y"]), name
        c = cases["texture"]                                                     # `err32 <= th16`
        base, _ = c.oracle(orc)
        e = int(np.sort(base[int(c.jobs["blk_index"][0])]["err32"])[2])
        blk, _ = T.python_subpel(orc, c.with_th16(e), mutate=("th_le",))
        assert not same_blocks(blk, c.with_th16(e).oracle(orc)[0])
    for fmt in T.NOISE_FMTS:                                                     # `ga <= 50`
        for name, buf, w, h, closed in T.noise_edge_cases(fmt):
            if name in ("ga_edge", "ga_strip"):
                assert T.numpy_noise(buf[:, :w], fmt[1], smooth=lambda ga: ga <= 50) != T.numpy_noise(buf[:, :w], fmt[1]), name
            if name == "ga_smooth":
                assert T.numpy_noise(buf[:, :w], fmt[1], smooth=lambda ga: ga < 48) != T.numpy_noise(buf[:, :w], fmt[1])


# ------------------------------------------------------------------------------------------------------------------------ against the compiled reference
def test_variance_forms_against_reference(ref):
    """the restatement's two variance forms == svt_aom_variance32x32_c / 16x16_c and variance_highbd_c of the compiled reference on the saturated blocks"""
    ref.variance_highbd_c.restype = C.c_uint32
    for fn in ("svt_aom_variance32x32_c", "svt_aom_variance16x16_c"): getattr(ref, fn).restype = C.c_uint32
    rng = np.random.default_rng(5)
    for bs in (32, 16):
        n = bs * bs
        for bd in (8, 10):
            mx = (1 << bd) - 1
            for a_v, b_v in ((0, mx), (mx, 0), (None, None)):
                a = np.full((bs, bs + 3), a_v, np.uint16) if a_v is not None else (rng.integers(0, 2, (bs, bs + 3)) * mx).astype(np.uint16)
                b = np.full((bs, bs + 5), b_v, np.uint16) if b_v is not None else (rng.integers(0, 8, (bs, bs + 5)) * (mx // 8)).astype(np.uint16)
                d = a[:, :bs].astype(np.int64) - b[:, :bs]
                sse_out = C.c_uint32(0)
                got = ref.variance_highbd_c(ptr(a), bs + 3, ptr(b), bs + 5, bs, bs, C.byref(sse_out))
                assert got == T.variance_u16(int((d * d).sum()), int(d.sum()), n), (bs, bd, a_v)
                if bd == 8:
                    a8, b8 = np.ascontiguousarray(a.astype(np.uint8)), np.ascontiguousarray(b.astype(np.uint8))
                    got8 = getattr(ref, "svt_aom_variance%dx%d_c" % (bs, bs))(ptr(a8), bs + 3, ptr(b8), bs + 5, C.byref(sse_out))
                    assert got8 == T.variance_u8(int((d * d).sum()), int(d.sum()), n)
