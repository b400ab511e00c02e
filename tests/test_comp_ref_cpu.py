"""CPU proof of the case lists of tests/comp_common.py (compound, blend, OBMC, warp, compound warp) that tests/test_compound_gpu.py launches:
what every list contains (exact counts of the combinations it exists for), that the oracle equals a plain int64 numpy restatement on every record, the closed
forms, and that each of five deliberately wrong numpy variants changes a result somewhere on its list."""
from collections import Counter

import numpy as np
import pytest

from conftest import ptr
import comp_common as cmc

FMTS = [pytest.param(8, None, id="8"), pytest.param(10, None, id="10"), pytest.param(12, None, id="12"), pytest.param(8, np.uint16, id="u16-8")]


# ---------------------------------------------------------------- coverage
def test_compound_list_is_the_full_product():
    c = cmc.compound_cases(8)
    d = c.desc
    assert len(d) == 1408 == len({(x["size"], x["type"], x["f0"], x["f1"]) for x in d})
    assert len({(x["size"], x["type"]) for x in d}) == 88
    for t in range(4): assert len({(x["f0"], x["f1"]) for x in d if x["type"] == t}) == 16
    for s in cmc.SIZES: assert len({(x["f0"], x["f1"]) for x in d if x["size"] == s}) == 16
    assert len({(x["type"], x["f0"], x["f1"]) for x in d}) == 64 and len({(x["size"], x["f0"], x["f1"]) for x in d}) == 22 * 16
    # every (bank, phase) as an x filter and as a y filter: 96 pairs per direction, the 90 with a non-zero phase among them
    for axis in (0, 1):
        pairs = {(x["banks"][axis], x["subpel"][2 * r + axis]) for x in d for r in (0, 1)}
        assert len(pairs) == 96 and len({p for p in pairs if p[1]}) == 90, axis
        for r in (0, 1): assert len({(x["banks"][axis], x["subpel"][2 * r + axis]) for x in d}) == 96, (axis, r)      # ... and for either reference alone
    assert any(x["banks"][0] != x["banks"][1] and x["f0"] == 3 and x["f1"] == 3 for x in d)
    # the cycling properties
    assert {x["dist"] for x in d if x["type"] == 1} == set(cmc.DIST_PAIRS)
    assert {(x["size"], x["dist"]) for x in d if x["type"] == 1} == {(s, p) for s in cmc.SIZES for p in cmc.DIST_PAIRS}
    assert {(x["size"], x["mask_type"]) for x in d if x["type"] == 2} == {(s, m) for s in cmc.SIZES for m in (0, 1)}
    assert Counter(x["size"] for x in d if x["type"] == 2 and x["mask_off"] < 0) == Counter(cmc.SIZES)
    assert {(x["size"], x["mask_sub"]) for x in d if x["type"] == 3} == {(s, m) for s in cmc.SIZES for m in (0, 1) if m == 0 or max(s) <= 64}
    for sub in (0, 1):
        wide = {x["mask_stride"] > (x["size"][0] << sub) for x in d if x["type"] == 3 and x["mask_sub"] == sub}
        assert wide == {False, True}
    for t in (2, 3): assert {x["mask_off"] % 4 for x in d if x["type"] == t and x["mask_off"] >= 0} == {0, 1, 2, 3}
    # every size and type meets every content, the saturated ones included; every flavour pair of every type meets a saturated one
    assert {(x["size"], x["type"], x["content"]) for x in d} == {(s, t, k) for s in cmc.SIZES for t in range(4) for k in cmc.CONTENTS}
    assert len({(x["type"], x["f0"], x["f1"]) for x in d if x["content"] in ("max_on_0", "0_on_max")}) == 64
    assert any(x["type"] == 1 and x["dist"] == (13, 3) and x["content"] == "max_on_0" for x in d)


@pytest.mark.parametrize("bd,fmt", FMTS)
def test_compound_list_geometry(bd, fmt):
    """destinations packed and disjoint, mask ranges disjoint, every footprint the kernel reads inside its plane, the saturated regions really saturated"""
    c = cmc.compound_cases(bd, fmt)
    H, W = c.ref0.shape
    seen = np.zeros((c.dst_h, c.dst_w), np.int32); mseen = np.zeros(c.masks.size, np.int32)
    mx = (1 << bd) - 1
    for b, d in zip(c.blks, c.desc):
        seen[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w] += 1
        assert b.dst_x + b.w <= c.dst_w and b.dst_y + b.h <= c.dst_h
        for (x, y) in ((b.src0_x, b.src0_y), (b.src1_x, b.src1_y)):
            x0, y0, x1, y1 = cmc.footprint(x, y, b.w, b.h)
            assert 0 <= x0 and 0 <= y0 and x1 < W and y1 < H, d
        if d["content"] in ("max_on_0", "0_on_max"):
            v0, v1 = (mx, 0) if d["content"] == "max_on_0" else (0, mx)
            x0, y0, x1, y1 = cmc.footprint(b.src0_x, b.src0_y, b.w, b.h); assert (c.ref0[y0:y1 + 1, x0:x1 + 1] == v0).all()
            x0, y0, x1, y1 = cmc.footprint(b.src1_x, b.src1_y, b.w, b.h); assert (c.ref1[y0:y1 + 1, x0:x1 + 1] == v1).all()
        if b.mask_off >= 0:
            n = b.w * b.h if b.type == 2 else b.mask_stride * (b.h << b.mask_sub)
            assert b.mask_off + n <= c.masks.size
            mseen[b.mask_off:b.mask_off + n] += 1
    assert seen.max() == 1 and mseen.max() == 1
    assert seen.sum() == sum(w * h for w, h in cmc.SIZES) * 64 and seen.sum() > 0.9 * seen.size      # packed: under a tenth of the plane is left over
    assert c.ref0.size < 1 << 18                                                                      # small reference planes


def test_blend_lists_cover_every_size_mode_mask():
    for in_place in (True, False):
        c = cmc.blend_cases(in_place)
        want = {(s, m, sub, k) for s in cmc.BLEND_SIZES for k in cmc.MASK_CLASSES
                for (m, sub) in [(0, (sw, sh)) for sw in (0, 1) for sh in (0, 1) if max(s) <= 64 or (sw, sh) == (0, 0)] + [(1, (0, 0)), (2, (0, 0))]}
        assert len(want) == (15 * 6 + 3 * 3) * 3 == 297 == c.n
        assert {(x["size"], x["mode"], x["sub"], x["mask"]) for x in c.desc} == want
        seen = np.zeros((c.h, c.w), np.int32); mseen = np.zeros(c.masks.size, np.int32)
        for b in c.blks:
            seen[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w] += 1
            need = b.mask_stride * (b.h << b.subh) if b.mode == 0 else (b.w if b.mode == 1 else b.h)
            mseen[b.mask_off:b.mask_off + need] += 1
            assert b.mask_off + need <= c.masks.size
            for (x, y) in ((b.src0_x, b.src0_y), (b.src1_x, b.src1_y), (b.dst_x, b.dst_y)): assert 0 <= x and 0 <= y and x + b.w <= c.w and y + b.h <= c.h
            if in_place: assert (b.src0_x, b.src0_y) == (b.dst_x, b.dst_y)      # out of place the destination is a plane of its own
        assert seen.max() == 1 and mseen.max() == 1
        assert {b.mask_stride > (b.w << b.subw) for b in c.blks if b.mode == 0} == {False, True}
    a, b1, _ = cmc.blend_planes(c, np.uint16)
    assert a.max() == 4095 == b1.max() and a.min() == 0 == b1.min()


def test_obmc_list_covers_every_size_offset_content():
    c = cmc.obmc_cases()
    assert c.n == 352 == len({(x["size"], x["offsets"], x["content"]) for x in c.desc})
    assert {(x["size"], x["offsets"], x["content"]) for x in c.desc} == {(s, o, k) for s in cmc.SIZES for o in cmc.OBMC_OFFSETS for k in cmc.OBMC_CONTENTS}
    assert {x["eighths"][0] for x in c.desc if x["offsets"][0]} == set(range(1, 8)) == {x["eighths"][1] for x in c.desc if x["offsets"][1]}
    assert all((x["eighths"][0] != 0, x["eighths"][1] != 0) == (bool(x["offsets"][0]), bool(x["offsets"][1])) for x in c.desc)
    seen = np.zeros(c.pre.shape, np.int32); wseen = np.zeros(c.wsrc.size, np.int32)
    for b, d in zip(c.blks, c.desc):
        assert b.pre_x + b.w + 1 <= c.pre.shape[1] and b.pre_y + b.h + 1 <= c.pre.shape[0]      # one sample of margin right and below
        seen[b.pre_y:b.pre_y + b.h + 1, b.pre_x:b.pre_x + b.w + 1] += 1
        wseen[b.wm_off:b.wm_off + b.w * b.h] += 1
        if d["content"] == "pre_max": assert (c.pre[b.pre_y:b.pre_y + b.h + 1, b.pre_x:b.pre_x + b.w + 1] == 255).all()
    assert seen.max() == 1 and wseen.min() == 1 == wseen.max()                                  # every content in its block's own rectangle and range
    assert c.mask.max() == 4096 and c.wsrc.max() == 255 * 4096


@pytest.mark.parametrize("ss", cmc.WARP_SS)
def test_warp_lists_cover_every_size_and_edge(ss):
    main, small = cmc.warp_cases(ss)
    assert len(cmc.WARP_ALL_SIZES) == 21 and (main.n, small.n) == (63, 21)
    for lst in (main, small):
        assert Counter(x["size"] for x in lst.desc) == Counter({s: lst.n // 21 for s in cmc.WARP_ALL_SIZES})
        seen = np.zeros((lst.dst_h, lst.dst_w), np.int32)
        for b in lst.blks: seen[b.p_row:b.p_row + b.p_height, b.p_col:b.p_col + b.p_width] += 1
        assert seen.max() == 1
    assert {x["cls"] for x in main.desc} == set(cmc.WARP_CLASSES)
    # what a record is labelled is what its cells do, by their footprints
    for x in main.desc:
        if x["cls"] in ("left", "right", "above", "below"): assert x["cls"] in x["edges"] and not any(e.startswith("astride") for e in x["edges"]), x
        elif x["cls"] not in ("random", "extreme"): assert x["cls"] in x["edges"], x
    edges = set().union(*(x["edges"] for x in main.desc))
    assert edges >= {"left", "right", "above", "below", "astride_left", "astride_right", "astride_top", "astride_bottom", "corner", "inside"}
    corners = {(("astride_left" in x["edges"]), ("astride_top" in x["edges"])) for x in main.desc if x["cls"] == "corner"}
    assert corners == {(a, b) for a in (False, True) for b in (False, True)}          # each of the four corners
    assert any(min(x["size"]) == 4 and any(e.startswith("astride") for e in x["edges"]) for x in main.desc)
    assert all("column_both_clamps" in x["edges"] for x in small.desc) and sum("row_both_clamps" in x["edges"] for x in small.desc) >= 10
    assert {x["cls"] for x in small.desc} >= {"random", "extreme", "astride_left", "corner"}
    assert cmc.WARP_SMALL[0] < 8 and cmc.WARP_SMALL[1] < 15 and cmc.WARP_SMALL[2] > cmc.WARP_SMALL[0]


def test_warp_compound_lists():
    c = cmc.warp_comp_cases()
    first, second, mixed, nulld = c.lists
    assert [l.name for l in c.lists] == ["first", "second", "mixed", "null_dst"]
    for l in c.lists: assert {(8, 8), (128, 128)} <= {x["size"] for x in l.desc} and any(x["size"][0] == 4 for x in l.desc)
    assert all(x["do_average"] == 0 and x["cb_stride"] > x["size"][0] for x in first.desc + nulld.desc)
    assert len({x["cb_off"] for x in first.desc}) == len(first.desc) and all(x["cb_off"] > 0 for x in first.desc)
    assert all(x["do_average"] == 1 for x in second.desc) and {x["jnt"] for x in second.desc} == {0, 1} and len({x["dist"] for x in second.desc if x["jnt"]}) >= 3
    assert [(x["cb_off"], x["cb_stride"]) for x in second.desc] == [(x["cb_off"], x["cb_stride"]) for x in first.desc]
    assert {x["do_average"] for x in mixed.desc} == {0, 1}
    # buffer ranges: a first-pass range is written once; destinations of the averaging blocks are disjoint
    used = np.zeros(c.cb_len, np.int32); seen = np.zeros((c.dst_h, c.dst_w), np.int32)
    for l in c.lists:
        for b in l.blks:
            w, h = b.blk.p_width, b.blk.p_height
            assert b.cb_off + (h - 1) * b.cb_stride + w <= c.cb_len
            if not b.do_average:
                for y in range(h): used[b.cb_off + y * b.cb_stride:b.cb_off + y * b.cb_stride + w] += 1
            else: seen[b.blk.p_row:b.blk.p_row + h, b.blk.p_col:b.blk.p_col + w] += 1
    assert used.max() == 1 and seen.max() == 1


# ---------------------------------------------------------------- restatement: oracle == numpy on every record
@pytest.mark.parametrize("bd,fmt", FMTS)
def test_compound_oracle_equals_numpy_and_closed_forms(orc, bd, fmt):
    c = cmc.compound_cases(bd, fmt)
    dst0, m0, exp, m_exp = cmc.compound_expected(orc, bd, fmt)
    taps = cmc.interp_taps(orc)
    outside = ~cmc.cover(exp.shape, [(b.dst_x, b.dst_y, b.w, b.h) for b in c.blks])
    assert np.array_equal(exp[outside], dst0[outside])
    stored = np.zeros(m0.size, bool)
    closed = Counter()
    for i, (b, d) in enumerate(zip(c.blks, c.desc)):
        out, seg = cmc.numpy_compound_block(b, c.ref0, c.ref1, c.masks, bd, taps)
        e = exp[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w]
        assert np.array_equal(out, e), (i, d, np.argwhere(out != e)[:4])
        if b.type == 2 and b.mask_off >= 0:
            assert np.array_equal(m_exp[b.mask_off:b.mask_off + b.w * b.h].reshape(b.h, b.w), seg), (i, d)
            stored[b.mask_off:b.mask_off + b.w * b.h] = True
        cf = cmc.closed_compound(d, bd)
        if cf:
            assert (e == cf[0]).all() and (cf[1] is None or (seg == cf[1]).all()), (i, d, cf)
            closed[(d["size"], d["type"])] += 1
            if d["content"] == "max_on_0":      # the table as stated
                if d["type"] == 0: assert cf[0] == cmc.CLOSED_COMPOUND["average"][bd]
                if d["type"] == 1 and d["dist"] == (13, 3): assert cf[0] == cmc.CLOSED_COMPOUND["distance_13_3"][bd]
                if d["type"] == 2 and d["mask_type"] == 0: assert cf == (cmc.CLOSED_COMPOUND["diffwtd_38_sample"][bd], cmc.CLOSED_COMPOUND["diffwtd_38_mask"][bd])
    assert np.array_equal(m_exp[~stored], m0[~stored])          # mask_off < 0: nothing stored anywhere
    assert len(closed) == 22 * 3                                # every size meets a closed form under AVERAGE, DISTANCE and DIFFWTD


@pytest.mark.parametrize("pix", [1, 2])
@pytest.mark.parametrize("in_place", [True, False])
def test_blend_oracle_equals_numpy_and_closed_forms(orc, pix, in_place):
    c = cmc.blend_cases(in_place)
    dt = np.uint8 if pix == 1 else np.uint16
    a, b1, dst = cmc.blend_planes(c, dt)
    exp = dst.copy()
    src0 = exp if in_place else a
    orc.orc_blend_a64_batch(pix, ptr(src0), c.w, ptr(b1), c.w, ptr(exp), c.w, ptr(c.masks), c.blks, c.n)
    changed = 0
    for i, (b, d) in enumerate(zip(c.blks, c.desc)):
        s0, s1 = a[b.src0_y:b.src0_y + b.h, b.src0_x:b.src0_x + b.w], b1[b.src1_y:b.src1_y + b.h, b.src1_x:b.src1_x + b.w]
        e = exp[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w]
        assert np.array_equal(cmc.numpy_blend_block(b, s0, s1, c.masks), e), (i, d)
        if d["mask"] == "all_64": assert np.array_equal(e, s0), (i, d)
        if d["mask"] == "all_0": assert np.array_equal(e, s1), (i, d)
        if d["sub"][1] and d["mask"] == "random": changed += not np.array_equal(cmc.numpy_blend_block(b, s0, s1, c.masks, ignore_subh=True), e)
    outside = ~cmc.cover(exp.shape, [(b.dst_x, b.dst_y, b.w, b.h) for b in c.blks])
    assert np.array_equal(exp[outside], dst[outside])
    assert changed >= 20                                         # sensitivity: a blend that ignores subh is wrong on the sub-sampled records


def test_obmc_oracle_equals_numpy_and_closed_forms(orc):
    c = cmc.obmc_cases()
    exp = cmc.obmc_expected(orc)
    narrow = []
    for i, (b, d) in enumerate(zip(c.blks, c.desc)):
        assert cmc.numpy_obmc_block(b, c.pre, c.wsrc, c.mask) == tuple(int(v) for v in exp[i]), (i, d)
        cf = cmc.closed_obmc(d)
        if cf: assert tuple(int(v) for v in exp[i]) == cf, (i, d)
        if cmc.numpy_obmc_block(b, c.pre, c.wsrc, c.mask, narrow_square=True) != tuple(int(v) for v in exp[i]): narrow.append((d["size"], d["content"]))
    big = [i for i, d in enumerate(c.desc) if d["size"] == (128, 128) and d["content"] == "pre_max"]
    assert len(big) == 4 and all(tuple(int(v) for v in exp[i]) == (4177920, 1065369600, 0) for i in big) and 4177920 ** 2 > 1 << 32
    assert ((128, 128), "pre_max") in narrow                     # sensitivity: a 32-bit sum * sum is wrong on the saturated 128 x 128 (and others)


@pytest.mark.parametrize("bd,fmt", FMTS)
@pytest.mark.parametrize("ss", cmc.WARP_SS)
def test_warp_oracle_equals_numpy(orc, bd, fmt, ss):
    dt = cmc.dtype_of(bd, fmt)
    unclamped = 0
    for lst in cmc.warp_cases(ss):
        plane, dst0, exp = cmc.warp_expected(orc, lst, ss, bd, dt)
        w, h, _ = lst.plane
        for i, (b, d) in enumerate(zip(lst.blks, lst.desc)):
            e = exp[b.p_row:b.p_row + b.p_height, b.p_col:b.p_col + b.p_width]
            out = cmc.numpy_warp_block(b, plane, w, h, ss, bd)
            assert np.array_equal(out, e), (lst.name, i, d, np.argwhere(out != e)[:4])
            if d["edges"] & {"left", "astride_left"}: unclamped += not np.array_equal(cmc.numpy_warp_block(b, plane, w, h, ss, bd, no_left_clamp=True), e)
        outside = ~cmc.cover(exp.shape, [(b.p_col, b.p_row, b.p_width, b.p_height) for b in lst.blks])
        assert np.array_equal(exp[outside], dst0[outside]) and (exp[~outside] != dst0[~outside]).any()
    assert unclamped >= 5                                        # sensitivity: not clamping at the left edge is wrong on the records that reach it


@pytest.mark.parametrize("bd,fmt", FMTS)
def test_warp_compound_oracle_equals_numpy(orc, bd, fmt):
    dt = cmc.dtype_of(bd, fmt)
    c = cmc.warp_comp_cases()
    w, h, _ = cmc.WARP_PLANE
    planes, steps = cmc.warp_comp_expected(orc, c, bd, dt)
    for n, l in enumerate(c.lists):
        (cb0, dst0), (cb1, dst1) = steps[n], steps[n + 1]
        want_cb, want_dst = cb0.copy(), dst0.copy()
        for i, b in enumerate(l.blks):
            bw, bh = b.blk.p_width, b.blk.p_height
            idx = b.cb_off + np.arange(bh)[:, None] * b.cb_stride + np.arange(bw)[None, :]
            out = cmc.numpy_warp_block(b.blk, planes[l.which], w, h, c.ss, bd, (b.do_average, b.use_jnt_comp_avg, b.fwd_offset, b.bck_offset), cb0[idx])
            if b.do_average: want_dst[b.blk.p_row:b.blk.p_row + bh, b.blk.p_col:b.blk.p_col + bw] = out
            else: want_cb[idx] = out
        assert np.array_equal(want_cb, cb1) and np.array_equal(want_dst, dst1), (l.name, bd)      # whole buffers: nothing else was touched
        assert (not np.array_equal(cb0, cb1)) == any(not b.do_average for b in l.blks) and (not np.array_equal(dst0, dst1)) == any(b.do_average for b in l.blks)


# ---------------------------------------------------------------- sensitivity of the compound list (blend, OBMC and warp: in their tests above)
def test_compound_list_is_sensitive(orc):
    c = cmc.compound_cases(8)
    _, _, exp, _ = cmc.compound_expected(orc, 8)
    taps = cmc.interp_taps(orc)
    outer, flavour, parity = set(), set(), set()
    for b, d in zip(c.blks, c.desc):
        e = exp[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w]
        if d["content"] in ("random", "binary"):
            if not np.array_equal(cmc.numpy_compound_block(b, c.ref0, c.ref1, c.masks, 8, cmc.zero_outer_taps(taps))[0], e): outer.add(d["size"])
            if d["f0"] != d["f1"] and not np.array_equal(cmc.numpy_compound_block(b, c.ref0, c.ref1, c.masks, 8, taps, same_flavour=True)[0], e):
                flavour.add((d["f0"], d["f1"]))
            if not np.array_equal(cmc.numpy_compound_block(b, c.ref0, c.ref1, c.masks, 8, taps, wrong_type=True)[0], e): parity.add((d["size"], d["type"]))
    assert outer == set(cmc.SIZES)                               # dropping the outer taps of the 8-tap banks shows at every size
    assert flavour == {(a, b) for a in range(4) for b in range(4) if a != b}      # reference 1 filtered as reference 0: at all 12 unequal pairs
    assert len(parity) == 88                                     # a type handled as its neighbour: at every (size, type)
