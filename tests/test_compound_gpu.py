"""GPU parity: compound (two-reference) prediction (HIP through the C ABI) vs the oracle, which tests/test_oracle_vs_ref.py pins to two
svt_av1_[highbd_]jnt_convolve_*_c calls, svt_av1_build_compound_diffwtd_mask_d16_c and svt_aom_{lowbd,highbd}_blend_a64_d16_mask_c.
All 22 AV1 block sizes, the four convolve flavours per reference, average / distance / diff-weighted / supplied-mask (also sub-sampled).
The test_*_every_* tests and test_warp_compound_batched launch the deterministic lists of tests/comp_common.py, whose content tests/test_comp_ref_cpu.py proves
on the CPU: one launch per list and format, every buffer the kernel writes pre-filled with a non-zero pattern that must survive outside the blocks."""
import numpy as np
import pytest

from conftest import ptr
import comp_common as cmc
import fmt_common as fc

pytestmark = pytest.mark.gpu


def plant(plane, bd, x0, y0):
    """all max, all 0, a 0 / max checkerboard and random 0 / max samples, 192 x 192 each, from (x0, y0) on: the interpolators overshoot the range there"""
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:192, 0:192]
    plane[y0:y0 + 192, x0:x0 + 192] = mx; plane[y0:y0 + 192, x0 + 192:x0 + 384] = 0
    plane[y0 + 192:y0 + 384, x0:x0 + 192] = ((yy + xx) & 1) * mx
    plane[y0 + 192:y0 + 384, x0 + 192:x0 + 384] = np.random.default_rng(x0 + y0).integers(0, 2, (192, 192)) * mx


@pytest.mark.parametrize("bd,fmt", fc.bd_fmts(8, 10, 12))
def test_compound_blocks(hip, orc, bd, fmt):
    fc.two_witnesses(_compound_blocks, fmt, bd, hip, orc)


def _compound_blocks(hip, orc, bd, dt, wide):
    rng = np.random.default_rng(500 + bd)
    W, H = 1536, 1152
    ref0 = rng.integers(0, 1 << bd, (H, W)).astype(dt); ref1 = rng.integers(0, 1 << bd, (H, W)).astype(dt)
    ref0[:200, :200] = (1 << bd) - 1; ref1[:200, :200] = 0
    if wide:
        plant(ref0, bd, 256, 0); plant(ref1, bd, 320, 64)      # the two references' regions overlap out of step
    n = 80
    blks, masks = cmc.make_blocks(rng, W - 256, H - 128, n, 1 << 21)
    for b in blks:
        b.src0_x += 64; b.src0_y += 64; b.src1_x += 64; b.src1_y += 64; b.dst_x += 8; b.dst_y += 8
    exp = np.zeros((H, W), dt); m_exp = masks.copy()
    orc.orc_compound_predict_batch(ref0.itemsize, bd, ptr(ref0), W, ptr(ref1), W, ptr(exp), W, ptr(m_exp), blks, 0, n)
    d_r0, d_r1, d_dst, d_m = hip.to_device(ref0), hip.to_device(ref1), hip.to_device(np.zeros((H, W), dt)), hip.to_device(masks)
    d_b = hip.to_device(np.frombuffer(bytes(blks), np.uint8).copy())
    hip.check(hip.L.svt_hip_compound_predict_batch_dev(hip.h, ref0.itemsize, bd, d_r0, W, d_r1, W, d_dst, W, d_m, d_b, n), "compound")
    got = hip.to_host(d_dst, (H, W), dt); m_got = hip.to_host(d_m, masks.shape, np.uint8)
    hip.free(d_r0, d_r1, d_dst, d_m, d_b)
    for i, b in enumerate(blks):
        g, e = got[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w], exp[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w]
        assert np.array_equal(g, e), (bd, i, b.type, b.w, b.h, (b.subpel0_x, b.subpel0_y, b.subpel1_x, b.subpel1_y), np.argwhere(g != e)[:4])
    assert np.array_equal(got, exp) and np.array_equal(m_got, m_exp)
    assert (m_exp != masks).any() and exp.any()
    return got, exp


def test_compound_empty_and_bad_args(hip):
    assert hip.L.svt_hip_compound_predict_batch_dev(hip.h, 1, 8, None, 0, None, 0, None, 0, None, None, 0) == 0
    assert hip.L.svt_hip_compound_predict_batch_dev(hip.h, 1, 10, None, 0, None, 0, None, 0, None, None, 0) != 0
    assert hip.L.svt_hip_compound_predict_batch_dev(hip.h, 1, 8, None, 0, None, 0, None, 0, None, None, 3) != 0


def test_obmc_costs(hip, orc):
    """svt_hip_obmc_cost_batch_dev vs the oracle (pinned to svt_aom_obmc_sad / obmc_variance / obmc_sub_pixel_variance for all block sizes)."""
    rng = np.random.default_rng(9)
    W, H = 640, 480
    pre = rng.integers(0, 256, (H, W)).astype(np.uint8); pre[:140, :140] = 255
    n = 4 * len(cmc.SIZES)
    blks = (cmc.ObmcBlk * n)()
    off = 0
    for i in range(n):
        w, h = cmc.SIZES[i % len(cmc.SIZES)]
        blks[i] = cmc.ObmcBlk(int(rng.integers(0, W - 130)) if i else 0, int(rng.integers(0, H - 130)) if i else 0, w, h,
                          0 if i % 3 == 0 else int(rng.integers(0, 8)), 0 if i % 3 == 0 else int(rng.integers(0, 8)), off)
        off += w * h
    wsrc = rng.integers(0, 255 * 4096 + 1, off).astype(np.int32); mask = rng.integers(0, 4097, off).astype(np.int32)
    wsrc[:128 * 128] = 0; mask[:128 * 128] = 4096
    exp = np.zeros((n, 3), np.uint32)
    orc.orc_obmc_batch(ptr(pre), W, ptr(wsrc), ptr(mask), blks, n, ptr(exp))
    d_pre, d_w, d_m, d_b, d_o = hip.to_device(pre), hip.to_device(wsrc), hip.to_device(mask), hip.to_device(np.frombuffer(bytes(blks), np.uint8).copy()), hip.empty(exp.nbytes)
    hip.check(hip.L.svt_hip_obmc_cost_batch_dev(hip.h, d_pre, W, d_w, d_m, d_b, n, d_o), "obmc")
    got = hip.to_host(d_o, exp.shape, np.uint32)
    hip.free(d_pre, d_w, d_m, d_b, d_o)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:6]
    assert exp.any() and hip.L.svt_hip_obmc_cost_batch_dev(hip.h, None, 0, None, None, None, 0, None) == 0


@pytest.mark.parametrize("bd,fmt", fc.bd_fmts(8, 10, 12))
@pytest.mark.parametrize("ss", [0, 1])
def test_warp_blocks(hip, orc, bd, fmt, ss):
    """svt_hip_warp_predict_batch_dev vs the oracle (pinned to svt_av1_[highbd_]warp_affine_c): block sizes 8..128, random and extreme shear,
    models that move the block outside the plane (edge clamping), luma and 4:2:0 chroma sub-sampling."""
    fc.two_witnesses(_warp_blocks, fmt, bd, hip, orc, ss)


def _warp_blocks(hip, orc, ss, bd, dt, wide):
    rng = np.random.default_rng(700 + bd + ss)
    W, H = 1152, 640
    plane = rng.integers(0, 1 << bd, (H, W)).astype(dt)
    if wide:
        plant(plane, bd, 0, 0); plant(plane, bd, 640, 192)
    n = 40
    blks = cmc.warp_blocks(rng, W, H, n)
    exp = np.zeros((H, W), dt)
    orc.orc_warp_predict_batch(plane.itemsize, bd, ptr(plane), W, H, W, ptr(exp), W, ss, ss, blks, n)
    d_p, d_o, d_b = hip.to_device(plane), hip.to_device(np.zeros((H, W), dt)), hip.to_device(np.frombuffer(bytes(blks), np.uint8).copy())
    hip.check(hip.L.svt_hip_warp_predict_batch_dev(hip.h, plane.itemsize, bd, d_p, W, H, W, d_o, W, ss, ss, d_b, n), "warp")
    got = hip.to_host(d_o, (H, W), dt)
    hip.free(d_p, d_o, d_b)
    for i, b in enumerate(blks):
        g, e = got[b.p_row:b.p_row + b.p_height, b.p_col:b.p_col + b.p_width], exp[b.p_row:b.p_row + b.p_height, b.p_col:b.p_col + b.p_width]
        assert np.array_equal(g, e), (bd, ss, i, b.p_width, b.p_height, np.argwhere(g != e)[:4])
    assert np.array_equal(got, exp) and exp.any()
    return got, exp


@pytest.mark.parametrize("bd", [8, 10])
def test_blend_a64(hip, orc, bd):
    """svt_hip_blend_a64_batch_dev vs the oracle (pinned to svt_aom_[highbd_]blend_a64_{mask,hmask,vmask}_c), incl. blocks blended in place."""
    rng = np.random.default_rng(900 + bd)
    dt = np.uint8 if bd == 8 else np.uint16
    W, H = 1024, 768
    a = rng.integers(0, 1 << bd, (H, W)).astype(dt); b1 = rng.integers(0, 1 << bd, (H, W)).astype(dt)
    n = 48
    blks, masks = cmc.blend_blocks(rng, W, H, n, 1 << 19)
    # in-place blocks read their own destination; keep every other block's sources away from all destinations so that block order cannot matter
    for b in blks:
        if (b.src0_x, b.src0_y) != (b.dst_x, b.dst_y): b.src0_x, b.src0_y = b.dst_x, b.dst_y
    exp = a.copy()
    orc.orc_blend_a64_batch(a.itemsize, ptr(exp), W, ptr(b1), W, ptr(exp), W, ptr(masks), blks, n)
    d_a, d_b, d_m, d_k = hip.to_device(a), hip.to_device(b1), hip.to_device(masks), hip.to_device(np.frombuffer(bytes(blks), np.uint8).copy())
    hip.check(hip.L.svt_hip_blend_a64_batch_dev(hip.h, a.itemsize, d_a, W, d_b, W, d_a, W, d_m, d_k, n), "blend")
    got = hip.to_host(d_a, (H, W), dt)
    hip.free(d_a, d_b, d_m, d_k)
    assert np.array_equal(got, exp) and (exp != a).any()


# ================================================================ the full case grids of tests/comp_common.py
def _dev_blks(hip, blks):
    return hip.to_device(np.frombuffer(bytes(blks), np.uint8).copy())


def _fmt(dt, wide):
    return dt if wide else None


@pytest.mark.parametrize("bd,fmt", fc.bd_fmts(8, 10, 12))
def test_compound_every_size_type_flavour(hip, orc, bd, fmt):
    """compound_predict_kernel on 22 sizes x 4 types x 16 flavour pairs (1408 blocks, one launch): every block against the oracle, the plane and the mask buffer
    whole, the closed forms on saturated content, the pre-fill outside the blocks and in the mask buffer wherever no DIFFWTD record stores."""
    fc.two_witnesses(_compound_every, fmt, bd, hip, orc)


def _compound_every(hip, orc, bd, dt, wide):
    c = cmc.compound_cases(bd, _fmt(dt, wide))
    dst0, m0, exp, m_exp = cmc.compound_expected(orc, bd, _fmt(dt, wide))
    d_r0, d_r1, d_dst, d_m, d_b = hip.to_device(c.ref0), hip.to_device(c.ref1), hip.to_device(dst0), hip.to_device(m0), _dev_blks(hip, c.blks)
    hip.check(hip.L.svt_hip_compound_predict_batch_dev(hip.h, c.ref0.itemsize, bd, d_r0, c.ref0.shape[1], d_r1, c.ref1.shape[1], d_dst, c.dst_w, d_m, d_b, c.n), "compound")
    got = hip.to_host(d_dst, exp.shape, dt); m_got = hip.to_host(d_m, m0.shape, np.uint8)
    hip.free(d_r0, d_r1, d_dst, d_m, d_b)
    stored = np.zeros(m0.size, bool)
    for i, (b, d) in enumerate(zip(c.blks, c.desc)):
        g, e = got[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w], exp[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w]
        assert np.array_equal(g, e), (bd, i, d, np.argwhere(g != e)[:4])
        if b.type == 2 and b.mask_off >= 0:
            stored[b.mask_off:b.mask_off + b.w * b.h] = True
            assert np.array_equal(m_got[b.mask_off:b.mask_off + b.w * b.h], m_exp[b.mask_off:b.mask_off + b.w * b.h]), (bd, i, d, "stored mask")
    assert np.array_equal(got, exp) and np.array_equal(m_got, m_exp)
    for i, (b, d) in enumerate(zip(c.blks, c.desc)):
        cf = cmc.closed_compound(d, bd)
        if cf:
            assert (got[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w] == cf[0]).all(), (bd, i, d, cf)
            if cf[1] is not None and b.mask_off >= 0: assert (m_got[b.mask_off:b.mask_off + b.w * b.h] == cf[1]).all(), (bd, i, d, cf)
    outside = ~cmc.cover(exp.shape, [(b.dst_x, b.dst_y, b.w, b.h) for b in c.blks])
    assert outside.any() and np.array_equal(got[outside], dst0[outside])
    assert (~stored).any() and np.array_equal(m_got[~stored], m0[~stored])      # the supplied masks, the gaps, and everything a mask_off < 0 record could have hit
    return got, exp


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("pix", [1, 2])
def test_blend_every_size_mode_mask(hip, orc, pix, in_place):
    """blend_a64_kernel on 18 sizes x (2-D mask with every sub-sampling, hmask, vmask) x (random, all 64, all 0): blended into src0 itself, and into a plane of its own."""
    c = cmc.blend_cases(in_place)
    dt = np.uint8 if pix == 1 else np.uint16
    a, b1, dst0 = cmc.blend_planes(c, dt)
    exp = dst0.copy()
    orc.orc_blend_a64_batch(pix, ptr(exp if in_place else a), c.w, ptr(b1), c.w, ptr(exp), c.w, ptr(c.masks), c.blks, c.n)
    d_a, d_b, d_m, d_k = hip.to_device(a), hip.to_device(b1), hip.to_device(c.masks), _dev_blks(hip, c.blks)
    d_dst = d_a if in_place else hip.to_device(dst0)
    hip.check(hip.L.svt_hip_blend_a64_batch_dev(hip.h, pix, d_a, c.w, d_b, c.w, d_dst, c.w, d_m, d_k, c.n), "blend")
    got = hip.to_host(d_dst, exp.shape, dt); a_after = hip.to_host(d_a, a.shape, dt)
    hip.free(d_a, d_b, d_m, d_k, *([] if in_place else [d_dst]))
    for i, (b, d) in enumerate(zip(c.blks, c.desc)):
        g, e = got[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w], exp[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w]
        assert np.array_equal(g, e), (pix, in_place, i, d, np.argwhere(g != e)[:4])
    assert np.array_equal(got, exp)
    for i, (b, d) in enumerate(zip(c.blks, c.desc)):
        g = got[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w]
        if d["mask"] == "all_64": assert np.array_equal(g, a[b.src0_y:b.src0_y + b.h, b.src0_x:b.src0_x + b.w]), (pix, in_place, i, d)
        if d["mask"] == "all_0": assert np.array_equal(g, b1[b.src1_y:b.src1_y + b.h, b.src1_x:b.src1_x + b.w]), (pix, in_place, i, d)
    outside = ~cmc.cover(exp.shape, [(b.dst_x, b.dst_y, b.w, b.h) for b in c.blks])
    assert outside.any() and np.array_equal(got[outside], dst0[outside]) and (got != dst0).any()
    if not in_place: assert np.array_equal(a_after, a)


def test_obmc_every_size_offset_content(hip, orc):
    """obmc_cost_kernel on 22 sizes x the four offset classes x (random, predictor 255 on wsrc 0, predictor 0 on the largest wsrc, half and half), each content in
    its block's own rectangle: the saturated 128 x 128 needs the 64-bit sum * sum and the largest sse."""
    c = cmc.obmc_cases()
    exp = cmc.obmc_expected(orc)
    out0 = cmc.pattern((c.n + 2, 3), np.uint32, 0x80000001, 9973)
    d_pre, d_w, d_m, d_b, d_o = hip.to_device(c.pre), hip.to_device(c.wsrc), hip.to_device(c.mask), _dev_blks(hip, c.blks), hip.to_device(out0)
    hip.check(hip.L.svt_hip_obmc_cost_batch_dev(hip.h, d_pre, c.pre.shape[1], d_w, d_m, d_b, c.n, d_o), "obmc")
    got = hip.to_host(d_o, out0.shape, np.uint32)
    hip.free(d_pre, d_w, d_m, d_b, d_o)
    for i, d in enumerate(c.desc):
        assert tuple(got[i]) == tuple(exp[i]), (i, d, tuple(got[i]), tuple(exp[i]))
    assert np.array_equal(got[:c.n], exp)
    for i, d in enumerate(c.desc):
        cf = cmc.closed_obmc(d)
        if cf: assert tuple(int(v) for v in got[i]) == cf, (i, d, tuple(got[i]), cf)
    assert np.array_equal(got[c.n:], out0[c.n:])


@pytest.mark.parametrize("bd,fmt", fc.bd_fmts(8, 10, 12))
@pytest.mark.parametrize("ss", cmc.WARP_SS, ids=["444", "420", "422"])
def test_warp_every_size_edge_ss(hip, orc, bd, fmt, ss):
    """warp_predict_kernel<.., false> on 17 sizes + 4 x 4, 4 x 8, 8 x 4, 4 x 16, cells left of / right of / above / below the plane, astride each edge and each
    corner, and on a 6 x 5 plane where both clamps bind inside one filter; luma, 4:2:0 and 4:2:2 sub-sampling."""
    fc.two_witnesses(_warp_every, fmt, bd, hip, orc, ss)


def _warp_every(hip, orc, ss, bd, dt, wide):
    gots, exps = [], []
    for lst in cmc.warp_cases(ss):
        plane, dst0, exp = cmc.warp_expected(orc, lst, ss, bd, dt)
        w, h, stride = lst.plane
        d_p, d_o, d_b = hip.to_device(plane), hip.to_device(dst0), _dev_blks(hip, lst.blks)
        hip.check(hip.L.svt_hip_warp_predict_batch_dev(hip.h, plane.itemsize, bd, d_p, w, h, stride, d_o, lst.dst_w, ss[0], ss[1], d_b, lst.n), "warp")
        got = hip.to_host(d_o, exp.shape, dt)
        hip.free(d_p, d_o, d_b)
        for i, (b, d) in enumerate(zip(lst.blks, lst.desc)):
            g, e = got[b.p_row:b.p_row + b.p_height, b.p_col:b.p_col + b.p_width], exp[b.p_row:b.p_row + b.p_height, b.p_col:b.p_col + b.p_width]
            assert np.array_equal(g, e), (bd, ss, lst.name, i, d, np.argwhere(g != e)[:4])
        assert np.array_equal(got, exp)
        outside = ~cmc.cover(exp.shape, [(b.p_col, b.p_row, b.p_width, b.p_height) for b in lst.blks])
        assert outside.any() and np.array_equal(got[outside], dst0[outside]) and (got != dst0).any()
        gots.append(got); exps.append(exp)
    return gots, exps


@pytest.mark.parametrize("bd,fmt", fc.bd_fmts(8, 10, 12))
def test_warp_compound_batched(hip, orc, bd, fmt):
    """warp_predict_kernel<.., true> on lists of several blocks: a first pass (every block its own cb_off, cb_stride wider than the block), the second pass over the
    same buffer mixing plain average and distance weights, one launch mixing both passes on disjoint blocks, a first pass without a destination plane."""
    fc.two_witnesses(_warp_compound, fmt, bd, hip, orc)


def _warp_compound(hip, orc, bd, dt, wide):
    c = cmc.warp_comp_cases()
    w, h, stride = cmc.WARP_PLANE
    planes, steps = cmc.warp_comp_expected(orc, c, bd, dt)
    d_p = [hip.to_device(p) for p in planes]
    d_cb, d_dst = hip.to_device(steps[0][0]), hip.to_device(steps[0][1])
    gots, exps = [], []
    for n, l in enumerate(c.lists):
        d_b = _dev_blks(hip, l.blks)
        hip.check(hip.L.svt_hip_warp_compound_batch_dev(hip.h, planes[0].itemsize, bd, d_p[l.which], w, h, stride, None if l.null_dst else d_dst, c.dst_w, c.ss[0], c.ss[1],
                                                        d_cb, d_b, len(l.blks)), "warp compound " + l.name)
        cb = hip.to_host(d_cb, steps[0][0].shape, np.uint16); dst = hip.to_host(d_dst, steps[0][1].shape, dt)
        hip.free(d_b)
        (cb0, dst0), (cb1, dst1) = steps[n], steps[n + 1]
        touched_cb = np.zeros(cb.shape, bool); touched = np.zeros(dst.shape, bool)
        for i, (b, d) in enumerate(zip(l.blks, l.desc)):
            bw, bh = b.blk.p_width, b.blk.p_height
            idx = b.cb_off + np.arange(bh)[:, None] * b.cb_stride + np.arange(bw)[None, :]
            if b.do_average:
                g, e = dst[b.blk.p_row:b.blk.p_row + bh, b.blk.p_col:b.blk.p_col + bw], dst1[b.blk.p_row:b.blk.p_row + bh, b.blk.p_col:b.blk.p_col + bw]
                touched[b.blk.p_row:b.blk.p_row + bh, b.blk.p_col:b.blk.p_col + bw] = True
            else:
                g, e = cb[idx], cb1[idx]
                touched_cb[idx] = True
            assert np.array_equal(g, e), (bd, l.name, i, d, np.argwhere(g != e)[:4])
        assert np.array_equal(cb, cb1) and np.array_equal(dst, dst1), (bd, l.name)
        assert np.array_equal(cb[~touched_cb], cb0[~touched_cb]) and np.array_equal(dst[~touched], dst0[~touched]), (bd, l.name)      # the pre-fill, or the launch before
        gots += [cb, dst]; exps += [cb1, dst1]
    hip.free(d_cb, d_dst, *d_p)
    return gots, exps
