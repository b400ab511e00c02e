"""GPU: the per-call list kernels through their entry points by name, on the lists of percall_common (whose CPU test pins what they cover): more than one job
per launch, in list order and reversed, strides that are not the packed row length, per-job offsets, single units above 128 x 128.  One launch per list; every
output buffer is pre-filled and compared whole, the gaps between the jobs' outputs and what lies behind the last one included; n == 0 returns OK and writes
nothing.  Expected values: the oracle where it has the function, else the reference's `*_c` function (the `ref` fixture), exactly as the CPU test computes them."""
import ctypes as C

import numpy as np
import pytest

import percall_common as pc

pytestmark = pytest.mark.gpu


def at(dptr, nbytes):
    return C.c_void_p(dptr.value + nbytes)


def orders(n):
    """the list as built, and back to front"""
    return (list(range(n)), list(range(n - 1, -1, -1)))


def picked(jobs, order):
    return type(jobs)(*[jobs[i] for i in order])


def with_guard(a, fill):
    return np.concatenate([np.ascontiguousarray(a).ravel(), np.full(pc.GUARD, fill, a.dtype)])


def test_ext_all_sad_list(hip, orc):
    case = pc.ext_case()
    snaps = pc.ext_run(orc.orc_ext_all_sad_8x8_16x16, case)
    f = hip.L.svt_hip_ext_all_sad_8x8_16x16_batch_dev
    with hip.scope() as s:
        d_src, d_ref = s.upload(case["src"]), s.upload(case["ref"])
        for order in orders(6):
            d_state = s.upload(with_guard(case["state"][order], pc.FILL32))   # carried over the three launches on the device
            for g, jobs in enumerate(case["groups"]):
                hip.check(f(hip.h, d_src, pc.EXT_SS, d_ref, pc.EXT_RS, s.structs(picked(jobs, order)), 6, d_state), "ext all sad list")
                got = s.download(d_state, (6 * 800 + pc.GUARD,), np.uint32)
                assert np.array_equal(got[:4800].reshape(6, 800), snaps[g][order]) and (got[4800:] == pc.FILL32).all(), ("ext all sad", order[0], g)
            hip.check(f(hip.h, d_src, pc.EXT_SS, d_ref, pc.EXT_RS, s.structs(case["groups"][0]), 0, d_state), "ext all sad, n = 0")
            assert np.array_equal(s.download(d_state, (6 * 800 + pc.GUARD,), np.uint32), got)


def test_ext_eight_sad_list(hip, orc):
    snaps = pc.ext_run(orc.orc_ext_all_sad_8x8_16x16, pc.ext_case())
    f = hip.L.svt_hip_ext_eight_sad_32x32_64x64_batch_dev
    with hip.scope() as s:
        for (before, after), mvs in zip(pc.eight_run(orc.orc_ext_eight_sad_32x32_64x64, snaps), pc.EIGHT_MVS):
            for order in orders(5):
                d_state, d_mv = s.upload(with_guard(before[order], pc.FILL32)), s.upload(mvs[order])
                hip.check(f(hip.h, d_mv, 0, d_state), "ext eight sad, n = 0")
                assert np.array_equal(s.download(d_state, (5 * 170 + pc.GUARD,), np.uint32), with_guard(before[order], pc.FILL32))
                hip.check(f(hip.h, d_mv, 5, d_state), "ext eight sad list")
                assert np.array_equal(s.download(d_state, (5 * 170 + pc.GUARD,), np.uint32), with_guard(after[order], pc.FILL32)), ("ext eight sad", order[0])


def test_interm_var_list(hip, ref):
    case = pc.ivar_case()
    n = pc.IVAR_N
    mean, mean_sq = pc.ivar_run(ref, case["plane"], case["offs"])
    f = hip.L.svt_hip_interm_var_four8x8_batch_dev
    with hip.scope() as s:
        d_plane = s.upload(case["plane"])
        for order in orders(n):
            slots = (4 * np.array(order)[:, None] + np.arange(4)).ravel()
            d_offs, d_mean, d_sq = s.upload(case["offs"][order]), s.filled(4 * n + pc.GUARD, pc.FILL64, np.uint64), s.filled(4 * n + pc.GUARD, pc.FILL64, np.uint64)
            hip.check(f(hip.h, d_plane, pc.IVAR_STRIDE, d_offs, 0, d_mean, d_sq), "interm var, n = 0")
            assert (s.download(d_mean, (4 * n + pc.GUARD,), np.uint64) == pc.FILL64).all() and (s.download(d_sq, (4 * n + pc.GUARD,), np.uint64) == pc.FILL64).all()
            hip.check(f(hip.h, d_plane, pc.IVAR_STRIDE, d_offs, n, d_mean, d_sq), "interm var list")
            assert np.array_equal(s.download(d_mean, (4 * n + pc.GUARD,), np.uint64), with_guard(mean[slots], pc.FILL64)), ("mean", order[0])
            assert np.array_equal(s.download(d_sq, (4 * n + pc.GUARD,), np.uint64), with_guard(mean_sq[slots], pc.FILL64)), ("mean of squares", order[0])


def test_upsampled_pred_lists(hip, orc):
    f = hip.L.svt_hip_upsampled_pred_batch_dev
    for name, plane, stride, jobs, nbytes in pc.ups_lists():
        exp = pc.ups_run(pc.ups_by_oracle(orc), plane, stride, jobs, nbytes)
        with hip.scope() as s:
            d_plane = s.upload(plane)
            for order in orders(len(jobs)):
                d_dst = s.filled(len(exp), pc.FILL8, np.uint8)
                if name == "mixed":
                    hip.check(f(hip.h, d_plane, stride, d_dst, s.structs(jobs), 0), "upsampled pred, n = 0")
                    assert (s.download(d_dst, exp.shape, np.uint8) == pc.FILL8).all()
                hip.check(f(hip.h, d_plane, stride, d_dst, s.structs(picked(jobs, order)), len(jobs)), "upsampled pred list")
                got = s.download(d_dst, exp.shape, np.uint8)
                bad = [(j.w, j.h, j.subpel_x_q3, j.subpel_y_q3, j.bank) for j in jobs if not np.array_equal(got[j.dst_off:j.dst_off + j.w * j.h], exp[j.dst_off:j.dst_off + j.w * j.h])]
                assert not bad and np.array_equal(got, exp), (name, order[0], bad)


@pytest.mark.parametrize("stride,cs,dst8", pc.CDEF_RUNS)
def test_cdef_filter_block_list(hip, orc, stride, cs, dst8):
    case = pc.cdef_case(stride, cs)
    jobs = case["jobs"]
    exp = pc.cdef_run(pc.cdef_by_oracle(orc, stride), case["img"], stride, jobs, dst8)
    f = hip.L.svt_hip_cdef_filter_block_batch_dev
    with hip.scope() as s:
        d_img = s.upload(case["img"])
        for order in orders(len(jobs)):
            d_dst = s.filled(exp.shape, pc.FILL8 if dst8 else pc.FILL16, exp.dtype)
            dsts = (d_dst, None) if dst8 else (None, d_dst)
            hip.check(f(hip.h, d_img, stride, s.structs(jobs), 0, *dsts, pc.CDEF_DST_STRIDE), "cdef filter block, n = 0")
            assert (s.download(d_dst, exp.shape, exp.dtype) == exp.flat[0]).all()
            hip.check(f(hip.h, d_img, stride, s.structs(picked(jobs, order)), len(jobs), *dsts, pc.CDEF_DST_STRIDE), "cdef filter block list")
            got = s.download(d_dst, exp.shape, exp.dtype)
            assert np.array_equal(got, exp), (stride, cs, dst8, order[0], np.argwhere(got != exp)[:4].tolist())


def test_search_one_dual_steps(hip, ref):
    """nb_strengths 0 .. 7, the pairs chosen so far carried on the device; entries of d_lev0 / d_lev1 behind the step's own stay as they were"""
    f = hip.L.svt_hip_cdef_search_one_dual_dev
    for (sb_count, (start, end)), (m0, m1), steps in zip(pc.DUAL_SETS, pc.dual_tables(), pc.dual_run(ref)):
        with hip.scope() as s:
            d_m0, d_m1, d_lev, d_work = s.upload(m0), s.upload(m1), s.filled(16 + pc.GUARD, -7, np.int32), s.empty(8 * (4097 + sb_count))
            for nb, (l0, l1, tot) in enumerate(steps):
                hip.check(f(hip.h, d_m0, d_m1, sb_count, d_lev, at(d_lev, 32), nb, start, end, d_work), "search one dual")
                lev = s.download(d_lev, (16 + pc.GUARD,), np.int32)
                got = int(s.download(d_work, (1,), np.uint64)[0])
                assert got == tot and np.array_equal(lev[:8], l0) and np.array_equal(lev[8:16], l1) and (lev[16:] == -7).all(), (sb_count, nb, got, tot, lev[:16], l0, l1)


def test_convolve8_units(hip, ref):
    src, cases = pc.conv8_case()
    table, _ = pc.conv8_table()
    with hip.scope() as s:
        d_src, d_table = s.upload(src), s.upload(table)
        for case in cases:
            vert, step, q0, w, h = case
            exp = pc.conv8_expected(ref, src, case)
            ds = exp.shape[1]
            d_dst = s.filled(exp.shape, pc.FILL8, np.uint8)
            hip.check(hip.L.svt_hip_convolve8_dev(hip.h, vert, at(d_src, pc.CONV8_AT[0] * pc.CONV8_SS + pc.CONV8_AT[1]), pc.CONV8_SS, at(d_dst, ds + 2), ds, d_table, q0, step, w, h), "convolve8")
            assert np.array_equal(s.download(d_dst, exp.shape, np.uint8), exp), case


@pytest.mark.parametrize("pix_bytes,bd,r0,r1", pc.WIENER_FORMATS)
def test_wiener_convolve_units(hip, orc, pix_bytes, bd, r0, r1):
    src = pc.wiener_plane(pix_bytes, bd)
    with hip.scope() as s:
        d_src, d_taps = s.upload(src), s.upload(pc.WIENER_TAPS)
        for w, h in pc.WIENER_SIZES:
            exp = pc.wiener_expected(orc, pix_bytes, bd, r0, r1, w, h)
            ds = exp.shape[1]
            d_dst = s.upload(np.full(exp.shape, exp.flat[0], exp.dtype))
            hip.check(hip.L.svt_hip_wiener_convolve_add_src_dev(hip.h, pix_bytes, bd, at(d_src, (pc.WIENER_AT[0] * pc.WIENER_SS + pc.WIENER_AT[1]) * pix_bytes), pc.WIENER_SS,
                                                                at(d_dst, (ds + 3) * pix_bytes), ds, d_taps, w, h, r0, r1), "wiener convolve")
            assert np.array_equal(s.download(d_dst, exp.shape, exp.dtype), exp), (pix_bytes, bd, w, h)


def test_jnt_convolve_units(hip, orc, ref):
    banks = pc.interp_banks(orc)
    f = hip.L.svt_hip_jnt_convolve_dev
    for case in pc.jnt_cases():
        pb, bd, variant, w, h, _, _, (jnt, fwd, bck) = case
        exp_cb, exp_out = pc.jnt_expected(ref, banks, case)
        cshape, coff, dshape, doff = pc.jnt_layout(w, h)
        with hip.scope() as s:
            d_imgs = [s.upload(p) for p in pc.jnt_planes(pb, bd)]
            d_cb, d_out, d_taps = s.filled(cshape, 4321, np.uint16), s.upload(np.full(dshape, exp_out.flat[0], exp_out.dtype)), s.upload(pc.jnt_taps(banks, case))
            for do_avg in (0, 1):
                hip.check(f(hip.h, pb, bd, variant, at(d_imgs[do_avg], (pc.JNT_AT[0] * pc.JNT_SS + pc.JNT_AT[1]) * pb), pc.JNT_SS, at(d_out, doff * pb), dshape[1], at(d_cb, 2 * coff),
                            cshape[1], d_taps, w, h, 5 if bd == 12 else 3, 7, do_avg, jnt, fwd, bck), "jnt convolve")
                cb, out = s.download(d_cb, cshape, np.uint16), s.download(d_out, dshape, exp_out.dtype)
                assert np.array_equal(cb, exp_cb), ("compound buffer", case, do_avg)
                assert np.array_equal(out, exp_out) if do_avg else (out == exp_out.flat[0]).all(), ("pixels", case, do_avg)


def test_masked_compound_units(hip, ref):
    for kind, pb, bd in pc.MASK_KINDS:
        rnd, shift = pc.mask_args(kind, bd)
        for w, h in pc.BIG_SIZES:
            a, b = pc.mask_inputs(kind, bd, w, h)
            with hip.scope() as s:
                d_a, d_b = s.upload(a), s.upload(b)
                for inverse in (0, 1):
                    exp = pc.mask_expected(ref, kind, bd, w, h, inverse)
                    d_mask = s.filled(exp.shape, pc.FILL8, np.uint8)
                    hip.check(hip.L.svt_hip_diffwtd_mask_dev(hip.h, pb, d_mask, at(d_a, (a.shape[1] + 2) * pb), a.shape[1], at(d_b, (b.shape[1] + 3) * pb), b.shape[1], w, h, inverse,
                                                             rnd, shift), "diffwtd mask")
                    assert np.array_equal(s.download(d_mask, exp.shape, np.uint8), exp), (kind, bd, w, h, inverse)
    for pb, bd in pc.JNT_FORMATS:
        for w, h in pc.BIG_SIZES:
            c0, c1 = pc.mask_inputs("d16", bd, w, h)
            with hip.scope() as s:
                d_0, d_1 = s.upload(c0), s.upload(c1)
                for subw, subh in ((0, 0), (1, 1), (1, 0), (0, 1)):
                    mk = pc.blend_mask(w, h, subw, subh)
                    exp = pc.blend_expected(ref, pb, bd, w, h, subw, subh)
                    d_mk, d_dst = s.upload(mk), s.upload(np.full(exp.shape, exp.flat[0], exp.dtype))
                    hip.check(hip.L.svt_hip_blend_a64_d16_dev(hip.h, pb, bd, at(d_dst, (w + 4 + 1) * pb), w + 4, at(d_0, 2 * (c0.shape[1] + 2)), c0.shape[1], at(d_1, 2 * (c1.shape[1] + 3)),
                                                              c1.shape[1], at(d_mk, 1), mk.shape[1], w, h, subw, subh, 5 if bd == 12 else 3, 7), "blend a64 d16")
                    assert np.array_equal(s.download(d_dst, exp.shape, exp.dtype), exp), (pb, bd, w, h, subw, subh)


@pytest.mark.parametrize("pix_bytes", [1, 2])
def test_sgr_flt_proj_units(hip, orc, pix_bytes):
    f = hip.L.svt_hip_sgr_flt_proj_dev
    for w, h in pc.SGR_SIZES:
        arrays = pc.sgr_inputs(pix_bytes, w, h)
        with hip.scope() as s:
            d = [s.upload(a) for a in arrays]
            ptrs = [(at(dp, (a.shape[1] + 2) * a.itemsize), a.shape[1]) for dp, a in zip(d, arrays)]
            flat = [v for p in ptrs for v in p]
            for radii in pc.SGR_RADII + ((0, 0),):
                sums, xq, err = pc.sgr_expected(orc, pix_bytes, w, h, radii)
                for mode in ((0, 1) if radii != (0, 0) else (1,)):
                    d_acc, d_xq = s.filled(5 + pc.GUARD, pc.FILL64, np.uint64), s.filled(2 + pc.GUARD, -7, np.int32)
                    hip.check(f(hip.h, pix_bytes, *flat, w, h, radii[0], radii[1], mode, pc.vp(pc.SGR_XQ), d_acc, d_xq), "sgr flt proj")
                    acc, got_xq = s.download(d_acc, (5 + pc.GUARD,), np.uint64), s.download(d_xq, (2 + pc.GUARD,), np.int32)
                    assert (acc[5:] == pc.FILL64).all() and (got_xq[2:] == -7).all()
                    if mode == 0:
                        assert np.array_equal(acc[:5].view(np.int64), sums) and np.array_equal(got_xq[:2], xq), (pix_bytes, w, h, radii, acc[:5].view(np.int64), sums, got_xq[:2], xq)
                    else:
                        assert int(acc[0]) == err and not acc[1:5].any() and (got_xq[:2] == -7).all(), (pix_bytes, w, h, radii, int(acc[0]), err)
