"""CPU: oracle restatement vs the REAL reference C functions (oracle/_ref, only where it was built —
i.e. in the build container).  Input distributions mirror /root/reference/test/SadTest.cc:
REF_MAX / SRC_MAX / RANDOM / ties (:194-246), Allsad/Extsad kernels (:838-1222), sad_LoopTest (:611-785)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_package, ptr


def _pair(rng, it):
    src = rng.integers(0, 256, (64, 80), dtype=np.uint8)
    refb = rng.integers(0, 256, (64, 96), dtype=np.uint8)
    if it % 5 == 1: src[:] = 255
    if it % 5 == 2: refb[:] = 255
    if it % 5 == 3: refb[:] = src[:, :1]
    return src, refb


# The three sample formats of the pins below: (uint16, 8) is 8-bit samples in 16-bit planes (the encoder's 16-bit pipeline on 8-bit video) -- the reference's
# HIGH-bit-depth function with bd = 8, content drawn from 0 .. 255.
FMT3 = ((8, np.uint8), (10, np.uint16), (8, np.uint16))


def test_ext_all_sad_and_32x32_64x64(orc, ref):
    rng = np.random.default_rng(13596)
    for it in range(120):
        sub = it & 1
        src, refb = _pair(rng, it)
        mv = int(rng.integers(0, 2 ** 32))
        outs = []
        for lib, n8, n32 in ((ref, "svt_ext_all_sad_calculation_8x8_16x16_c", "svt_ext_eight_sad_calculation_32x32_64x64_c"),
                             (orc, "orc_ext_all_sad_8x8_16x16", "orc_ext_eight_sad_32x32_64x64")):
            r2 = np.random.default_rng(it)
            bs8 = r2.integers(0, 20000, 64, dtype=np.uint32); bs16 = r2.integers(0, 70000, 16, dtype=np.uint32)
            bm8 = np.zeros(64, np.uint32); bm16 = np.zeros(16, np.uint32)
            e16 = np.zeros((16, 8), np.uint32); e8 = np.zeros((64, 8), np.uint32)
            getattr(lib, n8)(ptr(src), 80, ptr(refb), 96, C.c_uint32(mv), ptr(bs8), ptr(bs16), ptr(bm8), ptr(bm16), ptr(e16), ptr(e8), sub)
            bs32 = r2.integers(0, 270000, 4, dtype=np.uint32); bs64 = r2.integers(0, 1100000, 1, dtype=np.uint32)
            bm32 = np.zeros(4, np.uint32); bm64 = np.zeros(1, np.uint32); e32 = np.zeros((4, 8), np.uint32)
            getattr(lib, n32)(ptr(e16), ptr(bs32), ptr(bs64), ptr(bm32), ptr(bm64), C.c_uint32(mv), ptr(e32))
            outs.append([bs8, bs16, bm8, bm16, e16, e8, bs32, bs64, bm32, bm64, e32])
        for a, b in zip(*outs):
            assert np.array_equal(a, b)


def test_single_candidate_kernels(orc, ref):
    rng = np.random.default_rng(7)
    for it in range(60):
        sub = it & 1
        src, refb = _pair(rng, it)
        mv = int(rng.integers(0, 2 ** 32))
        outs = []
        for lib, n8, n32 in ((ref, "svt_ext_sad_calculation_8x8_16x16_c", "svt_ext_sad_calculation_32x32_64x64_c"),
                             (orc, "orc_ext_sad_8x8_16x16", "orc_ext_sad_32x32_64x64")):
            r2 = np.random.default_rng(it)
            bs8 = r2.integers(0, 20000, 4, dtype=np.uint32); bs16 = r2.integers(0, 70000, 1, dtype=np.uint32)
            bm8 = np.zeros(4, np.uint32); bm16 = np.zeros(1, np.uint32); s16 = np.zeros(1, np.uint32); s8 = np.zeros(4, np.uint32)
            getattr(lib, n8)(ptr(src), 80, ptr(refb), 96, ptr(bs8), ptr(bs16), ptr(bm8), ptr(bm16), C.c_uint32(mv), ptr(s16), ptr(s8), sub)
            sad16 = r2.integers(0, 60000, 16, dtype=np.uint32)
            bs32 = r2.integers(0, 200000, 4, dtype=np.uint32); bs64 = r2.integers(0, 900000, 1, dtype=np.uint32)
            bm32 = np.zeros(4, np.uint32); bm64 = np.zeros(1, np.uint32); s32 = np.zeros(4, np.uint32)
            getattr(lib, n32)(ptr(sad16), ptr(bs32), ptr(bs64), ptr(bm32), ptr(bm64), C.c_uint32(mv), ptr(s32))
            outs.append([bs8, bs16, bm8, bm16, s16, s8, bs32, bs64, bm32, bm64, s32])
        for a, b in zip(*outs):
            assert np.array_equal(a, b)


def test_sad_loop_and_nxm(orc, ref):
    rng = np.random.default_rng(1)
    orc.orc_nxm_sad.restype = C.c_uint32
    ref.svt_fast_loop_nxm_sad_kernel.restype = C.c_uint32
    for it in range(80):
        bw = int(rng.choice([4, 8, 16, 24, 32, 48, 64])); bh = int(rng.choice([4, 8, 16, 32, 64]))
        saw = int(rng.integers(1, 40)); sah = int(rng.integers(1, 20))
        src = rng.integers(0, 256, (bh, bw), dtype=np.uint8); rs = bw + saw + 5
        refb = rng.integers(0, 256, (bh + sah + 2, rs), dtype=np.uint8)
        if it % 4 == 0: refb[:] = 7; src[:] = 9
        res = []
        for lib, name in ((ref, "svt_sad_loop_kernel_c"), (orc, "orc_sad_loop")):
            best = C.c_uint64(0); xc = C.c_int16(-5); yc = C.c_int16(-7)
            getattr(lib, name)(ptr(src), bw, ptr(refb), rs, bh, bw, C.byref(best), C.byref(xc), C.byref(yc), rs, C.c_int16(saw), C.c_int16(sah))
            res.append((best.value, xc.value, yc.value))
        assert res[0] == res[1]
        assert ref.svt_fast_loop_nxm_sad_kernel(ptr(src), bw, ptr(refb), rs, bh, bw) == orc.orc_nxm_sad(ptr(src), bw, ptr(refb), rs, bh, bw)


def test_md_subpel_probe(orc, ref):
    """oracle/md_oracle.c::orc_md_subpel_probe (one probe of mode decision's sub-pel refinement) vs the reference's own svt_aom_upsampled_pred + svt_aom_variance{W}x{W}
    (svt_upsampled_pref_error, Encoder/Codec/mcomp.c:102-156) through oracle/ref_bench.c::refb_upsampled_var_batch: square blocks 8 .. 64, every eighth-pel phase, the three
    tap sets, saturating content."""
    rng = np.random.default_rng(47)
    orc.orc_md_subpel_probe.restype = C.c_uint32
    pad, W, H = 48, 256, 192
    src = rng.integers(0, 256, (H, W), dtype=np.uint8)
    refp = rng.integers(0, 256, (H + 2 * pad, W + 2 * pad), dtype=np.uint8)
    refp[pad:pad + 80, pad:pad + 80] = np.where(rng.random((80, 80)) < 0.5, 0, 255)
    st = refp.shape[1]
    n = 600
    jobs = np.zeros(n, np.dtype([("ref_off", "<i4"), ("dst_off", "<i4"), ("w", "u1"), ("h", "u1"), ("sx", "u1"), ("sy", "u1"), ("bank", "u1"), ("r", "u1", 3)]))
    src_off = np.zeros(n, np.int32)
    cases = []
    for i in range(n):
        s = int(rng.choice([8, 16, 32, 64])); bank = int(rng.choice([0, 3, 4]))
        x = int(rng.integers(0, (W - s) // 8 + 1)) * 8 if i >= 40 else 0; y = int(rng.integers(0, (H - s) // 8 + 1)) * 8 if i >= 40 else 0
        mvx, mvy = int(rng.integers(-30 * 8, 30 * 8 + 1)), int(rng.integers(-30 * 8, 30 * 8 + 1))
        jobs[i] = ((pad + y + (mvy >> 3)) * st + pad + x + (mvx >> 3), 0, s, s, mvx & 7, mvy & 7, bank, (0, 0, 0))
        src_off[i] = y * W + x
        cases.append((x, y, s, mvx, mvy, bank))
    e_var, e_sse = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    ref.refb_upsampled_var_batch(ptr(refp), st, ptr(src), W, ptr(jobs), ptr(src_off), 0, n, ptr(e_var), ptr(e_sse))
    base = C.c_void_p(refp.ctypes.data + pad * st + pad)
    for i, (x, y, s, mvx, mvy, bank) in enumerate(cases):
        sse = C.c_uint32(0)
        v = orc.orc_md_subpel_probe(ptr(src), W, base, st, x, y, s, mvx, mvy, bank, C.byref(sse))
        assert (v, sse.value) == (int(e_var[i]), int(e_sse[i])), (i, x, y, s, mvx, mvy, bank)


def test_md_compound_average_candidate(orc, ref):
    """oracle/md_oracle.c::orc_md_fullpel_avg_candidate (a NEW_NEWMV / COMPOUND_AVERAGE candidate of two full-pel vectors) vs what av1_inter_prediction runs for it: two calls of
    svt_av1_jnt_convolve_2d_copy_c (Common/Codec/convolve.c; svt_inter_predictor's table at [0][0][1]) with the compound conv_params of get_conv_params_no_round (round_0 3,
    round_1 7, a 16-bit destination plane; the second call averages: do_average 1, no distance weights for compound_idx 1), then svt_nxm_sad_kernel_helper_c."""
    rng = np.random.default_rng(53)
    orc.orc_md_fullpel_avg_candidate.restype = C.c_uint32
    ref.svt_nxm_sad_kernel_helper_c.restype = C.c_uint32
    fx = _IFP(C.addressof((C.c_int16 * 8 * 16).in_dll(ref, REF_BANKS[0])), 8, 16, 0)
    pad, W, H = 48, 256, 192
    src = rng.integers(0, 256, (H, W), dtype=np.uint8)
    r0 = rng.integers(0, 256, (H + 2 * pad, W + 2 * pad), dtype=np.uint8)
    r1 = rng.integers(0, 256, (H + 2 * pad, W + 2 * pad), dtype=np.uint8)
    r0[pad:pad + 64, pad:pad + 64] = 255; r1[pad:pad + 64, pad:pad + 64] = np.where(rng.random((64, 64)) < 0.5, 254, 255); src[:64, :64] = 0   # the rounding at the top of the range
    st = r0.shape[1]
    for it in range(200):
        s = int(rng.choice([8, 16, 32, 64]))
        x = int(rng.integers(0, (W - s) // 8 + 1)) * 8 if it >= 4 else 0; y = int(rng.integers(0, (H - s) // 8 + 1)) * 8 if it >= 4 else 0
        if it < 4: s = 64
        mv = [0, 0, 0, 0] if it < 4 else [int(v) for v in rng.integers(-40, 41, 4)]
        tmp16 = np.zeros((s, s), np.uint16); pred = np.zeros((s, s), np.uint8)
        cp = _ConvP(); cp.round_0 = 3; cp.round_1 = 7; cp.is_compound = 1; cp.dst = tmp16.ctypes.data; cp.dst_stride = s
        cp.do_average = 0
        ref.svt_av1_jnt_convolve_2d_copy_c(C.c_void_p(r0.ctypes.data + (pad + y + mv[1]) * st + pad + x + mv[0]), st, ptr(pred), s, s, s, C.byref(fx), C.byref(fx), 0, 0, C.byref(cp))
        cp.do_average = 1
        ref.svt_av1_jnt_convolve_2d_copy_c(C.c_void_p(r1.ctypes.data + (pad + y + mv[3]) * st + pad + x + mv[2]), st, ptr(pred), s, s, s, C.byref(fx), C.byref(fx), 0, 0, C.byref(cp))
        e = ref.svt_nxm_sad_kernel_helper_c(C.c_void_p(src.ctypes.data + y * W + x), W, ptr(pred), s, s, s)
        base0, base1 = C.c_void_p(r0.ctypes.data + pad * st + pad), C.c_void_p(r1.ctypes.data + pad * st + pad)
        g = orc.orc_md_fullpel_avg_candidate(ptr(src), W, base0, st, base1, st, x, y, s, s, mv[0], mv[1], mv[2], mv[3])
        assert e == g, (it, x, y, s, mv)


def test_md_candidates_on_16_bit_planes(orc, ref):
    """The 16-bit forms of the two mode-decision tables (a 10-bit encode's fast loop: reference_picture16bit, sad_16b_kernel): orc_md_fullpel_candidate16 vs the reference's
    svt_av1_highbd_convolve_2d_copy_sr_c + sad_16b_kernel_c, orc_md_fullpel_avg_candidate16 vs two svt_av1_highbd_jnt_convolve_2d_copy_c calls + sad_16b_kernel_c."""
    rng = np.random.default_rng(59)
    orc.orc_md_fullpel_candidate16.restype = C.c_uint32; orc.orc_md_fullpel_avg_candidate16.restype = C.c_uint32
    ref.sad_16b_kernel_c.restype = C.c_uint32
    fx = _IFP(C.addressof((C.c_int16 * 8 * 16).in_dll(ref, REF_BANKS[0])), 8, 16, 0)
    pad, W, H, bd = 48, 256, 192, 10
    src = rng.integers(0, 1024, (H, W), dtype=np.uint16)
    r0 = rng.integers(0, 1024, (H + 2 * pad, W + 2 * pad), dtype=np.uint16)
    r1 = rng.integers(0, 1024, (H + 2 * pad, W + 2 * pad), dtype=np.uint16)
    r0[pad:pad + 64, pad:pad + 64] = 1023; r1[pad:pad + 64, pad:pad + 64] = np.where(rng.random((64, 64)) < 0.5, 1022, 1023); src[:64, :64] = 0
    st = r0.shape[1]
    el = lambda arr, yy, xx: C.c_void_p(arr.ctypes.data + 2 * (yy * arr.shape[1] + xx))
    for it in range(200):
        s = int(rng.choice([8, 16, 32, 64]))
        x = int(rng.integers(0, (W - s) // 8 + 1)) * 8 if it >= 4 else 0; y = int(rng.integers(0, (H - s) // 8 + 1)) * 8 if it >= 4 else 0
        if it < 4: s = 64
        mv = [0, 0, 0, 0] if it < 4 else [int(v) for v in rng.integers(-40, 41, 4)]
        pred = np.zeros((s, s), np.uint16)
        cp = _ConvP(); cp.round_0 = 3; cp.round_1 = 11
        ref.svt_av1_highbd_convolve_2d_copy_sr_c(el(r0, pad + y + mv[1], pad + x + mv[0]), st, ptr(pred), s, s, s, C.byref(fx), C.byref(fx), 0, 0, C.byref(cp), bd)
        e = ref.sad_16b_kernel_c(el(src, y, x), W, ptr(pred), s, s, s)
        g = orc.orc_md_fullpel_candidate16(ptr(src), W, el(r0, pad, pad), st, x, y, s, s, mv[0], mv[1])
        assert e == g, ("single", it, x, y, s, mv)
        tmp16 = np.zeros((s, s), np.uint16)
        cp = _ConvP(); cp.round_0 = 3; cp.round_1 = 7; cp.is_compound = 1; cp.dst = tmp16.ctypes.data; cp.dst_stride = s
        cp.do_average = 0
        ref.svt_av1_highbd_jnt_convolve_2d_copy_c(el(r0, pad + y + mv[1], pad + x + mv[0]), st, ptr(pred), s, s, s, C.byref(fx), C.byref(fx), 0, 0, C.byref(cp), bd)
        cp.do_average = 1
        ref.svt_av1_highbd_jnt_convolve_2d_copy_c(el(r1, pad + y + mv[3], pad + x + mv[2]), st, ptr(pred), s, s, s, C.byref(fx), C.byref(fx), 0, 0, C.byref(cp), bd)
        e = ref.sad_16b_kernel_c(el(src, y, x), W, ptr(pred), s, s, s)
        g = orc.orc_md_fullpel_avg_candidate16(ptr(src), W, el(r0, pad, pad), st, el(r1, pad, pad), st, x, y, s, s, mv[0], mv[1], mv[2], mv[3], bd)
        assert e == g, ("compound", it, x, y, s, mv)


def test_md_fullpel_candidate(orc, ref):
    """oracle/md_oracle.c vs the two reference kernels fast_loop_core (EbProductCodingLoop.c:907) runs for a full-pel single-reference candidate: the prediction
    svt_av1_convolve_2d_copy_sr_c (what svt_inter_predictor's table holds at [0][0][0]) and the distortion svt_nxm_sad_kernel_helper_c (= svt_nxm_sad_kernel_sub_sampled's
    C pointer, aom_dsp_rtcd.c:372).  Then the table form against its own per-candidate function."""
    import md_common as M
    rng = np.random.default_rng(31)
    orc.orc_md_fullpel_candidate.restype = C.c_uint32
    ref.svt_nxm_sad_kernel_helper_c.restype = C.c_uint32
    cp = _ConvP(); cp.round_0 = 3; cp.round_1 = 11
    fx = _IFP(C.addressof((C.c_int16 * 8 * 16).in_dll(ref, REF_BANKS[0])), 8, 16, 0)
    pad = 48
    src = rng.integers(0, 256, (192, 256), dtype=np.uint8)
    refp = rng.integers(0, 256, (192 + 2 * pad, 256 + 2 * pad), dtype=np.uint8)
    refp[pad:pad + 64, pad:pad + 64] = 255; src[:64, :64] = 0
    for it in range(200):
        s = int(rng.choice([8, 16, 32, 64]))
        x = int(rng.integers(0, (256 - s) // 8 + 1)) * 8; y = int(rng.integers(0, (192 - s) // 8 + 1)) * 8
        mx, my = (0, 0) if it < 4 else (int(rng.integers(-40, 41)), int(rng.integers(-40, 41)))
        if it < 4: x = y = 0; s = 64
        pred = np.zeros((s, s), np.uint8)
        rp = C.c_void_p(refp.ctypes.data + (pad + y + my) * refp.shape[1] + pad + x + mx)
        ref.svt_av1_convolve_2d_copy_sr_c(rp, refp.shape[1], ptr(pred), s, s, s, C.byref(fx), C.byref(fx), 0, 0, C.byref(cp))
        e = ref.svt_nxm_sad_kernel_helper_c(C.c_void_p(src.ctypes.data + y * 256 + x), 256, ptr(pred), s, s, s)
        g = orc.orc_md_fullpel_candidate(ptr(src), 256, C.c_void_p(refp.ctypes.data + pad * refp.shape[1] + pad), refp.shape[1], x, y, s, s, mx, my)
        assert e == g, (it, x, y, s, mx, my)
    # the table: every computed slot equals the per-candidate function, every other slot says so
    src2, refs, pus, mv, sb_cols, n_sb, pad2 = M.make_case(rng, 200, 152, 3)
    tab = M.oracle_table(orc, src2, refs, pus, mv, sb_cols, n_sb, pad2, 200, 152)
    n_done = 0
    for sb in range(n_sb):
        for p, (px, py, pw, ph) in enumerate(pus):
            for r in range(3):
                x, y = (sb % sb_cols) * 64 + px, (sb // sb_cols) * 64 + py
                mx = int(np.int16(mv[sb, p, r] & 0xffff)); my = int(np.int16(mv[sb, p, r] >> 16))
                inside = x + pw <= 200 and y + ph <= 152 and mx != -32768 and x + mx >= -pad2 and y + my >= -pad2 and x + mx + pw + 4 <= refs[r].shape[1] - pad2 and y + my + ph <= refs[r].shape[0] - pad2
                if not inside:
                    assert tab[sb, p, r] == 0xffffffff
                    continue
                n_done += 1
                assert tab[sb, p, r] == orc.orc_md_fullpel_candidate(ptr(src2), src2.shape[1], C.c_void_p(refs[r].ctypes.data + pad2 * refs[r].shape[1] + pad2), refs[r].shape[1],
                                                                     x, y, pw, ph, mx, my)
    assert n_done > 1000


# ------------------------------------------------------------------------------------ transforms
import txfm_common as tc


def test_txfm_tables_and_1d(orc, ref):
    """cospi table == reference's; every 1-D kernel (fdct/idct 4..64, fadst/iadst 4..16) bit-exact
    (mirrors /root/reference/test/FwdTxfm1dTest.cc / InvTxfm1dTest.cc input ranges)."""
    orc.orc_cospi_arr.restype = C.POINTER(C.c_int32)
    t = (C.c_int32 * 64 * 7).in_dll(ref, "eb_av1_cospi_arr_data")
    for bit in range(10, 17):
        assert np.array_equal(np.ctypeslib.as_array(orc.orc_cospi_arr(bit), (64,)), np.array(t[bit - 10]))
    rng = np.random.default_rng(0)
    for n in (4, 8, 16, 32, 64):
        for bit in (10, 11, 12, 13):
            sr = (C.c_int8 * 12)(*([16] * 12))
            for _ in range(30):
                x = rng.integers(-(1 << 17), 1 << 17, n, dtype=np.int32)
                a, b = np.zeros(n, np.int32), np.zeros(n, np.int32)
                getattr(ref, f"svt_av1_fdct{n}_new")(ptr(x), ptr(a), C.c_int8(bit), sr)
                orc.orc_fdct(ptr(x), ptr(b), n, bit)
                assert np.array_equal(a, b), ("fdct", n, bit)
        for cb in (16, 18):
            sr = (C.c_int8 * 12)(*([cb] * 12))
            for _ in range(30):
                x = rng.integers(-(1 << (cb - 1)), 1 << (cb - 1), n, dtype=np.int32)
                a, b = np.zeros(n, np.int32), np.zeros(n, np.int32)
                getattr(ref, f"svt_av1_idct{n}_new")(ptr(x), ptr(a), C.c_int8(12), sr)
                orc.orc_idct(ptr(x), ptr(b), n, 12, cb)
                assert np.array_equal(a, b), ("idct", n, cb)
    for n in (4, 8, 16):
        sr = (C.c_int8 * 12)(*([16] * 12))
        for bit in (12, 13):
            for it in range(30):
                x = rng.integers(-(1 << 16), 1 << 16, n, dtype=np.int32)
                if it == 0: x[:] = 0
                a, b = np.zeros(n, np.int32), np.zeros(n, np.int32)
                getattr(ref, f"svt_av1_fadst{n}_new")(ptr(x), ptr(a), C.c_int8(bit), sr)
                orc.orc_fadst(ptr(x), ptr(b), n, bit)
                assert np.array_equal(a, b), ("fadst", n, bit)
                getattr(ref, f"svt_av1_iadst{n}_new")(ptr(x), ptr(a), C.c_int8(12), sr)
                orc.orc_iadst(ptr(x), ptr(b), n, 12, 16)
                assert np.array_equal(a, b), ("iadst", n)


def test_txfm_2d_all_sizes_types(orc, ref):
    """All 19 sizes x legal types x bd 8/10, inputs +-(2^bd-1) incl. the extreme patterns
    (/root/reference/test/FwdTxfm2dAsmTest.cc:153-454); inverse fed with the forward output and with
    random coefficients (/root/reference/test/InvTxfm2dAsmTest.cc:436-470, :691-760)."""
    rng = np.random.default_rng(13596)
    orc.orc_handle_transform.restype = C.c_uint64
    for ts in range(19):
        w, h = tc.TXW[ts], tc.TXH[ts]
        kw, kh = min(w, 32), min(h, 32)
        for tt in tc.legal_types(ts):
            for bd in (8, 10):
                for it in range(4):
                    lim = (1 << bd) - 1
                    x = rng.integers(-lim, lim + 1, (h, w + 3), dtype=np.int16)
                    if it == 0: x[:] = lim
                    if it == 1: x[:] = -lim
                    a = tc.ref_fwd(ref, x, w + 3, tt, ts, bd)
                    b = tc.orc_fwd(orc, x, w + 3, tt, ts, bd)
                    assert np.array_equal(a, b), ("fwd", ts, tt, bd, it)
                    if max(w, h) == 64:
                        ea = tc.ref_handle(ref, a, ts)
                        eb = orc.orc_handle_transform(ptr(b), ts)
                        assert ea == eb and np.array_equal(a[:kw * kh], b[:kw * kh]), ("handle", ts)
                    co = np.ascontiguousarray((a[:kw * kh] // 5) * 5).astype(np.int32)
                    if it == 2:
                        co = rng.integers(-(1 << (bd + 7)), 1 << (bd + 7), kw * kh, dtype=np.int32)
                    pred = rng.integers(0, 1 << bd, (h, w + 5), dtype=np.uint16)
                    r1 = np.zeros((h, w + 7), np.uint16); r2 = np.zeros((h, w + 7), np.uint16)
                    tc.ref_inv(ref, co, pred, w + 5, r1, w + 7, tt, ts, bd)
                    orc.orc_inv_txfm2d_add(ptr(co), ptr(pred), w + 5, ptr(r2), w + 7, tt, ts, bd)
                    assert np.array_equal(r1, r2), ("inv", ts, tt, bd, it)


def test_estimate_transform_coeff_shapes(orc, ref):
    """av1_estimate_transform (EbTransforms.c:3613) with every EB_TRANS_COEFF_SHAPE (DEFAULT / N2 / N4 / ONLY_DC): the packed coefficient
    block and three_quad_energy, all 19 sizes x legal types x bd 8 / 10.  The output buffer is pre-filled with garbage: the N2 / N4
    functions must write the zeros themselves."""
    orc.orc_estimate_transform.restype = C.c_uint64
    rng = np.random.default_rng(33)
    for ts in range(19):
        w, h = tc.TXW[ts], tc.TXH[ts]
        kw, kh = min(w, 32), min(h, 32)
        for bd in (8, 10):
            for tt in tc.legal_types(ts):
                res = rng.integers(-(1 << bd) + 1, 1 << bd, (h, w + 3)).astype(np.int16)
                for shape in range(4):
                    exp = np.full(w * h, 0x5A5A5A, np.int32)
                    e_en = C.c_uint64(0)
                    assert ref.av1_estimate_transform(ptr(res), w + 3, ptr(exp), w, ts, C.byref(e_en), bd, tt, 0, shape) == 0
                    got = np.zeros(kw * kh, np.int32)
                    g_en = orc.orc_estimate_transform(ptr(res), w + 3, ptr(got), tt, ts, bd, shape)
                    assert np.array_equal(got, exp[:kw * kh]), (tc.TX_NAMES[ts], bd, tt, shape)
                    assert g_en == e_en.value, (tc.TX_NAMES[ts], bd, tt, shape, g_en, e_en.value)
                    if shape == 3: assert not got[1:].any()


def test_quantize_variants(orc, ref):
    """quantize_b (8-bit c_ii), highbd_quantize_b, quantize_fp (3 scales), highbd_quantize_fp vs the
    reference across q-index, sizes and coefficient ranges +-2^(7+bd)
    (/root/reference/test/QuantAsmTest.cc:88-335, quantize_func_test.cc:276-658)."""
    rng = np.random.default_rng(42)
    orc.orc_cul_level.restype = C.c_int32
    for ts in (0, 1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17):
        ls = tc.TX_SCALE[ts]
        for tt in (0, 10, 11):
            if tt not in tc.legal_types(ts) and tt != 0:
                continue
            scan, iscan = tc.ref_scan(ref, ts, tt)
            n = len(scan)
            assert np.array_equal(iscan[scan], np.arange(n))
            for bd, variants in ((8, (0, 2)), (10, (1, 3))):
                for qindex in (0, 1, 20, 60, 120, 200, 255):
                    qp = tc.ref_qparams(ref, bd, qindex, int(rng.integers(0, 3)))
                    for it in range(3):
                        lim = 1 << (7 + bd)
                        coeff = rng.integers(-lim, lim + 1, n, dtype=np.int32)
                        if it == 1: coeff = (coeff // 64).astype(np.int32)      # mostly inside the dead zone
                        if it == 2: coeff[rng.integers(0, n, n // 2)] = 0
                        for v in variants:
                            a = tc.ref_quant(ref, v, coeff, qp, scan, iscan, ls)
                            b = tc.orc_quant(orc, v, coeff, qp, scan, ls)
                            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], (ts, tt, bd, qindex, v)


# ------------------------------------------------------------------------------------ deblocking
def test_deblock_edge_filters(orc, ref):
    """All 16 edge filters (lbd/hbd x 4/6/8/14 x h/v) on random and smooth data
    (/root/reference/test/DeblockTest.cc:210-306)."""
    rng = np.random.default_rng(99)
    for bd, dt in FMT3:
        hbd = dt == np.uint16
        for length in (4, 6, 8, 14):
            for d, dname in ((0, "vertical"), (1, "horizontal")):
                name = f"svt_aom_{'highbd_' if hbd else ''}lpf_{dname}_{length}_c"
                for it in range(300):
                    base = rng.integers(0, 1 << bd)
                    spread = int(rng.choice([1, 2, 4, 16, 64, 1 << bd]))
                    buf = np.clip(base + rng.integers(-spread, spread + 1, (24, 24)), 0, (1 << bd) - 1).astype(dt)
                    a, b = buf.copy(), buf.copy()
                    bl = np.full(16, rng.integers(0, 256), np.uint8); li = np.full(16, rng.integers(0, 64), np.uint8)
                    th = np.full(16, rng.integers(0, 16), np.uint8)
                    off = 10 * 24 + 10
                    pa = C.c_void_p(a.ctypes.data + off * a.itemsize); pb = C.c_void_p(b.ctypes.data + off * b.itemsize)
                    if hbd:
                        getattr(ref, name)(pa, 24, ptr(bl), ptr(li), ptr(th), bd)
                    else:
                        getattr(ref, name)(pa, 24, ptr(bl), ptr(li), ptr(th))
                    orc.orc_lpf_edge(pb, a.itemsize, 24, d, length, int(bl[0]), int(li[0]), int(th[0]), bd)
                    assert np.array_equal(a, b), (name, it)


# ------------------------------------------------------------------------------------------ CDEF
import cdef_common as cc


def test_deblocking_edges_of_a_frame(orc, ref):
    """E2, pinned below the whole-encode level: the reference's svt_av1_loop_filter_frame runs on synthetic pictures -- random AV1 partitions with every
    block size, transform depths, intra / inter, skip, modes, per-reference and per-mode level deltas, 64 and 128 superblocks, coded sizes with padding -- with the edge
    filters replaced by recorders (oracle/ref_shim.c: ref_shim_dlf_frame_edges), and the oracle's restatement (level table of svt_av1_loop_filter_frame_init, the per-unit
    summary = get_transform_size, set_lpf_parameters, the unit ranges of the frame loop) must name exactly the same edges, lengths and levels."""
    import dlf_common as D
    rng = np.random.default_rng(2024)
    P3 = C.POINTER(C.c_uint16) * 3
    cases = [(64, 64, 0, 0, 64), (200, 136, 0, 0, 64), (136, 72, 6, 6, 64), (192, 128, 6, 6, 64), (384, 256, 0, 0, 128), (328, 200, 0, 0, 128), (72, 72, 8, 8, 64), (264, 136, 2, 4, 128)]
    n_edges = 0
    for ci, (w, h, pr, pb, sb) in enumerate(cases):
        for it in range(4):
            f = D.make_reference_mode_info(rng, w, h, sb, p_skip=(0.2, 0.5, 0.9, 0.4)[it], p_inter=(0.7, 0.95, 0.5, 0.0)[it])
            lf = [int(rng.integers(0, 64)), int(rng.integers(0, 64)), int(rng.integers(0, 64)), int(rng.integers(0, 64)), int(rng.integers(0, 8)), it % 2] + \
                 [int(v) for v in rng.integers(-20, 21, 8)] + [int(v) for v in rng.integers(-20, 21, 2)]
            if it == 3: lf[2] = 0                      # a chroma plane that is not filtered at all
            if ci == 0 and it == 2: lf[0] = lf[1] = 0  # no luma level: the reference stops at plane 0 (loop_filter_sb's `break`)
            summ, edges, lvl = D.oracle_edges(orc, f, w, h, lf, pr, pb, sb)
            ev = [np.zeros_like(e[0]) for e in edges]; eh = [np.zeros_like(e[1]) for e in edges]
            rl = np.zeros((3, 2, 8, 2), np.uint8)
            bad = ref.ref_shim_dlf_frame_edges(w, h, pr, pb, sb, ptr(f["sb_type"]), ptr(f["tx_depth"]), ptr(f["ref_frame0"]), ptr(f["skip"]), ptr(f["mode"]),
                                               ptr(np.array(lf, np.int32)), P3(*[e.ctypes.data_as(C.POINTER(C.c_uint16)) for e in ev]),
                                               P3(*[e.ctypes.data_as(C.POINTER(C.c_uint16)) for e in eh]), ptr(rl))
            assert bad == 0
            luma_off = lf[0] == 0 and lf[1] == 0
            for plane in range(3):
                on = not luma_off and (plane == 0 or lf[1 + plane] != 0)   # svt_av1_loop_filter_frame_init / loop_filter_sb skip these planes (and everything after an unfiltered luma)
                if on:
                    # the level table, where the reference's init wrote it and the summary reads it (intra: [0][0] only)
                    assert np.array_equal(rl[plane, :, 1:, :], lvl[plane, :, 1:, :]) and np.array_equal(rl[plane, :, 0, 0], lvl[plane, :, 0, 0]), (ci, it, plane)
                    assert np.array_equal(ev[plane], edges[plane][0]), (ci, it, plane, "v", np.argwhere(ev[plane] != edges[plane][0])[:5])
                    assert np.array_equal(eh[plane], edges[plane][1]), (ci, it, plane, "h", np.argwhere(eh[plane] != edges[plane][1])[:5])
                    n_edges += int((ev[plane] != 0).sum() + (eh[plane] != 0).sum())
                else:
                    assert not ev[plane].any() and not eh[plane].any()
    assert n_edges > 20000


def test_cdef_find_dir_and_filter_block(orc, ref):
    """svt_cdef_find_dir_c and svt_cdef_filter_block_c for every direction / strength / damping / block
    size / bit depth, with CDEF_VERY_LARGE borders (/root/reference/test/CdefTest.cc:342-590)."""
    rng = np.random.default_rng(3)
    for cs in (0, 2):
        for it in range(200):
            img = rng.integers(0, 256 << cs, (8, 8), dtype=np.uint16)
            if it % 3 == 0:
                yy, xx = np.mgrid[0:8, 0:8]; img = (((xx * (it % 5) + yy * (it % 7)) * 9) % (256 << cs)).astype(np.uint16)
            v1, v2 = C.c_int32(0), C.c_int32(0)
            d1 = ref.svt_cdef_find_dir_c(ptr(img), 8, C.byref(v1), cs)
            d2 = orc.orc_cdef_find_dir(ptr(img), 8, C.byref(v2), cs)
            assert (d1, v1.value) == (d2, v2.value)
    for cs in (0, 2):
        for bsize, (bw, bh) in ((3, (8, 8)), (0, (4, 4))):
            for it in range(400):
                buf = rng.integers(0, 256 << cs, (8 + 6, cc.BSTRIDE), dtype=np.uint16)
                if it % 4 == 0: buf[:3] = cc.VERY_LARGE
                if it % 4 == 1: buf[:, :8] = cc.VERY_LARGE
                if it % 4 == 2: buf[3 + bh:] = cc.VERY_LARGE; buf[:, 8 + bw:] = cc.VERY_LARGE
                pri = int(rng.integers(0, 16)) << cs; sec = int(rng.choice([0, 1, 2, 4])) << cs
                d = int(rng.integers(0, 8)); pd = int(rng.integers(3, 7)) + cs; sd = int(rng.integers(3, 7)) + cs
                inp = C.c_void_p(buf.ctypes.data + 2 * (3 * cc.BSTRIDE + 8))
                a = np.zeros((8, 8), np.uint16); b = np.zeros((8, 8), np.uint16)
                ref.svt_cdef_filter_block_c(None, ptr(a), 8, inp, pri, sec, d, pd, sd, bsize, cs)
                orc.orc_cdef_filter_block(None, ptr(b), 8, inp, cc.BSTRIDE, pri, sec, d, pd, sd, bw, bh, cs)
                assert np.array_equal(a, b), (cs, bsize, it)


def test_cdef_search_filter_block_level(orc, ref):
    """Whole filter-block strength search (64 strengths x 3 planes incl. the FP64 luma distortion) vs
    svt_cdef_filter_fb + compute_cdef_dist* driven like cdef_seg_search; multi-fb frame so that inner
    and picture-edge halos are both exercised."""
    for bd, dt in FMT3:
        src, rec, skip8 = cc.make_frame(144, 80, bd, seed=bd, dtype=dt)   # 3 x 2 fbs, ragged right/bottom fb (16 px)
        mse = cc.orc_search(orc, rec, src, bd, skip8, 5)
        nh = 3
        for fbr in range(2):
            for fbc in range(3):
                r = cc.ref_search_fb(ref, rec, src, bd, skip8, fbr, fbc, 5)
                if r is None:
                    continue
                assert np.array_equal(r[0], mse[0, fbr * nh + fbc]), ("Y", bd, fbr, fbc)
                assert np.array_equal(r[1], mse[1, fbr * nh + fbc]), ("UV", bd, fbr, fbc)


def test_cdef_search_chart(orc, ref):
    """The same on the direction chart (cdef_common.make_chart_frame: every direction, flat blocks, exact cost ties, saturated samples at the picture
    edge, anti-correlated source), dampings 3-6.  208 x 144: ref_search_fb cannot stage an 8-sample-wide last filter block."""
    for bd, dt in FMT3:
        src, rec, skip8 = cc.make_chart_frame(208, 144, bd, cc.CHART_SEED, dt)
        for damping in (3, 4, 5, 6):
            mse = cc.orc_search(orc, rec, src, bd, skip8, damping)
            seen = 0
            for fb in range(12):
                r = cc.ref_search_fb(ref, rec, src, bd, skip8, fb // 4, fb % 4, damping)
                if r is None:
                    assert not mse[:, fb].any()
                    continue
                seen += 1
                assert np.array_equal(r[0], mse[0, fb]), ("Y", bd, damping, fb)
                assert np.array_equal(r[1], mse[1, fb]), ("UV", bd, damping, fb)
            assert seen == 11


def test_cdef_apply_chart(orc, ref):
    """orc_cdef_apply_frame vs svt_cdef_filter_fb driven like svt_av1_cdef_frame (cdef_common.ref_apply_fb) on the direction chart: strengths 0 / 0,
    luma off / chroma on, chroma off / luma on, 63 / 63 and secondary index 3 each meet another filter block at every damping."""
    pairs = set()
    for bd, dt in FMT3:
        src, rec, skip8 = cc.make_chart_frame(208, 144, bd, cc.CHART_SEED, dt)
        for damping in (3, 4, 5, 6):
            ys, uvs = cc.chart_strengths(12, damping)
            pairs |= set(zip(ys.tolist(), uvs.tolist()))
            exp = cc.orc_apply(orc, rec, bd, skip8, ys, uvs, damping)
            got = [p.copy() for p in rec]
            for fb in range(12):
                cc.ref_apply_fb(ref, rec, got, bd, skip8, fb // 4, fb % 4, int(ys[fb]), int(uvs[fb]), damping)
            for pli in range(3):
                assert (got[pli] != rec[pli]).any()
                assert np.array_equal(got[pli], exp[pli]), (bd, damping, pli, np.argwhere(got[pli] != exp[pli])[:5])
    assert {(0, 0), (63, 63), (3, 3)} <= pairs and any(y == 0 and uv for y, uv in pairs) and any(uv == 0 and y for y, uv in pairs)


# ----------------------------------------------------------------------- sub-pel convolve / variance
class _IFP(C.Structure):
    _fields_ = [("filter_ptr", C.c_void_p), ("taps", C.c_uint16), ("subpel_shifts", C.c_uint16), ("interp_filter", C.c_uint8)]


class _ConvP(C.Structure):
    _fields_ = [("ref", C.c_int32), ("do_average", C.c_int32), ("dst", C.c_void_p), ("dst_stride", C.c_int32), ("round_0", C.c_int32),
                ("round_1", C.c_int32), ("plane", C.c_int32), ("is_compound", C.c_int32), ("use_jnt_comp_avg", C.c_int32),
                ("fwd_offset", C.c_int32), ("bck_offset", C.c_int32), ("use_dist_wtd_comp_avg", C.c_int32)]


REF_BANKS = ["sub_pel_filters_8", "sub_pel_filters_8smooth", "sub_pel_filters_8sharp", "bilinear_filters", "sub_pel_filters_4", "sub_pel_filters_4smooth"]


def test_interp_kernels_and_convolve_sr(orc, ref):
    """Kernel tables == the reference's; convolve copy/x/y/2d for all 16x16 phases, lbd + hbd
    (/root/reference/test/convolve_2d_test.cc:785-1040)."""
    mine = np.ctypeslib.as_array((C.c_int16 * 8 * 16 * 6).in_dll(orc, "orc_interp_kernels"))
    for b, name in enumerate(REF_BANKS):
        assert np.array_equal(mine[b], np.ctypeslib.as_array((C.c_int16 * 8 * 16).in_dll(ref, name))), name
    rng = np.random.default_rng(2)
    cp = _ConvP(); cp.round_0 = 3; cp.round_1 = 11
    for bd, dt, pre in ((8, np.uint8, "svt_av1_"), (10, np.uint16, "svt_av1_highbd_"), (8, np.uint16, "svt_av1_highbd_")):
        for it in range(300):
            w = int(rng.choice([4, 8, 16, 32, 64, 128])); h = int(rng.choice([4, 8, 16, 32, 64, 128]))
            bx = int(rng.integers(0, 6)); by_ = int(rng.integers(0, 6))
            sx, sy = int(rng.integers(0, 16)), int(rng.integers(0, 16))
            if it % 5 == 0: sx = 0
            if it % 7 == 0: sy = 0
            src = rng.integers(0, 1 << bd, (h + 16, w + 24)).astype(dt)
            if it % 11 == 0: src[:] = (1 << bd) - 1
            if dt == np.uint16 and bd == 8 and it % 11 == 1: src[:] = rng.integers(0, 2, src.shape) * 255      # binary 0 / 255: the filters overshoot both ends
            a = np.zeros((h, w + 3), dt); b = np.zeros((h, w + 3), dt)
            fx = _IFP(C.addressof((C.c_int16 * 8 * 16).in_dll(ref, REF_BANKS[bx])), 8, 16, 0)
            fy = _IFP(C.addressof((C.c_int16 * 8 * 16).in_dll(ref, REF_BANKS[by_])), 8, 16, 0)
            name = pre + "convolve_" + {(0, 0): "2d_copy", (1, 0): "x", (0, 1): "y", (1, 1): "2d"}[(int(sx != 0), int(sy != 0))] + "_sr_c"
            sp = C.c_void_p(src.ctypes.data + (8 * src.shape[1] + 8) * src.itemsize)
            args = [sp, src.shape[1], ptr(a), a.shape[1], w, h, C.byref(fx), C.byref(fy), sx, sy, C.byref(cp)]
            if dt == np.uint16: args.append(bd)
            getattr(ref, name)(*args)
            orc.orc_convolve_sr(sp, src.shape[1], ptr(b), b.shape[1], src.itemsize, w, h, bx, by_, sx, sy, bd)
            assert np.array_equal(a, b), (name, w, h, sx, sy)


def test_upsampled_pred_and_variance(orc, ref):
    """svt_aom_upsampled_pred_c (2/4/8-tap) and the block variances (lbd + highbd_10)
    (/root/reference/test/VarianceTest.cc:129-401, HbdVarianceTest.cc:295-700)."""
    rng = np.random.default_rng(8)
    for it in range(200):
        w = int(rng.choice([4, 8, 16, 32, 64])); h = int(rng.choice([4, 8, 16, 32, 64]))
        sx, sy = int(rng.integers(0, 8)), int(rng.integers(0, 8))
        search = int(rng.integers(0, 3))   # USE_2_TAPS, USE_4_TAPS, USE_8_TAPS
        bank = [3, 4, 0][search]
        src = rng.integers(0, 256, (h + 20, w + 24)).astype(np.uint8)
        sp = C.c_void_p(src.ctypes.data + 8 * src.shape[1] + 8)
        a = np.zeros(w * h, np.uint8); b = np.zeros(w * h, np.uint8)
        ref.svt_aom_upsampled_pred_c(None, None, 0, 0, None, ptr(a), w, h, sx, sy, sp, src.shape[1], search + 1)  # USE_2_TAPS = 1
        orc.orc_upsampled_pred(sp, src.shape[1], ptr(b), w, h, sx, sy, bank)
        assert np.array_equal(a, b), (w, h, sx, sy, search)
    orc.orc_variance.restype = C.c_uint32; orc.orc_variance_hbd10.restype = C.c_uint32
    for (w, h) in ((4, 4), (8, 8), (16, 16), (16, 32), (32, 16), (64, 64), (8, 32), (64, 16)):
        for it in range(40):
            for bd, dt in ((8, np.uint8), (10, np.uint16)):
                a = rng.integers(0, 1 << bd, (h, w + 5)).astype(dt); b = rng.integers(0, 1 << bd, (h, w + 9)).astype(dt)
                if it == 0: a[:] = 0; b[:] = (1 << bd) - 1
                if it == 1: b[:, :w] = a[:, :w]
                s1, s2 = C.c_uint32(0), C.c_uint32(0)
                if bd == 8:
                    f = getattr(ref, f"svt_aom_variance{w}x{h}_c"); f.restype = C.c_uint32
                    v1 = f(ptr(a), a.shape[1], ptr(b), b.shape[1], C.byref(s1))
                    v2 = orc.orc_variance(ptr(a), a.shape[1], ptr(b), b.shape[1], w, h, C.byref(s2))
                else:
                    f = getattr(ref, f"svt_aom_highbd_10_variance{w}x{h}_c"); f.restype = C.c_uint32
                    v1 = f(C.c_void_p(a.ctypes.data >> 1), a.shape[1], C.c_void_p(b.ctypes.data >> 1), b.shape[1], C.byref(s1))   # CONVERT_TO_BYTEPTR
                    v2 = orc.orc_variance_hbd10(ptr(a), a.shape[1], ptr(b), b.shape[1], w, h, C.byref(s2))
                assert (v1, s1.value) == (v2, s2.value), (w, h, bd, it)


# -------------------------------------------------------------------------- pyramids (HME inputs)
def test_sad_x4d_and_mse16x16(orc, ref):
    """svt_aom_sad{W}x{H}x4d (four references = four block pairs of the batch SAD, EbComputeSAD_C.c:118-135) and svt_aom_mse16x16 (EbPsnr.c:84) /
    svt_aom_highbd_8_mse16x16 (C_DEFAULT/variance.c:381): the variance / sse outputs of a 16x16 pair, against the oracle's SAD / variance."""
    rng = np.random.default_rng(61)
    orc.orc_nxm_sad.restype = C.c_uint32; orc.orc_variance.restype = C.c_uint32
    for (w, h) in ((4, 4), (8, 16), (16, 16), (32, 8), (64, 64), (128, 64), (64, 128), (128, 128)):
        src = rng.integers(0, 256, (h, w + 5)).astype(np.uint8)
        refs = [rng.integers(0, 256, (h, w + 9)).astype(np.uint8) for _ in range(4)]
        pa = (C.c_void_p * 4)(*[r.ctypes.data for r in refs])
        out = (C.c_uint32 * 4)()
        getattr(ref, f"svt_aom_sad{w}x{h}x4d_c")(ptr(src), w + 5, pa, w + 9, out)
        for k in range(4):
            assert out[k] == orc.orc_nxm_sad(ptr(src), w + 5, ptr(refs[k]), w + 9, h, w) == getattr(ref, f"svt_aom_sad{w}x{h}_c")(ptr(src), w + 5, ptr(refs[k]), w + 9)
    a = rng.integers(0, 256, (16, 21)).astype(np.uint8); b = rng.integers(0, 256, (16, 19)).astype(np.uint8)
    e_sse, g_sse = C.c_uint32(), C.c_uint32()
    ref.svt_aom_mse16x16_c.restype = C.c_uint32
    e_var = ref.svt_aom_mse16x16_c(ptr(a), 21, ptr(b), 19, C.byref(e_sse))   # EbPsnr.c:84: a 16x16 variance; get_sse() reads *sse
    assert orc.orc_variance(ptr(a), 21, ptr(b), 19, 16, 16, C.byref(g_sse)) == e_var
    assert g_sse.value == e_sse.value
    a16, b16 = a.astype(np.uint16), b.astype(np.uint16)
    ref.svt_aom_highbd_8_mse16x16_c(C.c_void_p(a16.ctypes.data >> 1), 21, C.c_void_p(b16.ctypes.data >> 1), 19, C.byref(e_sse))   # CONVERT_TO_BYTEPTR
    assert g_sse.value == e_sse.value


def test_downsample_and_mean_kernels(orc, ref):
    """decimation_2d / downsample_2d and the 8x8 mean / mean-of-squares kernels behind the variance
    pyramid (/root/reference/test/compute_mean_test.cc:83-165)."""
    rng = np.random.default_rng(12)
    for step in (2, 4):
        for filt, name in ((0, "decimation_2d"), (1, "downsample_2d")):
            img = rng.integers(0, 256, (72, 104), dtype=np.uint8)
            a = np.zeros((72 // step, 104 // step + 3), np.uint8); b = a.copy()
            getattr(ref, name)(ptr(img), 104, 96, 64, ptr(a), a.shape[1], step)
            orc.orc_downsample_2d(ptr(img), 104, 96, 64, ptr(b), b.shape[1], step, filt)
            assert np.array_equal(a, b), (name, step)
    ref.svt_compute_sub_mean_8x8_c.restype = C.c_uint64
    ref.svt_compute_mean_squared_values_c.restype = C.c_uint64
    for it in range(50):
        sb = rng.integers(0, 256, (64, 80), dtype=np.uint8)
        if it == 0: sb[:] = 255
        if it == 1: sb[:] = 0
        for full in (0, 1):
            mean = np.zeros(85, np.uint8); var = np.zeros(85, np.uint16)
            orc.orc_variance_pyramid_sb(ptr(sb), 80, full, ptr(mean), ptr(var))
            # 8x8 level against the reference's kernels (raster order)
            for b in range(64):
                p = C.c_void_p(sb.ctypes.data + (b >> 3) * 8 * 80 + (b & 7) * 8)
                if full:
                    blk = sb[(b >> 3) * 8:(b >> 3) * 8 + 8, (b & 7) * 8:(b & 7) * 8 + 8].astype(np.uint64)
                    m = (int(blk.sum()) << 8) // 64
                    q = ref.svt_compute_mean_squared_values_c(p, 80, 8, 8)
                else:
                    m = ref.svt_compute_sub_mean_8x8_c(p, C.c_uint16(80))
                    mm = (C.c_uint64 * 4)(); qq = (C.c_uint64 * 4)()
                    if (b & 3) == 0:
                        ref.svt_compute_interm_var_four8x8_c(p, C.c_uint16(80), mm, qq)
                        assert mm[0] == m
                        q = qq[0]
                    else:
                        continue
                assert mean[21 + b] == (m >> 8) & 0xFF and var[21 + b] == ((q - m * m) >> 16) & 0xFFFF, (it, full, b)


# ------------------------------------------------------------------------ self-guided restoration
class _SgrP(C.Structure):
    _fields_ = [("r", C.c_int32 * 2), ("s", C.c_int32 * 2)]


def test_sgr_tables_filter_apply_and_projection(orc, ref):
    """Tables, the two box filters for all 16 parameter sets (lbd/hbd), apply, projection sums/solve and
    projection error (/root/reference/test/selfguided_filter_test.cc:248-562, RestorationPickTest.cc)."""
    prm = np.ctypeslib.as_array((C.c_int32 * 4 * 16).in_dll(orc, "orc_sgr_params"))
    rp = np.ctypeslib.as_array((C.c_int32 * 4 * 16).in_dll(ref, "eb_sgr_params"))      # {r[2], s[2]}
    assert np.array_equal(prm, rp)
    xt = np.ctypeslib.as_array((C.c_int32 * 256).in_dll(ref, "eb_x_by_xplus1")); ot = np.ctypeslib.as_array((C.c_int32 * 25).in_dll(ref, "eb_one_by_x"))
    assert [orc.orc_x_by_xplus1(z) for z in range(256)] == list(xt) and [orc.orc_one_by_x(n) for n in range(1, 26)] == list(ot)
    rng = np.random.default_rng(21)
    orc.orc_sgr_proj_error.restype = C.c_int64
    ref.svt_av1_lowbd_pixel_proj_error_c.restype = C.c_int64; ref.svt_av1_highbd_pixel_proj_error_c.restype = C.c_int64
    for bd, dt in FMT3:
        hb = int(dt == np.uint16)
        for it in range(24):
            ep = it % 16
            w, h = int(rng.choice([64, 40, 8, 64])), int(rng.choice([64, 56, 24, 8]))
            mode = it % 3
            base = rng.integers(0, 1 << bd, (h + 6, w + 10)) if mode == 0 else (np.full((h + 6, w + 10), (1 << bd) - 1) if mode == 1 else
                                                                                 (400 >> (10 - bd)) + rng.integers(-3, 4, (h + 6, w + 10)))
            dgd = np.clip(base, 0, (1 << bd) - 1).astype(dt)
            src = np.clip(dgd.astype(np.int32) + rng.integers(-12, 13, dgd.shape), 0, (1 << bd) - 1).astype(dt)
            st = dgd.shape[1]
            off = (3 * st + 3) * dgd.itemsize
            pd, ps = dgd.ctypes.data + off, src.ctypes.data + off
            cvt = (lambda a: C.c_void_p(a >> 1)) if hb else (lambda a: C.c_void_p(a))   # CONVERT_TO_BYTEPTR
            a0 = np.full((h, w), -7, np.int32); a1 = a0.copy(); b0 = a0.copy(); b1 = a0.copy()
            ref.svt_av1_selfguided_restoration_c(cvt(pd), w, h, st, ptr(a0), ptr(a1), w, ep, bd, hb)
            orc.orc_sgr_filter(C.c_void_p(pd), dgd.itemsize, w, h, st, ptr(b0), ptr(b1), w, ep, bd)
            assert np.array_equal(a0, b0) and np.array_equal(a1, b1), (bd, ep, it)
            # projection: sums -> solve vs svt_get_proj_subspace_c, then the projection error
            sp = _SgrP(); sp.r[0], sp.r[1], sp.s[0], sp.s[1] = [int(v) for v in prm[ep]]
            xq1 = (C.c_int32 * 2)(); xq2 = (C.c_int32 * 2)(); sums = (C.c_int64 * 5)()
            ref.svt_get_proj_subspace_c(cvt(ps), w, h, st, cvt(pd), st, hb, ptr(a0), w, ptr(a1), w, xq1, C.byref(sp))
            orc.orc_sgr_proj_sums(C.c_void_p(ps), st, C.c_void_p(pd), st, dgd.itemsize, w, h, ptr(b0), w, ptr(b1), w, ep, sums)
            orc.orc_sgr_solve(sums, w * h, ep, xq2)
            assert list(xq1) == list(xq2), (bd, ep, list(xq1), list(xq2))
            xq = (C.c_int32 * 2)(int(rng.integers(-96, 32)), int(rng.integers(-32, 96)))
            f = ref.svt_av1_highbd_pixel_proj_error_c if hb else ref.svt_av1_lowbd_pixel_proj_error_c
            e1 = f(cvt(ps), w, h, st, cvt(pd), st, ptr(a0), w, ptr(a1), w, xq, C.byref(sp))
            e2 = orc.orc_sgr_proj_error(C.c_void_p(ps), st, C.c_void_p(pd), st, dgd.itemsize, w, h, ptr(b0), w, ptr(b1), w, xq, ep)
            assert e1 == e2
            # apply
            xqd = (C.c_int32 * 2)(int(rng.integers(-96, 32)), int(rng.integers(-32, 96)))
            o1 = np.zeros((h, w), dt); o2 = np.zeros((h, w), dt)
            tmp = np.zeros(2 * 161 * 161 * 4 + 64, np.int32)
            ref.svt_apply_selfguided_restoration_c(cvt(pd), w, h, st, ep, xqd, cvt(o1.ctypes.data), w, ptr(tmp), bd, hb)
            orc.orc_sgr_apply(C.c_void_p(pd), dgd.itemsize, w, h, st, ep, xqd, ptr(o2), w, bd)
            assert np.array_equal(o1, o2), (bd, ep, "apply")


def test_sgr_finer_search_and_unit_search(orc, ref):
    """The per-unit self-guided search: finer_search_pixel_proj_error (EbRestorationPick.c:353) and search_selfguided_restoration (:583),
    both static in the reference and exported by oracle/ref_shim_restpick.c, vs the oracle's restatements.  Units of several shapes
    (luma 64-px and chroma 32-px processing units, ragged sizes), smooth + noisy content so that different sets win."""
    if not hasattr(ref, "ref_shim_sgr_search_unit"): pytest.skip("oracle/_ref predates ref_shim_restpick.c: rebuild it")
    orc.orc_sgr_finer_search.restype = C.c_int64; ref.ref_shim_sgr_finer_search.restype = C.c_int64
    rng = np.random.default_rng(91)
    rstbuf = np.zeros(ref.ref_shim_sgr_rstbuf_ints(), np.int32)
    for bd, dt in FMT3:
        hb = int(dt == np.uint16)
        cvt = (lambda a: C.c_void_p(a >> 1)) if hb else (lambda a: C.c_void_p(a))   # CONVERT_TO_BYTEPTR
        for it, (w, h, ss) in enumerate(((64, 64, 0), (96, 72, 0), (40, 56, 1), (128, 120, 0), (32, 32, 1), (72, 40, 1))):
            yy, xx = np.mgrid[0:h + 6, 0:w + 6]
            clean = (100 + 60 * np.sin(xx / (5.0 + it)) * np.cos(yy / 7.0) + 25 * (((xx + yy) // 9) % 2)) * (1 << (bd - 8))
            src = np.clip(clean, 0, (1 << bd) - 1).astype(dt)
            dgd = np.clip(clean + rng.normal(0, (2 + 3 * it) * (1 << (bd - 8)), clean.shape), 0, (1 << bd) - 1).astype(dt)
            st = w + 6; off = (3 * st + 3) * dgd.itemsize
            pd, ps = dgd.ctypes.data + off, src.ctypes.data + off
            pu = 64 >> ss
            # --- whole-unit search, all 16 sets (no reference-frame sets: ref_ep = -1, -1) and a window around a reference set
            for (e0, e1, step, mask) in ((-1, -1, 16, 0xFFFF), (6, -1, 1, 0x0060), (3, 12, 4, 0x0FF8)):
                out = (C.c_int32 * 3)()
                ref.ref_shim_sgr_search_unit(cvt(pd), w, h, st, cvt(ps), st, hb, bd, pu, pu, ptr(rstbuf), e0, e1, step, out)
                xqd = np.zeros((1, 16, 2), np.int32); err = np.zeros((1, 16), np.int64); best = np.zeros(1, np.uint8)
                # a single unit: the plane-level oracle with unit_size >= the plane (one unit; rows are not shifted for a 1-unit plane top)
                orc.orc_sgr_search_units_plane(C.c_void_p(pd), dgd.itemsize, st, C.c_void_p(ps), st, w, h, ss, ss, 256, bd, mask, ptr(xqd), ptr(err), ptr(best))
                assert (int(best[0]), int(xqd[0, best[0], 0]), int(xqd[0, best[0], 1])) == (out[0], out[1], out[2]), (bd, it, mask, list(out), best, xqd[0, best[0]])
            # --- the finer search on its own from arbitrary starting points (incl. the clamps of the tap range)
            for ep in (0, 5, 9, 10, 13, 14, 15):
                f0 = np.zeros((h, w + 8), np.int32); f1 = np.zeros_like(f0)
                for i in range(0, h, pu):
                    for j in range(0, w, pu):
                        orc.orc_sgr_filter(C.c_void_p(pd + (i * st + j) * dgd.itemsize), dgd.itemsize, min(pu, w - j), min(pu, h - i), st,
                                           C.c_void_p(f0.ctypes.data + (i * (w + 8) + j) * 4), C.c_void_p(f1.ctypes.data + (i * (w + 8) + j) * 4), w + 8, ep, bd)
                for start in ((-96, -32), (31, 95), (-20, 40), (0, 0), (-95, 94)):
                    a = (C.c_int32 * 2)(*start); b = (C.c_int32 * 2)(*start)
                    e1 = ref.ref_shim_sgr_finer_search(cvt(ps), w, h, st, cvt(pd), st, hb, ptr(f0), w + 8, ptr(f1), w + 8, 2, a, ep)
                    e2 = orc.orc_sgr_finer_search(C.c_void_p(ps), st, C.c_void_p(pd), st, dgd.itemsize, w, h, ptr(f0), w + 8, ptr(f1), w + 8, 2, b, ep)
                    assert (e1, list(a)) == (e2, list(b)), (bd, it, ep, start)


def test_plane_sse_kernels(orc, ref):
    """orc_plane_sse == svt_spatial_full_distortion_kernel_c (8-bit) / svt_full_distortion_kernel16_bits_c (16-bit),
    the two kernels picture_sse_calculations calls (EbDeblockingFilter.c:830-961)."""
    rng = np.random.default_rng(404)
    orc.orc_plane_sse.restype = C.c_uint64
    ref.svt_spatial_full_distortion_kernel_c.restype = C.c_uint64
    ref.svt_full_distortion_kernel16_bits_c.restype = C.c_uint64
    for (w, h) in ((4, 4), (37, 19), (128, 64), (641, 130)):
        a8 = rng.integers(0, 256, (h, w + 11)).astype(np.uint8); b8 = rng.integers(0, 256, (h, w + 2)).astype(np.uint8)
        assert orc.orc_plane_sse(1, ptr(a8), a8.shape[1], ptr(b8), b8.shape[1], w, h) == \
            ref.svt_spatial_full_distortion_kernel_c(ptr(a8), 0, a8.shape[1], ptr(b8), 0, b8.shape[1], w, h)
        a16 = rng.integers(0, 1024, (h, w + 5)).astype(np.uint16); b16 = rng.integers(0, 1024, (h, w + 8)).astype(np.uint16)
        assert orc.orc_plane_sse(2, ptr(a16), a16.shape[1], ptr(b16), b16.shape[1], w, h) == \
            ref.svt_full_distortion_kernel16_bits_c(ptr(a16), 0, a16.shape[1], ptr(b16), 0, b16.shape[1], w, h)
        a16 = rng.integers(0, 256, (h, w + 5)).astype(np.uint16); b16 = rng.integers(0, 256, (h, w + 8)).astype(np.uint16)     # 8-bit samples in 16-bit planes
        a16[:h // 2] = 255; b16[:h // 2] = 0
        assert orc.orc_plane_sse(2, ptr(a16), a16.shape[1], ptr(b16), b16.shape[1], w, h) == \
            ref.svt_full_distortion_kernel16_bits_c(ptr(a16), 0, a16.shape[1], ptr(b16), 0, b16.shape[1], w, h)


def test_restoration_units_and_stripe_apply(orc, ref):
    """Frame-level loop restoration: the oracle's unit limits and stripe-boundary apply vs the reference's own
    av1_foreach_rest_unit_in_frame + save_tile_row_boundary_lines + svt_av1_loop_restoration_filter_unit (driven through
    oracle/ref_shim.c), luma and chroma, 8- and 10-bit, unit sizes 64 / 128, ragged picture sizes."""
    rng = np.random.default_rng(77)
    for (fw, fh) in ((200, 152), (328, 264), (64, 48), (136, 200)):
        for plane in (0, 1):
            ss = 1 if plane else 0
            pw, ph = (fw + ss) >> ss, (fh + ss) >> ss
            for US in (64, 128):
                nu = orc.orc_rest_units(pw, US) * orc.orc_rest_units(ph, US)
                lo = np.zeros((nu, 4), np.int32); lr = np.zeros((nu, 4), np.int32)
                assert orc.orc_rest_unit_limits(pw, ph, ss, US, ptr(lo)) == nu
                assert ref.ref_shim_rest_unit_limits(fw, fh, plane, US, ptr(lr)) == nu
                assert np.array_equal(lo, lr), (fw, fh, plane, US)
                for bd, dt in FMT3:
                    yy, xx = np.mgrid[0:ph, 0:pw]
                    base = (90 + 50 * np.sin(xx / 9.0) * np.cos(yy / 6.0) + 25 * (((xx // 8) + (yy // 8)) % 2)) * (1 << (bd - 8))
                    dbl = np.clip(base + rng.normal(0, 6 * (1 << (bd - 8)), (ph, pw)), 0, (1 << bd) - 1).astype(dt)
                    cdef = np.clip(dbl.astype(np.int32) + rng.integers(-3, 4, (ph, pw)) * (1 << (bd - 8)), 0, (1 << bd) - 1).astype(dt)
                    E = 8   # border of the CDEF picture buffer (the reference swaps 4 extra columns, reads 3)
                    buf_o = np.ascontiguousarray(np.pad(cdef, E, mode="edge")); buf_r = buf_o.copy()
                    st = buf_o.shape[1]; off = (E * st + E) * buf_o.itemsize
                    u_ep = rng.integers(0, 16, nu).astype(np.uint8)
                    if nu > 2: u_ep[1] = 255
                    u_ep[rng.random(nu) < 0.4] = 254                       # RESTORE_WIENER units
                    u_xqd = np.stack([rng.integers(-96, 32, nu), rng.integers(-32, 96, nu)], 1).astype(np.int32)
                    u_wn = np.zeros((nu, 2, 8), np.int16)
                    for u in range(nu):
                        for d in range(2):
                            t = [int(rng.integers(-5, 11)), int(rng.integers(-23, 9)), int(rng.integers(-17, 47))]
                            if plane: t[0] = 0                              # 5-tap chroma filters
                            u_wn[u, d, :7] = [t[0], t[1], t[2], -2 * sum(t), t[2], t[1], t[0]]
                    dst_o = np.zeros((ph, pw), dt); dst_r = np.zeros((ph, pw), dt)
                    orc.orc_lr_apply_plane(ptr(dbl), pw, C.c_void_p(buf_o.ctypes.data + off), st, buf_o.itemsize, pw, ph, ss, ss, US, bd,
                                           ptr(u_ep), ptr(u_xqd), ptr(u_wn), ptr(dst_o), pw)
                    dst_pad = np.zeros((ph + 8, pw + 32), dt)               # the reference's stripe filter overshoots up to 15 columns
                    assert ref.ref_shim_lr_apply_plane_ex(plane, bd, int(dt == np.uint16), fw, fh, ptr(dbl), pw, C.c_void_p(buf_r.ctypes.data + off), st,
                                                          ptr(dst_pad), pw + 32, US, ptr(u_ep), ptr(u_xqd), ptr(u_wn)) == 0
                    dst_r = dst_pad[:ph, :pw]
                    assert np.array_equal(dst_o, dst_r), (fw, fh, plane, US, bd, np.argwhere(dst_o != dst_r)[:5])
                    assert np.array_equal(buf_o, buf_r), "the CDEF picture must be restored after the stripes"


def test_coefficient_and_pixel_distortion(orc, ref):
    """orc_coeff_distortion == svt_full_distortion_kernel32_bits_c / _cbf_zero32_bits_c / svt_av1_block_error_c /
    svt_aom_satd_c; orc_plane_sse == svt_aom_sse_c on blocks."""
    rng = np.random.default_rng(515)
    ref.svt_av1_block_error_c.restype = C.c_int64
    ref.svt_aom_sse_c.restype = C.c_int64
    orc.orc_plane_sse.restype = C.c_uint64
    for (w, h) in ((4, 4), (8, 16), (32, 32), (64, 16)):
        n = w * h
        c = rng.integers(-30000, 30000, n).astype(np.int32); r = (c + rng.integers(-900, 900, n)).astype(np.int32)
        o = np.zeros(3, np.uint64); d = np.zeros(2, np.uint64)
        orc.orc_coeff_distortion(ptr(c), ptr(r), n, ptr(o))
        ref.svt_full_distortion_kernel32_bits_c(ptr(c), w, ptr(r), w, ptr(d), w, h)
        assert (o[0], o[1]) == (d[0], d[1])
        ssz = C.c_int64()
        c2 = np.clip(c, -20000, 20000).astype(np.int32); r2 = (c2 + rng.integers(-900, 900, n)).astype(np.int32)   # block_error squares in 32-bit int
        orc.orc_coeff_distortion(ptr(c2), ptr(r2), n, ptr(o))
        assert ref.svt_av1_block_error_c(ptr(c2), ptr(r2), C.c_int64(n), C.byref(ssz)) == int(o[0]) and ssz.value == int(o[1])
        assert ref.svt_aom_satd_c(ptr(c2), n) == int(o[2])
        orc.orc_coeff_distortion(ptr(c), None, n, ptr(o))
        ref.svt_full_distortion_kernel_cbf_zero32_bits_c(ptr(c), w, ptr(d), w, h)
        assert (o[0], o[1]) == (d[0], d[1]) and o[0] == o[1]
        a = rng.integers(0, 256, (h, w + 3)).astype(np.uint8); b = rng.integers(0, 256, (h, w + 9)).astype(np.uint8)
        assert ref.svt_aom_sse_c(ptr(a), w + 3, ptr(b), w + 9, w, h) == orc.orc_plane_sse(1, ptr(a), w + 3, ptr(b), w + 9, w, h)


def test_wiener_stats_and_convolve(orc, ref):
    """orc_wiener_compute_stats == svt_av1_compute_stats_c / _highbd_c (windows 7, 5, 3; ragged unit rectangles),
    orc_wiener_convolve_add_src == svt_av1_[highbd_]wiener_convolve_add_src_c (symmetric 7-tap kernels over the legal tap ranges)."""
    rng = np.random.default_rng(808)
    for bd, dt in FMT3:
        dgd = rng.integers(0, 1 << bd, (120, 140)).astype(dt); src = np.clip(dgd.astype(np.int32) + rng.integers(-20, 21, dgd.shape), 0, (1 << bd) - 1).astype(dt)
        for win in (7, 5, 3):
            for (h0, h1, v0, v1) in ((8, 72, 8, 72), (10, 101, 5, 37), (30, 31, 40, 41)):
                w2 = win * win
                Mo, Ho = np.zeros(w2, np.int64), np.zeros(w2 * w2, np.int64); Mr, Hr = Mo.copy(), Ho.copy()
                orc.orc_wiener_compute_stats(win, ptr(dgd), ptr(src), dgd.itemsize, bd, h0, h1, v0, v1, 140, 140, ptr(Mo), ptr(Ho))
                if dt == np.uint8:
                    ref.svt_av1_compute_stats_c(win, ptr(dgd), ptr(src), h0, h1, v0, v1, 140, 140, ptr(Mr), ptr(Hr))
                else:
                    ref.svt_av1_compute_stats_highbd_c(win, C.c_void_p(dgd.ctypes.data >> 1), C.c_void_p(src.ctypes.data >> 1), h0, h1, v0, v1, 140, 140, ptr(Mr), ptr(Hr), bd)
                assert np.array_equal(Mo, Mr) and np.array_equal(Ho, Hr), (bd, win, h0, h1, v0, v1)
        # convolve: taps t0..t2 in the AV1 ranges, centre = -2 * (t0 + t1 + t2), tap[7] = 0 (EbRestoration.h:240-260)
        class CP(C.Structure):
            _fields_ = [("ref", C.c_int32), ("do_average", C.c_int32), ("dst", C.c_void_p), ("dst_stride", C.c_int32), ("round_0", C.c_int32), ("round_1", C.c_int32),
                        ("plane", C.c_int32), ("is_compound", C.c_int32), ("use_jnt_comp_avg", C.c_int32), ("fwd_offset", C.c_int32), ("bck_offset", C.c_int32),
                        ("use_dist_wtd_comp_avg", C.c_int32)]
        cp = CP(0, 0, None, 0, 3, 11, 0, 0, 0, 0, 0, 0)
        for trial in range(6):
            def taps():
                t = [int(rng.integers(-5, 11)), int(rng.integers(-23, 9)), int(rng.integers(-17, 47))]
                if trial == 0: t = [10, 8, 46]
                if trial == 1: t = [-5, -23, -17]
                f = np.zeros(64, np.int16)      # 128-byte block: the reference masks the pointer to a 256-byte table base
                f[:7] = [t[0], t[1], t[2], -2 * sum(t), t[2], t[1], t[0]]
                return f
            fx, fy = taps(), taps()
            w, h = (64, 56) if trial % 2 == 0 else (24, 9)
            eo = np.zeros((h, w + 5), dt); er = np.zeros((h, w + 5), dt)
            p = dgd.ctypes.data + (20 * 140 + 30) * dgd.itemsize
            orc.orc_wiener_convolve_add_src(C.c_void_p(p), 140, ptr(eo), w + 5, dgd.itemsize, ptr(fx), ptr(fy), w, h, bd)
            if dt == np.uint8:
                ref.svt_av1_wiener_convolve_add_src_c(C.c_void_p(p), C.c_int64(140), ptr(er), C.c_int64(w + 5), ptr(fx), ptr(fy), w, h, C.byref(cp))
            else:
                ref.svt_av1_highbd_wiener_convolve_add_src_c(C.c_void_p(p >> 1), C.c_int64(140), C.c_void_p(er.ctypes.data >> 1), C.c_int64(w + 5), ptr(fx), ptr(fy), w, h, C.byref(cp), bd)
            assert np.array_equal(eo, er), (bd, trial)


from wiener_common import wiener_unit_stats


def test_wiener_initial_filter(orc, ref):
    """orc_wiener_unit_init == the reference's wiener_decompose_sep_sym + finalize_sym_filter + compute_score (EbRestorationPick.c:946-1052, static there: reached through
    oracle/ref_shim_restpick.c), windows 7 / 5 / 3, 8- and 10-bit statistics of blurred, noisy, identical, flat and unrelated picture pairs, plus raw random M / H."""
    if not hasattr(ref, "ref_shim_wiener_unit_init"): pytest.skip("oracle/_ref predates the Wiener shim: rebuild it")
    rng = np.random.default_rng(4242)
    seen = set()
    cases = [(win, bd, kind, t) for win in (7, 5, 3) for bd in (8, 10) for kind in range(5) for t in range(3)]
    for win, bd, kind, t in cases + [(win, 0, 9, t) for win in (7, 5, 3) for t in range(6)]:
        if kind == 9:   # symmetric positive-definite-ish random statistics, then plain random ones
            w2 = win * win
            G = rng.integers(-300, 300, (w2, 3 * w2)).astype(np.int64)
            H = (G @ G.T).reshape(-1).copy() if t < 3 else rng.integers(-(1 << 30), 1 << 30, w2 * w2).astype(np.int64)
            M = rng.integers(-(1 << 26), 1 << 26, w2).astype(np.int64)
        else:
            M, H = wiener_unit_stats(orc, rng, win, bd, kind)
        vo, ho, vr, hr = (np.full(8, 77, np.int16) for _ in range(4))
        Mr, Hr = M.copy(), H.copy()
        ro = orc.orc_wiener_unit_init(win, ptr(M), ptr(H), ptr(vo), ptr(ho))
        rr = ref.ref_shim_wiener_unit_init(win, ptr(Mr), ptr(Hr), ptr(vr), ptr(hr))
        assert ro == rr and np.array_equal(vo, vr) and np.array_equal(ho, hr), (win, bd, kind, t, ro, rr, vo, vr, ho, hr)
        assert np.array_equal(M, Mr) and np.array_equal(H, Hr)
        seen.add(ro)
    assert seen == {1, 2}


import tf_common as tfc


@pytest.mark.parametrize("bd,fmt", [pytest.param(8, None, id="8"), pytest.param(10, None, id="10"), pytest.param(8, np.uint16, id="u16-8")])
@pytest.mark.parametrize("ss", [0, 1])
def test_wiener_tap_refinement_walk(ref, bd, fmt, ss):
    """The restatement of finer_tile_search_wiener_seg (Encoder/Codec/EbRestorationPick.c:1092-1200) that stands in for the device's wiener_walk_kernel on boxes without a
    GPU -- the state machine of oracle/hip_mock.c (svt_hip_wiener_walk_units_dev of the CPU test double, every probe on the oracle's restoration filter), which the GPU test
    tests/test_sgr_gpu.py::test_wiener_walk_units compares the device with -- against the reference's own static function, driven through oracle/ref_shim_restpick.c:
    the same refined taps, the same error and the same number of try_restoration_unit_seg probes for every unit.  Same cases as the GPU test."""
    import shard_common as sc
    import test_sgr_gpu as tg
    if not os.path.exists(sc.MOCK_LIB):
        pytest.skip("oracle/_ref/mock/libsvtav1_hip.so not built (make -f oracle/Makefile.enc)")
    M = sc.load(sc.MOCK_LIB)
    ref.ref_shim_wiener_finer_search_plane.argtypes = load_package().PROTOTYPES["svt_hip_wiener_walk_units_dev"][1][1:]   # the same walk without the context
    EXT = tg.EXT
    for (w, h, US, win) in ((200, 152, 64, 7), (328, 264, 128, 7), (200, 152, 64, 5), (136, 72, 64, 3)):
        if ss and win == 7: win = 5     # chroma planes search the 5-tap window at most (search_wiener_seg :1352-1358)
        src, ext = tg.make_planes(w, h, bd, 190 + bd + ss + US, fmt, fmt is not None)      # fmt: 8-bit samples in 16-bit planes, with the planted extremes of the GPU test
        st = ext.shape[1]; off = (EXT * st + EXT) * ext.itemsize
        rng = np.random.default_rng(31 + ss + win)
        dbl = np.clip(ext[EXT:EXT + h, EXT:EXT + w].astype(np.int32) + rng.integers(-9, 10, (h, w)) * (1 << (bd - 8)), 0, (1 << bd) - 1).astype(ext.dtype)
        nu = tg.units(w, US) * tg.units(h, US)
        act = (rng.random(nu) < 0.8).astype(np.uint8); act[0] = 1
        o = (7 - win) >> 1
        wn = np.zeros((nu, 2, 8), np.int16)
        for u in range(nu):
            for d in range(2):
                t = [int(rng.integers(-5, 11)), int(rng.integers(-23, 9)), int(rng.integers(-17, 47))]
                if u % 4 == 0: t = [0, 0, 0]
                if u == 1: t = [10, 8, 46] if d else [-5, -23, -17]
                for k in range(o): t[k] = 0
                wn[u, d, :7] = [t[0], t[1], t[2], -2 * sum(t), t[2], t[1], t[0]]
        m_wn = wn.copy(); m_err = np.full(nu, -1, np.int64); m_pr = np.zeros(nu, np.uint32)
        work = ext.copy()
        assert M.svt_hip_wiener_walk_units_dev(None, ext.itemsize, bd, C.c_void_p(work.ctypes.data + off), st, w, h, US, ss, ptr(dbl), w, ptr(src), w, ptr(m_wn), ptr(act), win, ptr(m_err), ptr(m_pr)) == 0
        r_wn = wn.copy(); r_err = np.full(nu, -1, np.int64); r_pr = np.zeros(nu, np.uint32)
        work2 = ext.copy()
        assert ref.ref_shim_wiener_finer_search_plane(ext.itemsize, bd, C.c_void_p(work2.ctypes.data + off), st, w, h, US, ss, ptr(dbl), w, ptr(src), w, ptr(r_wn), ptr(act), win, ptr(r_err), ptr(r_pr)) == 0
        on = act.astype(bool)
        assert np.array_equal(m_wn, r_wn), (bd, ss, w, h, US, win, np.argwhere(m_wn != r_wn)[:4])
        assert np.array_equal(m_err[on], r_err[on]), (bd, ss, US, win)
        assert np.array_equal(m_pr[on], r_pr[on]) and r_pr[on].min() >= 7, (bd, ss, US, win, m_pr, r_pr)
        assert (r_wn[on] != wn[on]).any()


def test_temporal_filter_planewise_noise_and_divu(orc, ref):
    """orc_tf_planewise vs svt_av1_apply_temporal_filter_planewise(_hbd)_c (libm expf / log1p / sqrtf on both sides), estimate_noise,
    and OD_DIVU == plain division on get_final_filtered_pixels' domain.  Inputs as test/TemporalFilterTestPlanewise.cc:200-330."""
    rng = np.random.default_rng(2024)
    def _cnt0(it):
        r2 = np.random.default_rng(it); [r2.integers(0, 1 << 20, 32 * 64) for _ in range(3)]
        return r2.integers(0, 3000, 32 * 64).astype(np.int64)
    for bd, dt in FMT3 + ((9, np.uint16), (11, np.uint16), (12, np.uint16)):      # the shifts (bd - 8) * 2 and bd - 8 are run-time values: every depth the entry points accept
        hbd = int(dt == np.uint16)
        seen = set()
        for it in range(24):
            ss = 1 if it % 6 else 0
            cw = 32 >> ss
            blk = tfc.make_blocks(rng, 1, bd, big_mv=(it % 4 == 1), err_max=(0, 3, 20, 60)[it % 4])
            if it % 3 == 0:     # the reference test's distribution: fully random pixels
                src = [rng.integers(0, 1 << bd, (32, 80)).astype(dt), rng.integers(0, 1 << bd, (cw, 48)).astype(dt), rng.integers(0, 1 << bd, (cw, 48)).astype(dt)]
                pre = [rng.integers(0, 1 << bd, (32, 64)).astype(dt), rng.integers(0, 1 << bd, (cw, 64 >> ss)).astype(dt), rng.integers(0, 1 << bd, (cw, 64 >> ss)).astype(dt)]
            else:               # close predictors: weights spread over the whole 0..1000 range
                src = [rng.integers(0, 1 << bd, (32, 80)).astype(dt), rng.integers(0, 1 << bd, (cw, 48)).astype(dt), rng.integers(0, 1 << bd, (cw, 48)).astype(dt)]
                amp = 0 if it in (4, 16) else (0, 1, 2, 4, 8, 23)[it % 6] << (bd - 8)      # 4, 16: zero error -> weight 1000
                pre = [np.clip(s[:, :p].astype(np.int32) + rng.integers(-amp, amp + 1, (s.shape[0], p)), 0, (1 << bd) - 1).astype(dt)
                       for s, p in zip(src, (32, cw, cw))]
                pre = [np.ascontiguousarray(np.pad(p, ((0, 0), (0, (64 >> (ss if i else 0)) - p.shape[1])))) for i, p in enumerate(pre)]
            noise = rng.uniform(0.0, 8.0, 3)
            decay = int(rng.integers(2, 5)); mfs = int(rng.choice([64, 240, 1080, 2160]))
            r, c = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            outs = []
            for which in ("ref", "orc"):
                r2 = np.random.default_rng(it)
                acc = [r2.integers(0, 1 << 20, 32 * 64).astype(np.uint32) for _ in range(3)]
                cnt = [r2.integers(0, 3000, 32 * 64).astype(np.uint16) for _ in range(3)]
                common = (r, c, it % 5 != 4, mfs)
                tail = (ptr(src[0]), 80, ptr(pre[0]), 64, ptr(src[1]), ptr(src[2]), 48, ptr(pre[1]), ptr(pre[2]), 64 >> ss, 32, 32, ss, ss,
                        ptr(noise), decay, ptr(acc[0]), ptr(cnt[0]), ptr(acc[1]), ptr(cnt[1]), ptr(acc[2]), ptr(cnt[2]))
                if which == "ref":
                    b = blk[0]
                    ref.ref_shim_tf_planewise(ptr(np.ascontiguousarray(b["mv16_x"])), ptr(np.ascontiguousarray(b["mv16_y"])), ptr(np.ascontiguousarray(b["err16"])),
                                              ptr(np.ascontiguousarray(b["mv32_x"])), ptr(np.ascontiguousarray(b["mv32_y"])), ptr(np.ascontiguousarray(b["err32"])),
                                              ptr(np.ascontiguousarray(b["split"])), *common, hbd, bd, *tail)
                else:
                    orc.orc_tf_planewise(ptr(blk), *common, src[0].itemsize, bd, *tail)
                outs.append(acc + cnt)
            for i, (a, b) in enumerate(zip(*outs)):
                assert np.array_equal(a, b), (bd, it, i, np.argwhere(a != b)[:4])
            seen.update(np.unique((outs[0][3].astype(np.int64) - _cnt0(it)) & 0xffff).tolist())
        assert 0 in seen and 1000 in seen and len(seen) > 300, (bd, len(seen))       # weights over the whole 0..1000 range were exercised
        # noise estimate
        ref.ref_shim_estimate_noise.restype = C.c_double; orc.orc_tf_estimate_noise.restype = C.c_double
        for it in range(4):
            w, h = 200 + 8 * it, 120
            img = np.clip(120 + 40 * np.sin(np.arange(w) / 9.0)[None, :] + rng.normal(0, 1 + 3 * it, (h, w)), 0, 255)
            img = (img * (1 << (bd - 8))).astype(dt)
            if it == 3: img[:] = rng.integers(0, 1 << bd, (h, w))          # all edges: too few smooth pixels -> -1
            out = np.zeros(2, np.int64)
            e = ref.ref_shim_estimate_noise(ptr(img), hbd, bd, w, h, w)
            g = orc.orc_tf_estimate_noise(ptr(img), img.itemsize, bd, w, h, w, ptr(out))
            assert e == g, (bd, it, e, g)
    ref.ref_shim_od_divu.restype = C.c_uint32
    for d in (1, 2, 3, 999, 1000, 1001, 1023, 1024, 5000, 13000, 65535):
        for x in (0, 1, d - 1, d, 255 * d + d // 2, 1023 * d + d // 2, 4095 * d + d // 2, 4095 * d + d // 2 - 1, (1 << 32) - 1):
            if d >= 1024 or x < (1 << 32) // 2:       # OD_DIVU_SMALL is documented exact for x below 2^31 here
                assert ref.ref_shim_od_divu(C.c_uint32(x), C.c_uint32(d)) == x // d, (x, d)
    rng = np.random.default_rng(3)
    for d in range(1000, 1024):
        for x in rng.integers(0, 4096 * d, 400):
            assert ref.ref_shim_od_divu(C.c_uint32(int(x)), C.c_uint32(d)) == int(x) // d


import comp_common as cmc


def test_compound_prediction(orc, ref):
    """orc_jnt_convolve_d16 / orc_compound_predict_batch == two svt_av1_[highbd_]jnt_convolve_*_c calls (do_average 0, then 1
    with / without use_jnt_comp_avg), svt_av1_build_compound_diffwtd_mask_d16_c + svt_aom_{lowbd,highbd}_blend_a64_d16_mask_c.
    Block sizes, phases and filters as /root/reference/test/convolve_2d_test.cc (jnt cases) and CompBlendTest.cc."""
    rng = np.random.default_rng(77)
    W, H = 1280, 1024
    for bd, dt in ((8, np.uint8), (10, np.uint16), (12, np.uint16), (8, np.uint16)):
        hbd = dt == np.uint16
        r0 = 5 if bd == 12 else 3           # get_conv_params_no_round: ROUND0_BITS (+ 2 at 12 bits)
        ref0 = rng.integers(0, 1 << bd, (H, W)).astype(dt); ref1 = rng.integers(0, 1 << bd, (H, W)).astype(dt)
        ref0[:130, :130] = (1 << bd) - 1; ref1[:130, :130] = 0                # extreme block
        n = 44
        blks, masks = cmc.make_blocks(rng, W - 256, H - 256, n, 1 << 20)
        for b in blks:                                                          # keep 8 samples of context inside the planes
            b.src0_x += 64; b.src0_y += 64; b.src1_x += 64; b.src1_y += 64
        dst = np.zeros((H, W), dt); m_orc = masks.copy()
        orc.orc_compound_predict_batch(ref0.itemsize, bd, ptr(ref0), W, ptr(ref1), W, ptr(dst), W, ptr(m_orc), blks, 0, n)
        _compound_vs_ref(orc, ref, bd, ref0, ref1, blks, masks, dst, m_orc)


def _compound_vs_ref(orc, ref, bd, ref0, ref1, blks, masks, dst, m_orc):
    """every block of a list: both 16-bit intermediates, the stored DIFFWTD mask and the samples of plane dst against the reference's functions"""
    dt, W = ref0.dtype, ref0.shape[1]
    assert ref1.shape[1] == W
    hbd = dt == np.uint16
    r0 = 5 if bd == 12 else 3
    pre = "svt_av1_highbd_" if hbd else "svt_av1_"
    for i, b in enumerate(blks):
        w, h = b.w, b.h
        fx = _IFP(C.addressof((C.c_int16 * 8 * 16).in_dll(ref, REF_BANKS[b.bank_x])), 8, 16, 0)
        fy = _IFP(C.addressof((C.c_int16 * 8 * 16).in_dll(ref, REF_BANKS[b.bank_y])), 8, 16, 0)
        d16 = [np.zeros((h, w), np.uint16), np.zeros((h, w), np.uint16)]
        out = np.zeros((h, w), dt)
        for r, (plane, sx_, sy_, px, py) in enumerate(((ref0, b.subpel0_x, b.subpel0_y, b.src0_x, b.src0_y), (ref1, b.subpel1_x, b.subpel1_y, b.src1_x, b.src1_y))):
            cp = _ConvP(); cp.round_0 = r0; cp.round_1 = 7; cp.is_compound = 1; cp.dst = d16[r].ctypes.data; cp.dst_stride = w
            name = pre + "jnt_convolve_" + {(0, 0): "2d_copy", (1, 0): "x", (0, 1): "y", (1, 1): "2d"}[(int(sx_ != 0), int(sy_ != 0))] + "_c"
            sp = C.c_void_p(plane.ctypes.data + (py * W + px) * plane.itemsize)
            args = [sp, W, ptr(out), w, w, h, C.byref(fx), C.byref(fy), sx_, sy_, C.byref(cp)]
            if hbd: args.append(bd)
            getattr(ref, name)(*args)
            mine = np.zeros((h, w), np.uint16)
            orc.orc_jnt_convolve_d16(sp, W, plane.itemsize, w, h, b.bank_x, b.bank_y, sx_, sy_, bd, ptr(mine), w)
            assert np.array_equal(mine, d16[r]), (bd, i, r, name)
        cp = _ConvP(); cp.round_0 = r0; cp.round_1 = 7; cp.is_compound = 1
        if b.type <= 1:      # second call with do_average: dst holds the first prediction
            cp.dst = d16[0].ctypes.data; cp.dst_stride = w; cp.do_average = 1; cp.use_jnt_comp_avg = b.type
            cp.fwd_offset, cp.bck_offset = b.fwd_offset, b.bck_offset
            name = pre + "jnt_convolve_" + {(0, 0): "2d_copy", (1, 0): "x", (0, 1): "y", (1, 1): "2d"}[(int(b.subpel1_x != 0), int(b.subpel1_y != 0))] + "_c"
            sp = C.c_void_p(ref1.ctypes.data + (b.src1_y * W + b.src1_x) * ref1.itemsize)
            args = [sp, W, ptr(out), w, w, h, C.byref(fx), C.byref(fy), b.subpel1_x, b.subpel1_y, C.byref(cp)]
            if hbd: args.append(bd)
            getattr(ref, name)(*args)
        else:
            if b.type == 2:
                seg = np.zeros((h, w), np.uint8)
                ref.svt_av1_build_compound_diffwtd_mask_d16_c(ptr(seg), int(b.mask_type), ptr(d16[0]), w, ptr(d16[1]), w, h, w, C.byref(cp), bd)
                if b.mask_off >= 0:
                    assert np.array_equal(m_orc[b.mask_off:b.mask_off + w * h].reshape(h, w), seg), (bd, i, "seg mask")
                mptr, mstride, sub = ptr(seg), w, 0
            else:
                mptr, mstride, sub = C.c_void_p(masks.ctypes.data + b.mask_off), b.mask_stride, int(b.mask_sub)
            if not hbd:
                ref.svt_aom_lowbd_blend_a64_d16_mask_c(ptr(out), w, ptr(d16[0]), w, ptr(d16[1]), w, mptr, mstride, w, h, sub, sub, C.byref(cp))
            else:
                ref.svt_aom_highbd_blend_a64_d16_mask_c(ptr(out), w, ptr(d16[0]), w, ptr(d16[1]), w, mptr, mstride, w, h, sub, sub, C.byref(cp), bd)
        got = dst[b.dst_y:b.dst_y + h, b.dst_x:b.dst_x + w]
        assert np.array_equal(got, out), (bd, i, b.type, w, h, np.argwhere(got != out)[:4])


def test_compound_prediction_every_size_type_flavour(orc, ref):
    """the same proof on the full product the device test launches (comp_common.compound_cases: 22 sizes x 4 types x 16 flavour pairs), every format"""
    for bd, dt in ((8, None), (10, None), (12, None), (8, np.uint16)):
        c = cmc.compound_cases(bd, dt)
        _, _, exp, m_exp = cmc.compound_expected(orc, bd, dt)
        _compound_vs_ref(orc, ref, bd, c.ref0, c.ref1, c.blks, c.masks, exp, m_exp)


def test_obmc_sad_variance(orc, ref):
    """orc_obmc_block == svt_aom_obmc_sad{W}x{H}_c / svt_aom_obmc_variance{W}x{H}_c / svt_aom_obmc_sub_pixel_variance{W}x{H}_c for every block size;
    wsrc / mask ranges as calc_target_weighted_pred produces them (mask <= 64 * 64, wsrc <= 255 * 4096) — /root/reference/test/OBMCSadTest.cc, OBMCVarianceTest.cc."""
    rng = np.random.default_rng(808)
    for (w, h) in cmc.SIZES:
        for it in range(6):
            pre = rng.integers(0, 256, (h + 2, w + 10)).astype(np.uint8)
            mask = rng.integers(0, 4097, (h, w)).astype(np.int32)
            wsrc = rng.integers(0, 255 * 4096 + 1, (h, w)).astype(np.int32)
            if it == 1: pre[:] = 255; wsrc[:] = 0; mask[:] = 4096                 # largest differences
            if it == 2: wsrc = (pre[:h, :w].astype(np.int32) * mask)              # zero difference
            xo, yo = (0, 0) if it < 3 else (int(rng.integers(0, 8)), int(rng.integers(0, 8)))
            out = np.zeros(3, np.uint32)
            orc.orc_obmc_block(ptr(pre), pre.shape[1], ptr(wsrc), ptr(mask), w, h, xo, yo, ptr(out))
            assert (int(out[0]), int(out[1]), int(out[2])) == _obmc_ref(ref, pre, wsrc, mask, w, h, xo, yo), (w, h, it, xo, yo)


def _obmc_ref(ref, pre, wsrc, mask, w, h, xo, yo):
    """(sad, sse, variance) of the reference's three functions; pre: a 2-D view whose first sample is the block's, wsrc / mask: the block's w * h values"""
    pp, stride = C.c_void_p(pre.ctypes.data), pre.strides[0]
    sad = getattr(ref, f"svt_aom_obmc_sad{w}x{h}_c")(pp, stride, ptr(wsrc), ptr(mask))
    sse = C.c_uint32(0)
    if xo == 0 and yo == 0:
        var = getattr(ref, f"svt_aom_obmc_variance{w}x{h}_c")(pp, stride, ptr(wsrc), ptr(mask), C.byref(sse))
        var2 = getattr(ref, f"svt_aom_obmc_sub_pixel_variance{w}x{h}_c")(pp, stride, 0, 0, ptr(wsrc), ptr(mask), C.byref(sse))
        assert (var & 0xFFFFFFFF) == (var2 & 0xFFFFFFFF)
    else:
        var = getattr(ref, f"svt_aom_obmc_sub_pixel_variance{w}x{h}_c")(pp, stride, xo, yo, ptr(wsrc), ptr(mask), C.byref(sse))
    return sad & 0xFFFFFFFF, sse.value, var & 0xFFFFFFFF


def test_obmc_every_size_offset_content(orc, ref):
    """the oracle's results on comp_common.obmc_cases (22 sizes x four offset classes x four contents, what the device test launches) == the reference's"""
    c = cmc.obmc_cases()
    exp = cmc.obmc_expected(orc)
    for i, (b, d) in enumerate(zip(c.blks, c.desc)):
        got = _obmc_ref(ref, c.pre[b.pre_y:, b.pre_x:], c.wsrc[b.wm_off:b.wm_off + b.w * b.h], c.mask[b.wm_off:b.wm_off + b.w * b.h], b.w, b.h, b.xoffset, b.yoffset)
        assert tuple(int(v) for v in exp[i]) == got, (i, d)


def test_warp_affine(orc, ref):
    """orc_warp_affine == svt_av1_warp_affine_c / svt_av1_highbd_warp_affine_c (non-compound), models as /root/reference/test/warp_filter_test_util.cc,
    including models that push the block outside the plane (edge clamping) and luma / 4:2:0 chroma sub-sampling."""
    rng = np.random.default_rng(66)
    W, H = 1024, 512
    for bd, dt in ((8, np.uint8), (10, np.uint16), (12, np.uint16), (8, np.uint16)):
        plane = rng.integers(0, 1 << bd, (H, W)).astype(dt)
        if dt == np.uint16 and bd == 8:
            plane[:256, :256] = 255; plane[:256, 256:512] = 0; plane[256:, :512] = rng.integers(0, 2, (H - 256, 512)) * 255
        n = 28
        blks = cmc.warp_blocks(rng, W, H, n)
        for ss in (0, 1):
            for i, b in enumerate(blks):
                w, h = b.p_width, b.p_height
                a = np.zeros((h, w), dt)
                mat = (C.c_int32 * 8)(*list(b.mat), 0, 0)
                e = _warp_ref(ref, b, plane, W, H, W, bd, (ss, ss))
                orc.orc_warp_affine(mat, ptr(plane), plane.itemsize, bd, W, H, W, ptr(a), b.p_col, b.p_row, w, h, w, ss, ss, b.alpha, b.beta, b.gamma, b.delta)
                assert np.array_equal(a, e), (bd, ss, i, w, h, np.argwhere(a != e)[:4])


def _warp_ref(ref, b, plane, width, height, stride, bd, ss, comp=None):
    """one record through svt_av1_[highbd_]warp_affine_c -> its w x h samples.  comp = (convbuf, cb_off, cb_stride, do_average, use_jnt_comp_avg, fwd, bck): the
    is_compound branches on the 16-bit buffer convbuf (written in place when do_average is 0)"""
    w, h = b.p_width, b.p_height
    e = np.zeros((h, w), plane.dtype)
    mat = (C.c_int32 * 8)(*list(b.mat), 0, 0)
    cp = _ConvP(); cp.round_0 = 5 if bd == 12 else 3; cp.round_1 = 2 * 7 - cp.round_0
    if comp:
        cb, off, cbs, avg, jnt, fwd, bck = comp
        cp.round_1 = 7; cp.is_compound = 1; cp.dst = cb.ctypes.data + 2 * off; cp.dst_stride = cbs
        cp.do_average, cp.use_jnt_comp_avg, cp.fwd_offset, cp.bck_offset = avg, jnt, fwd, bck
    args = (mat, ptr(plane), width, height, stride, ptr(e), b.p_col, b.p_row, w, h, w, ss[0], ss[1])
    if plane.dtype == np.uint8: ref.svt_av1_warp_affine_c(*args, C.byref(cp), b.alpha, b.beta, b.gamma, b.delta)
    else: ref.svt_av1_highbd_warp_affine_c(*args, bd, C.byref(cp), b.alpha, b.beta, b.gamma, b.delta)
    return e


WARP_FMTS = ((8, np.uint8), (10, np.uint16), (12, np.uint16), (8, np.uint16))


def test_warp_every_size_edge_ss(orc, ref):
    """the oracle on comp_common.warp_cases == the reference: 4-wide and 4-high blocks (the reference cuts the last cell of a row or column with
    AOMMIN(4, p_col + p_width - j - 4), so any size is within what it accepts), cells beyond and astride every edge, a 6 x 5 plane (every index is clamped: any
    plane from 1 x 1 up is accepted), 4:4:4, 4:2:0 and 4:2:2"""
    for bd, dt in WARP_FMTS:
        for ss in cmc.WARP_SS:
            for lst in cmc.warp_cases(ss):
                plane, _, exp = cmc.warp_expected(orc, lst, ss, bd, dt)
                w, h, stride = lst.plane
                for i, (b, d) in enumerate(zip(lst.blks, lst.desc)):
                    e = _warp_ref(ref, b, plane, w, h, stride, bd, ss)
                    a = exp[b.p_row:b.p_row + b.p_height, b.p_col:b.p_col + b.p_width]
                    assert np.array_equal(a, e), (bd, ss, lst.name, i, d, np.argwhere(a != e)[:4])


def test_warp_compound_batch(orc, ref):
    """orc_warp_compound_batch == the is_compound branches of svt_av1_[highbd_]warp_affine_c (Common/Codec/EbWarpedMotion.c:660-683, :812-835) on the four
    launches of comp_common.warp_comp_cases: first pass into the compound buffer, second pass averaged or distance-weighted into pixels, both mixed, no
    destination plane"""
    w, h, stride = cmc.WARP_PLANE
    for bd, dt in WARP_FMTS:
        for ss in cmc.WARP_SS:
            c = cmc.warp_comp_cases(ss)
            planes, steps = cmc.warp_comp_expected(orc, c, bd, dt)
            for n, l in enumerate(c.lists):
                cb, dst = steps[n][0].copy(), steps[n][1].copy()
                for b in l.blks:
                    e = _warp_ref(ref, b.blk, planes[l.which], w, h, stride, bd, ss, (cb, b.cb_off, b.cb_stride, b.do_average, b.use_jnt_comp_avg, b.fwd_offset, b.bck_offset))
                    if b.do_average: dst[b.blk.p_row:b.blk.p_row + b.blk.p_height, b.blk.p_col:b.blk.p_col + b.blk.p_width] = e
                    else: assert not e.any()                       # a first pass leaves the pixels alone
                assert np.array_equal(cb, steps[n + 1][0]) and np.array_equal(dst, steps[n + 1][1]), (bd, ss, l.name)
                assert not np.array_equal(cb, steps[n][0]) or not np.array_equal(dst, steps[n][1])


def test_warp_filter_table_headers(ref):
    """The generated Warped_Filters headers (HIP kernel and oracle) hold exactly the reference's eb_warped_filter."""
    import os, re
    from conftest import ROOT
    want = [int(v) for row in (C.c_int16 * 8 * 193).in_dll(ref, "eb_warped_filter") for v in row]
    for path in ("svt-av1_amd/csrc/warp_filter_table.h", "oracle/warp_filter_table.h"):
        txt = open(os.path.join(ROOT, path)).read()
        got = [int(v) for v in re.findall(r"-?\d+", txt[txt.index("#define SVT_WARPED_FILTER_TABLE"):])]
        assert got == want, path


def test_blend_a64_masks(orc, ref):
    """orc_blend_a64_batch == svt_aom_[highbd_]blend_a64_{mask,hmask,vmask}_c (/root/reference/test/BlendA64MaskTest.cc sizes 1..128, masks 0..64,
    the four mask sub-sampling combinations, in-place destination)."""
    rng = np.random.default_rng(123)
    W, H = 768, 640
    for bd, dt in ((8, np.uint8), (10, np.uint16)):
        a = rng.integers(0, 1 << bd, (H, W)).astype(dt); b1 = rng.integers(0, 1 << bd, (H, W)).astype(dt)
        n = 30
        blks, masks = cmc.blend_blocks(rng, W, H, n, 1 << 18)
        out = a.copy()                      # dst plane = src0 plane, so that the "in place" blocks really alias
        orc.orc_blend_a64_batch(a.itemsize, ptr(out), W, ptr(b1), W, ptr(out), W, ptr(masks), blks, n)
        run = a.copy()                      # the same sequence through the reference functions, block by block
        _blend_ref(ref, bd, run, b1, run, masks, blks)
        assert np.array_equal(out, run) and (out != a).any(), bd


def _blend_ref(ref, bd, src0, b1, run, masks, blks):
    """a block list through the reference's blend functions in order: src0 / b1 -> run (src0 may be run itself: in place)"""
    dt = run.dtype
    for i, b in enumerate(blks):
        w, h = b.w, b.h
        s0 = np.ascontiguousarray(src0[b.src0_y:b.src0_y + h, b.src0_x:b.src0_x + w]); s1 = np.ascontiguousarray(b1[b.src1_y:b.src1_y + h, b.src1_x:b.src1_x + w])
        e = np.zeros((h, w), dt)
        mp = C.c_void_p(masks.ctypes.data + b.mask_off)
        if bd == 8:
            if b.mode == 0: ref.svt_aom_blend_a64_mask_c(ptr(e), w, ptr(s0), w, ptr(s1), w, mp, b.mask_stride, w, h, int(b.subw), int(b.subh))
            elif b.mode == 1: ref.svt_aom_blend_a64_hmask_c(ptr(e), w, ptr(s0), w, ptr(s1), w, mp, w, h)
            else: ref.svt_aom_blend_a64_vmask_c(ptr(e), w, ptr(s0), w, ptr(s1), w, mp, w, h)
        else:
            if b.mode == 0: ref.svt_aom_highbd_blend_a64_mask_c(ptr(e), w, ptr(s0), w, ptr(s1), w, mp, b.mask_stride, w, h, int(b.subw), int(b.subh), bd)
            elif b.mode == 1: ref.svt_aom_highbd_blend_a64_hmask_8bit_c(ptr(e), w, ptr(s0), w, ptr(s1), w, mp, w, h, bd)
            else: ref.svt_aom_highbd_blend_a64_vmask_8bit_c(ptr(e), w, ptr(s0), w, ptr(s1), w, mp, w, h, bd)
        run[b.dst_y:b.dst_y + h, b.dst_x:b.dst_x + w] = e


def test_blend_every_size_mode_mask(orc, ref):
    """the oracle on comp_common.blend_cases, in place and out of place, 8-bit and 16-bit samples up to 4095 (bd 12) == the reference"""
    for in_place in (True, False):
        c = cmc.blend_cases(in_place)
        for bd, dt in ((8, np.uint8), (12, np.uint16)):
            a, b1, dst0 = cmc.blend_planes(c, dt)
            exp = dst0.copy()
            orc.orc_blend_a64_batch(a.itemsize, ptr(exp if in_place else a), c.w, ptr(b1), c.w, ptr(exp), c.w, ptr(c.masks), c.blks, c.n)
            run = dst0.copy()
            _blend_ref(ref, bd, run if in_place else a, b1, run, c.masks, c.blks)
            assert np.array_equal(exp, run) and (exp != dst0).any(), (in_place, bd)


def test_picture_format_conversions(orc, ref):
    """orc_picture_format == the reference's 8+2-bit <-> 16-bit conversions (Common/C_DEFAULT/EbPackUnPack_C.c), ragged strides and sizes."""
    rng = np.random.default_rng(55)
    for (w, h) in ((64, 16), (200, 37), (8, 3), (1924, 5)):
        w4 = w & ~3
        in8 = rng.integers(0, 256, (h, w + 5)).astype(np.uint8); inn = (rng.integers(0, 256, (h, w + 3))).astype(np.uint8)
        comp = rng.integers(0, 256, (h, w // 4 + 2)).astype(np.uint8)
        in16 = rng.integers(0, 1024, (h, w + 7)).astype(np.uint16); b16 = rng.integers(0, 1024, (h, w + 1)).astype(np.uint16)
        full16 = rng.integers(0, 65536, (h, w + 7)).astype(np.uint16)
        def run(mode, i0, i1, o0dt, o0w, o1=False):
            o0 = np.zeros((h, o0w + 2), o0dt); o1a = np.zeros((h, w + 4), np.uint8) if o1 else None
            orc.orc_picture_format(mode, ptr(i0), i0.shape[1], ptr(i1) if i1 is not None else None, i1.shape[1] if i1 is not None else 0, ptr(o0), o0.shape[1],
                                   ptr(o1a) if o1 else None, o1a.shape[1] if o1 else 0, w if mode not in (1, 5) else w4, h)
            return o0, o1a
        e = np.zeros((h, w + 2), np.uint16); ref.svt_enc_msb_pack2_d(ptr(in8), in8.shape[1], ptr(inn), ptr(e), inn.shape[1], e.shape[1], w, h)
        assert np.array_equal(run(0, in8, inn, np.uint16, w)[0], e)
        e = np.zeros((h, w + 2), np.uint16); ref.svt_compressed_packmsb_c(ptr(in8), in8.shape[1], ptr(comp), ptr(e), comp.shape[1], e.shape[1], w4, h)
        assert np.array_equal(run(1, in8, comp, np.uint16, w)[0], e)
        e8 = np.zeros((h, w + 2), np.uint8); en = np.zeros((h, w + 4), np.uint8)
        ref.svt_enc_msb_un_pack2_d(ptr(full16), full16.shape[1], ptr(e8), ptr(en), e8.shape[1], en.shape[1], w, h)
        g8, gn = run(2, full16, None, np.uint8, w, o1=True)
        assert np.array_equal(g8, e8) and np.array_equal(gn, en)
        e = np.zeros((h, w + 2), np.uint16); ref.svt_convert_8bit_to_16bit_c(ptr(in8), in8.shape[1], ptr(e), e.shape[1], w, h)
        assert np.array_equal(run(3, in8, None, np.uint16, w)[0], e)
        e = np.zeros((h, w + 2), np.uint8); ref.svt_convert_16bit_to_8bit_c(ptr(full16), full16.shape[1], ptr(e), e.shape[1], w, h)
        assert np.array_equal(run(4, full16, None, np.uint8, w)[0], e)
        e = np.zeros((h, w // 4 + 2), np.uint8); ref.svt_c_pack_c(ptr(inn), inn.shape[1], ptr(e), e.shape[1], None, w4, h)
        assert np.array_equal(run(5, inn, None, np.uint8, w // 4)[0], e)
        e = np.zeros((h, w + 2), np.uint8); ref.svt_unpack_avg_c(ptr(in16), in16.shape[1], ptr(b16), b16.shape[1], ptr(e), e.shape[1], w, h)
        assert np.array_equal(run(6, in16, b16, np.uint8, w)[0], e)


def test_generate_padding(orc, ref):
    """orc_generate_padding == generate_padding / generate_padding16_bit (Common/Codec/EbMcp.c) on a buffer whose stride is the padded width."""
    rng = np.random.default_rng(77)
    for (w, h, pw, ph) in ((64, 48, 16, 8), (200, 37, 68, 68), (8, 3, 4, 2), (33, 17, 1, 5)):
        for dt in (np.uint8, np.uint16):
            buf = rng.integers(0, 250, (h + 2 * ph, w + 2 * pw)).astype(dt)
            a, b = buf.copy(), buf.copy()
            if dt == np.uint8: ref.generate_padding(ptr(a), a.shape[1], w, h, pw, ph)
            else: ref.generate_padding16_bit(ptr(a), a.shape[1] * 2, w * 2, h, pw * 2, ph)      # byte units (EbMcp.c:166-214)
            orc.orc_generate_padding(C.c_void_p(b.ctypes.data + (ph * b.shape[1] + pw) * b.itemsize), b.itemsize, b.shape[1], w, h, pw, ph)
            assert np.array_equal(a, b), (w, h, pw, ph, dt)
            assert np.array_equal(b, np.pad(buf[ph:ph + h, pw:pw + w], ((ph, ph), (pw, pw)), mode="edge"))
