"""CPU side of the per-call list pins (percall_common): every case list is built and its expectation computed here, the conditions a list has to meet are
asserted on the expectation alone -- a list that stopped reaching its edge fails here and not silently on the GPU -- and, where the reference's C path is
built, the oracle is held against the reference's `*_c` function on these very lists.  Needs no GPU."""
import numpy as np
import pytest

import percall_common as pc


# ---- the 8-candidate SAD ladders
def test_ext_all_sad_lists_meet_their_conditions(orc):
    case = pc.ext_case()
    snaps = pc.ext_run(orc.orc_ext_all_sad_8x8_16x16, case)
    cond = pc.ext_conditions(case, snaps)
    assert all(cond.values()), cond
    jobs = case["groups"][0]
    assert len(jobs) == 6 and [j.sub_sad for j in jobs] == [0, 1] * 3 and pc.EXT_SS % 4 and pc.EXT_RS % 4 and pc.EXT_SS != pc.EXT_RS
    assert all(j.src_off > 0 and j.ref_off > 0 for g in case["groups"] for j in g) and len({j.src_off for j in jobs}) == 3
    assert all(len({(j.src_off, j.ref_off) for j in g}) == 6 for g in case["groups"])
    # content: the flat block reads 255 * 64 everywhere (sub_sad: 32 rows doubled), the period-3 block 0 at every third candidate
    flat, per = snaps[0][2 * pc.EXT_FLAT], snaps[0][2 * pc.EXT_PERIODIC]
    assert (flat[288:800] == 255 * 64).all() and (snaps[0][2 * pc.EXT_FLAT + 1][288:800] == 255 * 64).all()
    e8 = per[288:800].reshape(64, 8)
    assert (e8[:, [1, 4, 7]] == 0).all() and (e8[:, [0, 2, 3, 5, 6]] > 0).all() and (e8[:, 0] == e8[:, 3]).all() and (e8[:, 2] == e8[:, 5]).all()
    # every word of the state is written by the first launch, and the bests only ever go down
    assert not (snaps[0] == pc.FILL32).any() and not (snaps[0][:, :80] == pc.NO_SAD).any()
    assert all((b[:, :80] <= a[:, :80]).all() for a, b in zip(snaps, snaps[1:])) and any((b[:, :80] < a[:, :80]).any() for a, b in zip(snaps, snaps[1:]))


def test_ext_all_sad_conditions_notice_a_list_without_its_periodic_block(orc):
    case = pc.ext_case(periodic=False)
    cond = pc.ext_conditions(case, pc.ext_run(orc.orc_ext_all_sad_8x8_16x16, case))
    assert not cond["period3_ties"] and cond["tie8"]   # the flat block still ties, all eight at once


def test_ext_eight_sad_lists(orc):
    snaps = pc.ext_run(orc.orc_ext_all_sad_8x8_16x16, pc.ext_case())
    runs = pc.eight_run(orc.orc_ext_eight_sad_32x32_64x64, snaps)
    assert len(set(pc.EIGHT_MVS[0].tolist())) == 5 and len(set(pc.EIGHT_MVS[1].tolist())) == 5
    (b0, a0), (b1, a1) = runs
    assert not (a0 == pc.FILL32).any() and (a0[:, :128] == b0[:, :128]).all()
    # record 4: all eight candidates tie, the first keeps every vector; the second launch meets the same SADs and changes nothing there
    assert (a0[4, 133:138] == pc.EIGHT_MVS[0][4]).all() and np.array_equal(a1[2:, 128:138], a0[2:, 128:138])
    # records 0 and 1 of the second launch: some bests improve, some stay
    assert (a1[:2, 128:133] < a0[:2, 128:133]).any() and (a1[:2, 128:133] == a0[:2, 128:133]).any()
    # a vector whose x crosses zero inside the group, under a negative y
    assert (a0[0, 133:138] >> 16 == 0xfffd).all() and ((a0[0, 133:138] & 0xffff).astype(np.int16) >= -12).all()


def test_ext_sad_oracle_vs_reference_c(orc, ref):
    case = pc.ext_case()
    so = pc.ext_run(orc.orc_ext_all_sad_8x8_16x16, case)
    sr = pc.ext_run(pc.as_proto(pc.EXTALL, ref.svt_ext_all_sad_calculation_8x8_16x16_c), case)
    assert all(np.array_equal(a, b) for a, b in zip(so, sr))
    eo = pc.eight_run(orc.orc_ext_eight_sad_32x32_64x64, so)
    er = pc.eight_run(pc.as_proto(pc.EXT8, ref.svt_ext_eight_sad_calculation_32x32_64x64_c), so)
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(eo, er))


# ---- variance intermediates
def test_interm_var_list(ref):
    case = pc.ivar_case()
    offs, at = case["offs"], case["at"]
    assert len(offs) == pc.IVAR_N == 23 and all(x % 2 == 1 and y % 2 == 0 and x + 32 <= pc.IVAR_STRIDE for y, x in at) and any(y % 8 for y, x in at)
    mean, mean_sq = pc.ivar_run(ref, case["plane"], offs)
    m2, q2 = pc.ivar_run(ref, case["other"], offs)
    assert np.array_equal(mean, m2) and np.array_equal(mean_sq, q2) and (case["plane"][1::2] != case["other"][1::2]).any()   # rows 0, 2, 4, 6 only
    i255, i0 = at.index((38, 3)), at.index((38, 41))
    assert 0 < i255 < 22 and 0 < i0 < 22
    assert (mean[4 * i255:4 * i255 + 4] == (255 * 32) << 3).all() and (mean_sq[4 * i255:4 * i255 + 4] == (255 * 255 * 32) << 11).all()
    assert not mean[4 * i0:4 * i0 + 4].any() and not mean_sq[4 * i0:4 * i0 + 4].any()
    assert len(set(mean.tolist())) > 60   # the 92 slots are told apart (overlapping groups share blocks)


# ---- up-sampled prediction
def test_upsampled_pred_lists_meet_their_conditions(orc):
    banks = pc.interp_banks(orc)
    lists = pc.ups_lists()
    assert [(w, h) for w, h, *_ in pc.UPS_GROUPS] == [(8, 8), (16, 16), (64, 64), (128, 128), (4, 16), (16, 4), (64, 16), (128, 64)]
    all_jobs = [j for _, _, _, jobs, _ in lists for j in jobs]
    assert {j.bank for j in all_jobs[:64]} == set(range(6)) and {j.bank for j in all_jobs[64:]} == set(range(6))
    for jobs in (all_jobs[:64], all_jobs[64:]):
        assert {(j.subpel_x_q3 > 0, j.subpel_y_q3 > 0) for j in jobs} == {(False, False), (True, False), (False, True), (True, True)}
        assert {j.subpel_x_q3 for j in jobs} == set(range(8)) == {j.subpel_y_q3 for j in jobs}
    lo = hi = differs = False
    spread = 0   # groups whose candidates straddle an integer position: more than one ref_off in the window
    for name, plane, stride, jobs, nbytes in lists:
        exp = pc.ups_run(pc.ups_by_oracle(orc), plane, stride, jobs, nbytes)
        covered = np.zeros(len(exp), bool)
        for j in jobs:
            out = exp[j.dst_off:j.dst_off + j.w * j.h].reshape(j.h, j.w)
            assert not covered[j.dst_off:j.dst_off + j.w * j.h].any()   # disjoint outputs
            covered[j.dst_off:j.dst_off + j.w * j.h] = True
            assert np.array_equal(out, pc.ups_numpy(banks, plane, stride, j)), (name, j.w, j.h, j.subpel_x_q3, j.subpel_y_q3, j.bank)
            if j.subpel_x_q3 and j.subpel_y_q3:
                lo |= bool((out == 0).any()); hi |= bool((out == 255).any())
                differs |= not np.array_equal(out, pc.ups_numpy(banks, plane, stride, j, clip_between=False))
        assert (exp[~covered] == pc.FILL8).all() and (~covered).sum() >= pc.GUARD
        if name != "mixed":   # the hook's shape: eight jobs, one window, outputs packed by w * h
            assert len(jobs) == 8 and stride == 144 and [j.dst_off for j in jobs] == [i * jobs[0].w * jobs[0].h for i in range(8)]
            assert min(j.ref_off for j in jobs) >= 3 * 144 + 3
            spread += len({j.ref_off for j in jobs}) > 1
    assert lo and hi and differs and spread >= 4
    assert len(lists[-1][3]) == 40 and lists[-1][2] % 2 == 1


def test_upsampled_pred_oracle_vs_reference_c(orc, ref):
    """the three families the reference can select (banks 0, 3, 4), job by job"""
    fo, fr = pc.ups_by_oracle(orc), pc.ups_by_reference(ref)
    seen = 0
    for name, plane, stride, jobs, _ in pc.ups_lists():
        for j in jobs:
            if j.bank in (0, 3, 4):
                e, g = np.zeros(j.w * j.h, np.uint8), np.zeros(j.w * j.h, np.uint8)
                fo(pc.vp(plane, j.ref_off), stride, pc.vp(e), j); fr(pc.vp(plane, j.ref_off), stride, pc.vp(g), j)
                assert np.array_equal(e, g), (name, j.w, j.h, j.subpel_x_q3, j.subpel_y_q3, j.bank)
                seen += 1
    assert seen >= 40


# ---- CDEF block filter
@pytest.mark.parametrize("stride,cs,dst8", pc.CDEF_RUNS)
def test_cdef_filter_block_lists_meet_their_conditions(orc, stride, cs, dst8):
    case = pc.cdef_case(stride, cs)
    jobs, img = case["jobs"], case["img"]
    assert len(jobs) == pc.CDEF_N and pc.CDEF_DST_STRIDE % 8 and stride in (144, 200)
    assert (img[:, :6] == pc.CDEF_VERY_LARGE).all() and (img[:5] == pc.CDEF_VERY_LARGE).all() and int(img[5:, 6:].max()) < (256 << cs)
    assert {(j.bw_log2, j.bh_log2) for j in jobs} == {(2, 2), (2, 3), (3, 2), (3, 3)} and {j.dir for j in jobs} == set(range(8))
    assert {(j.pri_strength > 0, j.sec_strength > 0) for j in jobs} == {(False, False), (True, False), (False, True), (True, True)}
    assert len({j.in_off for j in jobs}) > 90 and len({j.dst_off for j in jobs}) == pc.CDEF_N
    assert [j.dst_off for j in jobs] != sorted(j.dst_off for j in jobs)
    exp = pc.cdef_run(pc.cdef_by_oracle(orc, stride), img, stride, jobs, dst8)
    plain = pc.cdef_run(pc.cdef_by_oracle(orc, stride), case["plain"], stride, jobs, dst8)
    fill = pc.FILL8 if dst8 else pc.FILL16
    written = np.zeros(exp.shape, bool)
    changed = strong = reached = 0
    for j in jobs:
        y, x = divmod(j.dst_off, pc.CDEF_DST_STRIDE)
        bw, bh = 1 << j.bw_log2, 1 << j.bh_log2
        assert not written[y - 1:y + bh + 1, x - 1:x + bw + 1].any()   # a free sample all around every block
        written[y:y + bh, x:x + bw] = True
        iy, ix = divmod(j.in_off, stride)
        assert (img[iy:iy + bh, ix:ix + bw] < pc.CDEF_VERY_LARGE).all()
        if j.pri_strength or j.sec_strength:
            strong += 1
            changed += not np.array_equal(exp[y:y + bh, x:x + bw], img[iy:iy + bh, ix:ix + bw].astype(exp.dtype))
        else:
            assert np.array_equal(exp[y:y + bh, x:x + bw], img[iy:iy + bh, ix:ix + bw].astype(exp.dtype))
        reached += not np.array_equal(exp[y:y + bh, x:x + bw], plain[y:y + bh, x:x + bw])
    assert (exp[~written] == fill).all() and int((~written).sum()) > written.sum()
    assert strong >= 70 and changed > strong // 2 and reached >= 1


def test_cdef_filter_block_oracle_vs_reference_c(orc, ref):
    """the reference's function reads its input at stride 144 only"""
    for stride, cs, dst8 in pc.CDEF_RUNS:
        if stride == 144:
            case = pc.cdef_case(stride, cs)
            assert np.array_equal(pc.cdef_run(pc.cdef_by_oracle(orc, stride), case["img"], stride, case["jobs"], dst8),
                                  pc.cdef_run(pc.cdef_by_reference(ref), case["img"], stride, case["jobs"], dst8)), (cs, dst8)


# ---- the strength-pair step
def test_search_one_dual_steps(ref):
    for (sb_count, (start, end)), (m0, m1), steps in zip(pc.DUAL_SETS, pc.dual_tables(), pc.dual_run(ref)):
        assert (m0[:, 7] == m0[:, 3]).all() and (m1[:, 9] == m1[:, 5]).all() and len(steps) == 8
        for nb, (l0, l1, tot) in enumerate(steps):
            assert (l0[nb + 1:] == -7).all() and (l1[nb + 1:] == -7).all() and start <= l0[nb] < end and start <= l1[nb] < end and tot > 0
            assert 7 not in l0[:nb + 1].tolist() or 3 >= end or 3 < start   # of two equal columns the first wins
        tots = [t for _, _, t in steps]
        assert all(b <= a for a, b in zip(tots, tots[1:])) and (sb_count == 1 or tots[7] < tots[0])


# ---- single-unit forms
def test_convolve8_cases(ref):
    src, cases = pc.conv8_case()
    assert {(v, s, q) for v, s, q, _, _ in cases} == {(v, s, q) for v in (0, 1) for s in (16, 24, 64) for q in range(16)}
    assert max(w for _, _, _, w, _ in cases) == 200 and max(h for _, _, _, _, h in cases) == 150
    assert all(any(c[0] == v and c[3] > 128 for c in cases) and any(c[0] == v and c[4] > 128 for c in cases) for v in (0, 1))
    for case in cases[5::16]:
        dst = pc.conv8_expected(ref, src, case)
        inner = dst[1:-1, 2:2 + case[3]]
        outside = dst.copy(); outside[1:-1, 2:2 + case[3]] = pc.FILL8
        assert (outside == pc.FILL8).all() and len(np.unique(inner)) > 50


@pytest.mark.parametrize("pix_bytes,bd,r0,r1", pc.WIENER_FORMATS)
def test_wiener_cases(orc, pix_bytes, bd, r0, r1):
    assert pc.WIENER_SIZES == ((136, 70), (7, 5)) and (pc.WIENER_TAPS[:, 7] == 0).all()
    for w, h in pc.WIENER_SIZES:
        lo, hi, lim = pc.wiener_unclamped_range(pix_bytes, bd, r0, w, h)
        if w > 128:
            assert lo < 0 and hi > lim, (lo, hi, lim)   # the intermediate clamp cuts at both ends
        dst = pc.wiener_expected(orc, pix_bytes, bd, r0, r1, w, h)
        inner = dst[1:-1, 3:3 + w]
        outside = dst.copy(); outside[1:-1, 3:3 + w] = dst.flat[0]
        assert (outside == dst.flat[0]).all() and int(inner.max()) <= (1 << bd) - 1 and len(np.unique(inner)) > 10


def test_wiener_oracle_vs_reference_c(orc, ref):
    """units up to 128 x 128: the reference's function cannot hold a wider one"""
    w, h = pc.WIENER_SIZES[1]
    for pix_bytes, bd, r0, r1 in pc.WIENER_FORMATS:
        assert np.array_equal(pc.wiener_expected(orc, pix_bytes, bd, r0, r1, w, h), pc.wiener_by_reference(ref, pix_bytes, bd, r0, r1, w, h)), (pix_bytes, bd)
        assert np.array_equal(pc.wiener_expected(orc, pix_bytes, bd, r0, r1, 120, 70), pc.wiener_by_reference(ref, pix_bytes, bd, r0, r1, 120, 70)), (pix_bytes, bd)


def test_jnt_convolve_cases(orc, ref):
    banks = pc.interp_banks(orc)
    cases = pc.jnt_cases()
    assert {(c[1], c[2], c[7][0]) for c in cases} == {(bd, v, j) for bd in (8, 10, 12) for v in range(4) for j in (0, 1)}
    assert {(c[3], c[4]) for c in cases} == set(pc.BIG_SIZES) and max(w for w, _ in pc.BIG_SIZES) > 128 and max(h for _, h in pc.BIG_SIZES) > 128
    for case in cases:
        pb, bd, variant, w, h = case[:5]
        cb, out = pc.jnt_expected(ref, banks, case)
        (cshape, coff, dshape, doff) = pc.jnt_layout(w, h)
        assert cshape[1] != dshape[1] != w and cshape[1] != pc.JNT_SS
        inner_cb, inner = cb[1:h + 1, 2:2 + w], out[1:h + 1, 1:1 + w]
        assert (cb[0] == 4321).all() and (cb[:, :2] == 4321).all() and (cb[:, 2 + w:] == 4321).all() and len(np.unique(inner_cb)) > 20
        assert (out[0] == out.flat[0]).all() and (out[:, 0] == out.flat[0]).all() and (out[:, 1 + w:] == out.flat[0]).all() and len(np.unique(inner)) > 20


def test_masked_compound_cases(ref):
    for kind, pb, bd in pc.MASK_KINDS:
        for w, h in pc.BIG_SIZES:
            a, b = pc.mask_inputs(kind, bd, w, h)
            assert a.shape[1] != b.shape[1] and w not in (a.shape[1], b.shape[1]) and a.itemsize == pb
            m = [pc.mask_expected(ref, kind, bd, w, h, inv) for inv in (0, 1)]
            assert (m[0][w * h:] == pc.FILL8).all() and (m[0][:w * h].astype(int) + m[1][:w * h] == 64).all()
            assert int(m[0][:w * h].min()) == 38 and int(m[0][:w * h].max()) >= 45
    for pb, bd in pc.JNT_FORMATS:
        for w, h in pc.BIG_SIZES:
            outs = []
            for subw, subh in ((0, 0), (1, 1), (1, 0), (0, 1)):
                mk = pc.blend_mask(w, h, subw, subh)
                assert mk.shape[1] != w << subw
                dst = pc.blend_expected(ref, pb, bd, w, h, subw, subh)
                assert (dst[0] == dst.flat[0]).all() and (dst[:, 0] == dst.flat[0]).all() and (dst[:, 1 + w:] == dst.flat[0]).all()
                outs.append(dst[1:h + 1, 1:1 + w].copy())
            assert all(not np.array_equal(outs[0], o) for o in outs[1:])


@pytest.mark.parametrize("pix_bytes", [1, 2])
def test_sgr_flt_proj_cases(orc, pix_bytes):
    assert pc.SGR_SIZES[0] == (300, 280) and 280 > 256 and 300 > 256
    for w, h in pc.SGR_SIZES:
        arrays = pc.sgr_inputs(pix_bytes, w, h)
        assert len({a.shape[1] for a in arrays} | {w}) == 5
        seen = set()
        for radii in pc.SGR_RADII:
            sums, xq, err = pc.sgr_expected(orc, pix_bytes, w, h, radii)
            assert (sums[0] > 0) == (radii[0] > 0) and (sums[2] > 0) == (radii[1] > 0) and (sums[1] != 0) == (radii[0] > 0 and radii[1] > 0)
            assert (radii[0] > 0 or xq[0] == 0) and (radii[1] > 0 or xq[1] == 0) and (xq[0] != 0 or xq[1] != 0) and err > 0
            seen.add((tuple(sums), tuple(xq), err))
        assert len(seen) == 3
        plain = pc.sgr_expected(orc, pix_bytes, w, h, (0, 0))[2]
        assert plain > 0 and all(plain != s[2] for s in seen)


def test_sgr_flt_proj_oracle_vs_reference_c(orc, ref):
    for pix_bytes in (1, 2):
        for w, h in pc.SGR_SIZES:
            for radii in pc.SGR_RADII + ((0, 0),):
                sums, xq, err = pc.sgr_expected(orc, pix_bytes, w, h, radii)
                rxq, rerr = pc.sgr_by_reference(ref, pix_bytes, w, h, radii)
                assert err == rerr and (radii == (0, 0) or np.array_equal(xq, rxq)), (pix_bytes, w, h, radii)
