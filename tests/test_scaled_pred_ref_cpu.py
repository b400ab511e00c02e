"""CPU: the numpy restatement of tests/scaled_common.py and the host entry points against the reference itself (oracle/_ref/libsvtav1_ref.so).
The restatement equals svt_av1_convolve_2d_scale_c / svt_av1_highbd_convolve_2d_scale_c on the whole case list the GPU test launches; svt_hip_scale_factors
equals svt_av1_setup_scale_factors_for_frame and svt_hip_scaled_block_params equals compute_subpel_params; at step 1024 the 2-D formula gives what the
reference's unscaled dispatch gives; and each of four deliberately wrong variants changes a named case."""
import ctypes as C

import numpy as np
import pytest

import scaled_common as sc

FMTS = [pytest.param(bd, dt, id="%s-%d" % (np.dtype(dt).name, bd)) for bd, dt in sc.FMTS]
TABLES = ["sub_pel_filters_8", "sub_pel_filters_8smooth", "sub_pel_filters_8sharp", "bilinear_filters", "sub_pel_filters_4", "sub_pel_filters_4smooth"]   # bank 0 .. 5


class InterpFilterParams(C.Structure):
    _fields_ = [("filter_ptr", C.c_void_p), ("taps", C.c_uint16), ("subpel_shifts", C.c_uint16), ("interp_filter", C.c_int)]


class ConvolveParams(C.Structure):
    _fields_ = [("ref", C.c_int32), ("do_average", C.c_int32), ("dst", C.c_void_p), ("dst_stride", C.c_int32), ("round_0", C.c_int32), ("round_1", C.c_int32),
                ("plane", C.c_int32), ("is_compound", C.c_int32), ("use_jnt_comp_avg", C.c_int32), ("fwd_offset", C.c_int32), ("bck_offset", C.c_int32),
                ("use_dist_wtd_comp_avg", C.c_int32)]


class RefScaleFactors(C.Structure):
    _fields_ = [("x_scale_fp", C.c_int32), ("y_scale_fp", C.c_int32), ("x_step_q4", C.c_int32), ("y_step_q4", C.c_int32), ("scale_value_x", C.c_void_p),
                ("scale_value_y", C.c_void_p)]


class SubpelParams(C.Structure):
    _fields_ = [("xs", C.c_int32), ("ys", C.c_int32), ("subpel_x", C.c_int32), ("subpel_y", C.c_int32)]


class MV(C.Structure):
    _fields_ = [("row", C.c_int16), ("col", C.c_int16)]


def conv_params(bd, compound, do_average, buf, kind=(1, 0, 0)):
    """get_conv_params_no_round (Common/Codec/convolve.h:44), and what its callers add for a distance-weighted pair"""
    r0 = 3 + max(0, bd + 7 - 3 + 2 - 16)
    dist = int(kind[0] == 2)
    return ConvolveParams(0, do_average, buf.ctypes.data if buf is not None else None, buf.shape[1] if buf is not None else 0, r0, 7 if compound else 14 - r0, 0,
                          int(compound), dist, kind[1], kind[2], dist)


def filter_params(ref, bank):
    return InterpFilterParams(C.addressof(C.c_int16.in_dll(ref, TABLES[bank])), 8, 16, bank if bank < 4 else bank - 4)


def address(plane, x, y):
    root, ox, oy = plane
    return root.ctypes.data + ((oy + y) * root.shape[1] + ox + x) * root.itemsize


def ref_scale(ref, dt, bd, plane, x, y, dst, b, sx, xs, sy, ys, cp):
    fx, fy = filter_params(ref, b.bank_x), filter_params(ref, b.bank_y)
    args = [C.c_void_p(address(plane, x, y)), plane[0].shape[1], C.c_void_p(dst.ctypes.data), dst.shape[1], b.w, b.h, C.byref(fx), C.byref(fy), sx, xs, sy, ys, C.byref(cp)]
    if dt == np.uint8: ref.svt_av1_convolve_2d_scale_c(*args)
    else: ref.svt_av1_highbd_convolve_2d_scale_c(*args, bd)


def ref_job(ref, b, planes, bd, dt):
    """one ScaledBlk through the reference: reference 0 into ConvolveParams::dst, reference 1 with do_average, as its callers do for a pair"""
    out, buf = np.zeros((b.h, b.w), dt), np.zeros((b.h, b.w), np.uint16)
    kind = (b.compound, b.fwd_offset, b.bck_offset)
    ref_scale(ref, dt, bd, planes[0], b.pos0_x, b.pos0_y, out, b, b.subpel0_x, b.xs0, b.subpel0_y, b.ys0, conv_params(bd, b.compound != 0, 0, buf if b.compound else None, kind))
    if b.compound:
        ref_scale(ref, dt, bd, planes[1], b.pos1_x, b.pos1_y, out, b, b.subpel1_x, b.xs1, b.subpel1_y, b.ys1, conv_params(bd, True, 1, buf, kind))
    return out


# ---------------------------------------------------------------- the restatement on the GPU case lists
def test_taps_are_the_reference_tables(ref):
    for bank, name in enumerate(TABLES):
        assert np.array_equal(np.ctypeslib.as_array((C.c_int16 * 8 * 16).in_dll(ref, name)), sc.taps()[bank]), name


@pytest.mark.parametrize("bd,dt", FMTS)
@pytest.mark.parametrize("which", ["single", "compound"])
def test_restatement_equals_the_reference_on_the_gpu_lists(ref, which, bd, dt):
    c = sc.single_cases() if which == "single" else sc.compound_cases()
    exp, planes, mx = sc.dst_view(sc.expected(which, bd, dt)), sc.planes_of(bd, dt), (1 << bd) - 1
    low = high = False
    for i, (b, d) in enumerate(zip(c.jobs, c.desc)):
        e = exp[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w]
        got = ref_job(ref, b, planes, bd, dt)
        assert np.array_equal(got, e), (i, d, np.argwhere(got != e)[:4])
        if d["content"] == "max": assert (e == mx).all(), (i, d)                 # closed form: a flat maximum stays the maximum in every format
        if d["content"] == "noise":
            raw = sc.predict_job(b, planes, bd, clip=False)
            low, high = low or bool((raw < 0).any()), high or bool((raw > mx).any())
    assert low and high                                                           # 0 / max noise: both clips bind
    root = sc.expected(which, bd, dt)
    outside = np.ones(root.shape, bool)
    for b in c.jobs: sc.dst_view(outside)[b.dst_y:b.dst_y + b.h, b.dst_x:b.dst_x + b.w] = False
    assert np.array_equal(root[outside], sc.dst_root(c, bd, dt)[outside])


# ---------------------------------------------------------------- scale factors and positions
def size_grid():
    pairs = set()
    for dim in (64, 352, 1920, 3840):
        for d in range(9, 17):
            small = (dim * 8 + d // 2) // d
            pairs |= {(dim, small), (small, dim)}                                 # every super-resolution denominator, both ways round
    for this in (16, 17, 100, 1081):
        pairs |= {(2 * this - 1, this), (2 * this, this), (2 * this + 1, this)}   # 2 * this >= other, from both sides
    for other in (1, 5, 67):
        pairs |= {(other, 16 * other - 1), (other, 16 * other), (other, 16 * other + 1)}   # this <= 16 * other, from both sides
    pairs |= {(640, 640), (1, 1), (65535, 65535), (65535, 32768)}
    return sorted(pairs)


def test_scale_factors_equal_the_reference(ref, pkg):
    L, grid = pkg.lib(), size_grid()
    invalid = 0
    for (ow, tw) in grid:
        for (oh, th) in grid[::3]:
            r, mine = RefScaleFactors(), pkg.ScaleFactors()
            ref.svt_av1_setup_scale_factors_for_frame(C.byref(r), ow, oh, tw, th)
            rc = L.svt_hip_scale_factors(ow, oh, tw, th, C.byref(mine))
            if r.x_scale_fp == -1:
                assert r.y_scale_fp == -1 and rc == 2 and (mine.x_scale_fp, mine.y_scale_fp) == (-1, -1) and sc.scale_factors(ow, oh, tw, th) is None, (ow, oh, tw, th)
                invalid += 1
            else:
                want = (r.x_scale_fp, r.y_scale_fp, r.x_step_q4, r.y_step_q4)
                assert rc == 0 and (mine.x_scale_fp, mine.y_scale_fp, mine.x_step_q4, mine.y_step_q4) == want == sc.scale_factors(ow, oh, tw, th), (ow, oh, tw, th)
                assert 64 <= r.x_step_q4 <= 2048 and 64 <= r.y_step_q4 <= 2048
    assert invalid > 50 and len(grid) > 80


def my_block_params(L, pkg, sf, pre_x, pre_y, mv_row, mv_col, ss_x, ss_y, fw, fh):
    o = [C.c_int32() for _ in range(6)]
    L.svt_hip_scaled_block_params(C.byref(pkg.ScaleFactors(*sf)), pre_x, pre_y, mv_row, mv_col, ss_x, ss_y, fw, fh, *[C.byref(v) for v in o])
    return tuple(v.value for v in o)


def ref_block_params(ref, sizes, pre_x, pre_y, mv_row, mv_col, ss_x, ss_y):
    r, sp, py, px = RefScaleFactors(), SubpelParams(), C.c_int32(), C.c_int32()
    ref.svt_av1_setup_scale_factors_for_frame(C.byref(r), *sizes)
    ref.compute_subpel_params.argtypes = [C.c_int16, C.c_int16, MV, C.c_void_p, C.c_uint16, C.c_uint16, C.c_uint8, C.c_uint8, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
    ref.compute_subpel_params(pre_y, pre_x, MV(mv_row, mv_col), C.addressof(r), sizes[0], sizes[1], 16, 16, None, ss_y, ss_x, C.addressof(sp), C.addressof(py), C.addressof(px))
    return px.value, py.value, sp.subpel_x, sp.subpel_y, sp.xs, sp.ys


def test_block_params_equal_compute_subpel_params(ref, pkg):
    """NULL MacroBlockD: the scaled branch never reads it.  The unscaled size pair of the list is left to the unscaled branch (it needs the MacroBlockD)."""
    L = pkg.lib()
    n = 0
    for sizes, pre_x, pre_y, mv_row, mv_col, ss_x, ss_y in sc.clamp_cases():      # the builder asserts: each clamp binds and does not, negative positions, both sub-samplings
        sf = sc.scale_factors(*sizes)
        mine = my_block_params(L, pkg, sf, pre_x, pre_y, mv_row, mv_col, ss_x, ss_y, sizes[0], sizes[1])
        assert mine == sc.block_params(sf, pre_x, pre_y, mv_row, mv_col, ss_x, ss_y, sizes[0], sizes[1])
        if sf[0] != 16384 or sf[1] != 16384:
            assert mine == ref_block_params(ref, sizes, pre_x, pre_y, mv_row, mv_col, ss_x, ss_y), (sizes, pre_x, pre_y, mv_row, mv_col, ss_x, ss_y)
            n += 1
    assert n == 252


# ---------------------------------------------------------------- step 1024: the 2-D formula against the reference's unscaled dispatch
@pytest.fixture
def dispatch(ref):
    """the reference with its convolve[sub_x][sub_y][compound] tables filled from the function pointers the `ref` fixture has set up, as the encoder does at start"""
    ref.asm_set_convolve_asm_table()
    ref.asm_set_convolve_hbd_asm_table()
    return ref


@pytest.mark.parametrize("bd,dt", FMTS)
def test_unscaled_half_of_a_pair_equals_the_reference_dispatch(dispatch, bd, dt):
    ref = dispatch
    """svt_inter_predictor / svt_highbd_inter_predictor with xs = ys = 1024 go to jnt_convolve_{2d_copy, x, y, 2d}; the other reference of the pair is scaled and goes
    to convolve_2d_scale.  Either order, at all four (phase-x zero / non-zero, phase-y zero / non-zero) combinations."""
    planes, rng, n = sc.planes_of(bd, dt), np.random.default_rng(5), 0
    kinds = [(1, 0, 0), (2, 9, 7), (2, 3, 13)]
    for (w, h) in [(4, 8), (8, 4), (16, 16), (32, 64), (64, 16)]:
        for qx, qy in [(0, 0), (5, 0), (0, 11), (9, 14)]:
            for unscaled_first in (True, False):
                kind = kinds[n % 3]
                fx, fy = n % 4, (n // 4) % 4                                      # InterpFilter of x / y
                steps = [(1024, 1024), [(1536, 1024), (2048, 2048), (683, 910)][n % 3]]
                phases = [(qx << 6, qy << 6), (int(rng.integers(0, 1024)), int(rng.integers(0, 1024)))]
                if not unscaled_first: steps, phases = steps[::-1], phases[::-1]
                pos = [(int(rng.integers(8, 100)), int(rng.integers(8, 100))) for _ in range(2)]
                b = sc.ScaledBlk(pos0_x=pos[0][0], pos0_y=pos[0][1], pos1_x=pos[1][0], pos1_y=pos[1][1], subpel0_x=phases[0][0], subpel0_y=phases[0][1], subpel1_x=phases[1][0],
                                 subpel1_y=phases[1][1], xs0=steps[0][0], ys0=steps[0][1], xs1=steps[1][0], ys1=steps[1][1], w=w, h=h, bank_x=sc.bank_of(fx, w),
                                 bank_y=sc.bank_of(fy, h), compound=kind[0], fwd_offset=kind[1], bck_offset=kind[2])
                out, buf, sf = np.zeros((h, w), dt), np.zeros((h, w), np.uint16), RefScaleFactors()
                for r in (0, 1):
                    cp = conv_params(bd, True, r, buf, kind)
                    sp = SubpelParams(steps[r][0], steps[r][1], phases[r][0], phases[r][1])
                    args = [C.c_void_p(address(planes[r], *pos[r])), planes[r][0].shape[1], C.c_void_p(out.ctypes.data), w, C.byref(sp), C.byref(sf), w, h, C.byref(cp),
                            C.c_uint32(fy | (fx << 16)), 0]
                    if dt == np.uint8: ref.svt_inter_predictor(*args)
                    else: ref.svt_highbd_inter_predictor(*args, bd)
                want = sc.predict_job(b, planes, bd)
                assert np.array_equal(out, want), ((w, h), (qx, qy), unscaled_first, kind, np.argwhere(out != want)[:4])
                n += 1
    assert n == 40


@pytest.mark.parametrize("bd,dt", FMTS)
def test_single_reference_at_step_1024_equals_the_sr_dispatch(dispatch, bd, dt):
    """the same for one reference: convolve_{2d_copy, x, y, 2d}_sr"""
    ref, planes, sf = dispatch, sc.planes_of(bd, dt), RefScaleFactors()
    for n, ((w, h), (qx, qy)) in enumerate(((s, q) for s in [(4, 4), (8, 16), (32, 8), (64, 64)] for q in [(0, 0), (3, 0), (0, 12), (15, 1)])):
        fx, fy = n % 4, (n // 2) % 4
        b = sc.ScaledBlk(pos0_x=20 + n, pos0_y=9 + n, subpel0_x=qx << 6, subpel0_y=qy << 6, xs0=1024, ys0=1024, w=w, h=h, bank_x=sc.bank_of(fx, w), bank_y=sc.bank_of(fy, h))
        out, cp, sp = np.zeros((h, w), dt), conv_params(bd, False, 0, None), SubpelParams(1024, 1024, qx << 6, qy << 6)
        args = [C.c_void_p(address(planes[0], b.pos0_x, b.pos0_y)), planes[0][0].shape[1], C.c_void_p(out.ctypes.data), w, C.byref(sp), C.byref(sf), w, h, C.byref(cp),
                C.c_uint32(fy | (fx << 16)), 0]
        if dt == np.uint8: ref.svt_inter_predictor(*args)
        else: ref.svt_highbd_inter_predictor(*args, bd)
        assert np.array_equal(out, sc.predict_job(b, planes, bd)), ((w, h), (qx, qy))


# ---------------------------------------------------------------- sensitivity: each wrong variant changes a named case
def test_wrong_variants_change_named_cases(ref, pkg):
    L = pkg.lib()
    # SCALE_EXTRA_OFF dropped: the block at the picture's origin with a zero vector, reference 1.5 times as wide
    sizes, case = (1920, 1080, 1280, 1080), (0, 0, 0, 0, 0, 0)
    sf = sc.scale_factors(*sizes)
    good = sc.block_params(sf, *case, sizes[0], sizes[1])
    assert good == ref_block_params(ref, sizes, *case) == my_block_params(L, pkg, sf, *case, sizes[0], sizes[1]) and good[2] == 288
    assert sc.block_params(sf, *case, sizes[0], sizes[1], variant="no_extra_off")[2] == 256
    # unsigned rounding in scaled_x: a position left of the picture that lands on a half
    sizes, case = (1000, 700, 777, 555), (0, 0, 0, -1508, 0, 0)
    sf = sc.scale_factors(*sizes)
    good = sc.block_params(sf, *case, sizes[0], sizes[1])
    assert good == ref_block_params(ref, sizes, *case) == my_block_params(L, pkg, sf, *case, sizes[0], sizes[1]) and good[0] < 0
    assert sc.block_params(sf, *case, sizes[0], sizes[1], variant="unsigned_round") != good
    # an 8-bit round_0 at bit depth 12, and the filter index taken as >> 4: the first random 16 x 16 job of the single list at steps (1536, 1024)
    c = sc.single_cases()
    i = next(i for i, d in enumerate(c.desc) if d["size"] == (16, 16) and d["steps"] == (1536, 1024) and d["content"] == "random")
    b = c.jobs[i]
    for bd, dt, variant in [(12, np.uint16, "round0_8bit"), (8, np.uint8, "filter_idx_shift4"), (12, np.uint16, "filter_idx_shift4")]:
        planes = sc.planes_of(bd, dt)
        good = sc.predict_job(b, planes, bd)
        assert np.array_equal(good, ref_job(ref, b, planes, bd, dt)) and not np.array_equal(sc.predict_job(b, planes, bd, variant=variant), good), (bd, variant)
