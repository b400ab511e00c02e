"""Case lists of the per-call list kernels (csrc/percall.hip, the list tail of csrc/cdef.hip, svt_hip_cdef_search_one_dual_dev) beyond the one way the per-call
table (csrc/rtcd_hip.cpp) drives them: many jobs per launch, strides that are not the packed row length, non-zero per-job offsets, sizes above 128.
Shared by test_percall_lists_ref_cpu.py (the expectations alone: oracle against the reference's `*_c` functions, and the conditions every list has to
meet) and test_percall_lists_gpu.py (the same lists through the entry points).  Every builder is deterministic and cached: both files see the same arrays,
and nothing here writes to an array after it has been returned.

Layouts are the ones of include/svt_hip.h.  Every expected buffer starts as the pre-fill pattern (FILL*) and is compared whole."""
import ctypes as C
import functools

import numpy as np

from conftest import load_package

pkg = load_package()
VP = C.c_void_p
FILL8, FILL16, FILL32, FILL64 = 0xA5, 0xA5A5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
NO_SAD = 0xffffffff
GUARD = 64   # words / bytes of pre-fill kept behind the last job's output


class FilterParams(C.Structure):   # InterpFilterParams
    _fields_ = [("filter_ptr", VP), ("taps", C.c_uint16), ("subpel_shifts", C.c_uint16), ("interp_filter", C.c_uint8)]


class ConvParams(C.Structure):   # ConvolveParams
    _fields_ = [("ref", C.c_int32), ("do_average", C.c_int32), ("dst", VP), ("dst_stride", C.c_int32), ("round_0", C.c_int32), ("round_1", C.c_int32),
                ("plane", C.c_int32), ("is_compound", C.c_int32), ("use_jnt_comp_avg", C.c_int32), ("fwd_offset", C.c_int32), ("bck_offset", C.c_int32),
                ("use_dist_wtd_comp_avg", C.c_int32)]


class SgrParams(C.Structure):   # SgrParamsType
    _fields_ = [("r", C.c_int32 * 2), ("s", C.c_int32 * 2)]


# the reference's `*_c` prototypes (the dispatch-table rows of test_rtcd_gpu.py)
EXTALL = C.CFUNCTYPE(None, VP, C.c_uint32, VP, C.c_uint32, C.c_uint32, VP, VP, VP, VP, VP, VP, C.c_uint8)
EXT8 = C.CFUNCTYPE(None, VP, VP, VP, VP, VP, C.c_uint32, VP)
IVAR = C.CFUNCTYPE(None, VP, C.c_uint16, VP, VP)
UPS = C.CFUNCTYPE(None, VP, VP, C.c_int, C.c_int, VP, VP, C.c_int, C.c_int, C.c_int, C.c_int, VP, C.c_int, C.c_int)
CFB = C.CFUNCTYPE(None, VP, VP, C.c_int32, VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32)
ONEDUAL = C.CFUNCTYPE(C.c_uint64, VP, VP, C.c_int, VP, C.c_int, C.c_int, C.c_int)
CONV8 = C.CFUNCTYPE(None, VP, C.c_ssize_t, VP, C.c_ssize_t, VP, C.c_int, VP, C.c_int, C.c_int, C.c_int)
WIENER = C.CFUNCTYPE(None, VP, C.c_ssize_t, VP, C.c_ssize_t, VP, VP, C.c_int32, C.c_int32, C.POINTER(ConvParams))
WIENERH = C.CFUNCTYPE(None, VP, C.c_ssize_t, VP, C.c_ssize_t, VP, VP, C.c_int32, C.c_int32, C.POINTER(ConvParams), C.c_int32)
CONV = C.CFUNCTYPE(None, VP, C.c_int32, VP, C.c_int32, C.c_int32, C.c_int32, C.POINTER(FilterParams), C.POINTER(FilterParams), C.c_int32, C.c_int32,
                   C.POINTER(ConvParams))
CONVH = C.CFUNCTYPE(None, VP, C.c_int32, VP, C.c_int32, C.c_int32, C.c_int32, C.POINTER(FilterParams), C.POINTER(FilterParams), C.c_int32, C.c_int32,
                    C.POINTER(ConvParams), C.c_int32)
DWM = C.CFUNCTYPE(None, VP, C.c_uint8, VP, C.c_int, VP, C.c_int, C.c_int, C.c_int)
DWMH = C.CFUNCTYPE(None, VP, C.c_uint8, VP, C.c_int, VP, C.c_int, C.c_int, C.c_int, C.c_int)
DWM16 = C.CFUNCTYPE(None, VP, C.c_uint8, VP, C.c_int, VP, C.c_int, C.c_int, C.c_int, C.POINTER(ConvParams), C.c_int)
BLD16 = C.CFUNCTYPE(None, VP, C.c_uint32, VP, C.c_uint32, VP, C.c_uint32, VP, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ConvParams))
BLD16H = C.CFUNCTYPE(None, VP, C.c_uint32, VP, C.c_uint32, VP, C.c_uint32, VP, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ConvParams), C.c_int)
PROJSUB = C.CFUNCTYPE(None, VP, C.c_int, C.c_int, C.c_int, VP, C.c_int, C.c_int, VP, C.c_int, VP, C.c_int, VP, VP)
PROJERR = C.CFUNCTYPE(C.c_int64, VP, C.c_int32, C.c_int32, C.c_int32, VP, C.c_int32, VP, C.c_int32, VP, C.c_int32, VP, VP)


def vp(a, off=0):
    """pointer to byte `off` of a numpy array"""
    return C.c_void_p(a.ctypes.data + off)


def as_proto(T, f):
    """the reference's `*_c` function behind an explicit prototype"""
    return T(C.cast(f, C.c_void_p).value)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def interp_banks(orc):
    return np.ctypeslib.as_array((C.c_int16 * 8 * 16 * 6).in_dll(orc, "orc_interp_kernels")).copy()


def sample_dtype(pix_bytes):
    return np.uint8 if pix_bytes == 1 else np.uint16


def extreme_plane(rng, shape, mx, dtype):
    """noise on the left third, a 0 / max checkerboard in the middle, random 0 / max samples on the right"""
    h, w = shape
    p = rng.integers(0, mx + 1, shape)
    yy, xx = np.mgrid[0:h, 0:w]
    a, b = w // 3, 2 * w // 3
    p[:, a:b] = (((yy + xx) & 1) * mx)[:, a:b]
    p[:, b:] = rng.integers(0, 2, (h, w - b)) * mx
    return p.astype(dtype)


# ------------------------------------------------------------------------------------------------ svt_hip_ext_all_sad_8x8_16x16_batch_dev
def mv_word(y, x):
    return ((y & 0xffff) << 16) | (x & 0xffff)


def step_mv(mv, k):
    """candidate k of a group: x advances by 4, the y half is untouched"""
    return (mv & 0xffff0000) | ((mv + 4 * k) & 0xffff)


EXT_SS, EXT_RS = 203, 237                     # source / reference strides: different, neither a multiple of 4
EXT_SRC_AT = ((1, 3), (5, 70), (2, 135))      # (y, x) of the three 64 x 64 source blocks
EXT_WIN_AT = ((2, 5), (3, 121), (71, 50))     # (y, x) of each block's 64 x 96 window in the reference plane
EXT_GROUPS = ((0, mv_word(-3, -12)), (16, mv_word(-3, 40)), (8, mv_word(5, -64)))   # (x of candidate 0 in the window, mv word) of the three launches
EXT_NOISE, EXT_FLAT, EXT_PERIODIC = 0, 1, 2   # the blocks


@functools.lru_cache(maxsize=None)
def ext_case(periodic=True):
    """n = 6 jobs = 3 blocks x sub_sad 0 / 1 (job 2 * block + sub).  The sub_sad 1 job of a block reads its window one column further right: same source,
    another reference.  periodic=False replaces the period-3 window by noise (the CPU test shows that its conditions notice)."""
    rng = np.random.default_rng(4101)
    src = rng.integers(0, 256, (72, EXT_SS)).astype(np.uint8)
    ref = rng.integers(0, 256, (140, EXT_RS)).astype(np.uint8)
    blk = lambda b: src[EXT_SRC_AT[b][0]:EXT_SRC_AT[b][0] + 64, EXT_SRC_AT[b][1]:EXT_SRC_AT[b][1] + 64]
    win = lambda b: ref[EXT_WIN_AT[b][0]:EXT_WIN_AT[b][0] + 64, EXT_WIN_AT[b][1]:EXT_WIN_AT[b][1] + 96]
    # noise: the block itself, slightly disturbed, sits at window column 21 = candidate 5 of the second group: its bests improve there
    win(EXT_NOISE)[:] = np.clip(np.pad(blk(EXT_NOISE), ((0, 0), (21, 11)), mode="edge").astype(np.int32) + rng.integers(-6, 7, (64, 96)), 0, 255)
    blk(EXT_FLAT)[:] = 255
    win(EXT_FLAT)[:] = 0
    if periodic:   # candidates k and k + 3 of any group read identical samples
        win(EXT_PERIODIC)[:] = np.tile(rng.integers(0, 256, (64, 3)), (1, 32))
        blk(EXT_PERIODIC)[:] = win(EXT_PERIODIC)[:, 1:65]
    groups = []
    for xoff, mv in EXT_GROUPS:
        jobs = (pkg.ExtSadJob * 6)()
        for b in range(3):
            for sub in (0, 1):
                j = jobs[2 * b + sub]
                j.src_off = EXT_SRC_AT[b][0] * EXT_SS + EXT_SRC_AT[b][1]
                j.ref_off = EXT_WIN_AT[b][0] * EXT_RS + EXT_WIN_AT[b][1] + xoff + sub
                j.mv, j.sub_sad = mv, sub
        groups.append(jobs)
    state = np.full((6, 800), FILL32, np.uint32)
    state[:, :80] = NO_SAD
    return dict(src=frozen(src), ref=frozen(ref), groups=groups, state=frozen(state))


def ext_run(fn, case):
    """the state after each of the three launches, by a function with the reference's signature (the oracle's, or `*_c`)"""
    st = case["state"].copy()
    snaps = []
    for jobs in case["groups"]:
        for i, j in enumerate(jobs):
            r = st[i]
            fn(vp(case["src"], j.src_off), EXT_SS, vp(case["ref"], j.ref_off), EXT_RS, C.c_uint32(j.mv), vp(r, 0), vp(r, 4 * 64), vp(r, 4 * 80), vp(r, 4 * 144), vp(r, 4 * 160),
               vp(r, 4 * 288), j.sub_sad)
        snaps.append(st.copy())
    return snaps


def ext_conditions(case, snaps):
    """what the list has to exercise, read off the expected states alone"""
    before = [case["state"]] + snaps[:-1]
    tie = {8: False, 16: False}        # a new minimum shared by two candidates of a group, the earlier one keeps the vector
    period3 = 0                        # ... shared by candidates k and k + 3 and not by all eight: what the period-3 window gives, at every block
    survives = {8: False, 16: False}   # a best that meets an equal SAD in a later group and stays
    for g, (jobs, prev, now) in enumerate(zip(case["groups"], before, snaps)):
        for i, j in enumerate(jobs):
            for size, best, mvs, eight, n in ((8, 0, 80, 288, 64), (16, 64, 144, 160, 16)):
                e = now[i, eight:eight + 8 * n].reshape(n, 8).astype(np.int64)
                m, first, shared = e.min(axis=1), e.argmin(axis=1), (e == e.min(axis=1)[:, None]).sum(axis=1)
                pb = prev[i, best:best + n].astype(np.int64)
                won = m < pb
                for k in np.nonzero(won & (shared >= 2))[0]:
                    assert now[i, mvs + k] == step_mv(j.mv, int(first[k])) and now[i, best + k] == m[k]
                    tie[size] = True
                    period3 += bool(shared[k] < 8 and first[k] < 5 and e[k, first[k] + 3] == m[k])
                keep = (m == pb) & (g > 0)
                if keep.any():
                    assert np.array_equal(now[i, mvs:mvs + n][keep], prev[i, mvs:mvs + n][keep])
                    survives[size] = True
    first_mvs = snaps[0][:, 80:160]
    return dict(tie8=tie[8], tie16=tie[16], period3_ties=period3 >= 2 * 80, survives8=survives[8], survives16=survives[16],
                # group 0: y = -3 in every stored vector, and some x at or past zero (candidates 3 ..): the carry out of x never reached y
                y_half_intact=bool((first_mvs >> 16 == 0xfffd).all()), x_crossed_zero=bool(((first_mvs & 0xffff) < 0x8000).any()),
                x_stayed_negative=bool(((first_mvs & 0xffff) >= 0x8000).any()),
                # (the flat block's two windows are both all 0: its two states are equal, as they must be)
                same_source_other_reference=all(not np.array_equal(snaps[-1][2 * b, 80:160], snaps[-1][2 * b + 1, 80:160]) for b in (EXT_NOISE, EXT_PERIODIC)))


# ------------------------------------------------------------------------------------------------ svt_hip_ext_eight_sad_32x32_64x64_batch_dev
EIGHT_MVS = (np.array([mv_word(-3, -12), mv_word(7, 100), mv_word(-1, -4), mv_word(0, 0), mv_word(-200, 32764)], np.uint32),
             np.array([mv_word(2, -28), mv_word(-9, 8), mv_word(1, 1), mv_word(-5, -16), mv_word(33, -32768)], np.uint32))


def eight_inputs(snaps):
    """two launches of n = 5: the 16x16 SADs of the ladder lists above (launch 0: after the last group, launch 1: records 0 and 1 take an earlier group's,
    the rest meet their own SADs again), record 4 with equal columns: all eight candidates tie"""
    rng = np.random.default_rng(4102)
    first = np.full((5, 170), FILL32, np.uint32)
    first[:4, :128] = snaps[-1][:4, 160:288]
    first[4, :128] = np.repeat(rng.integers(100, 16320, 16), 8)
    first[:, 128:133] = NO_SAD
    return first


def eight_run(fn, snaps):
    """[(state before, state after)] of the two launches"""
    out = []
    st = eight_inputs(snaps)
    for launch, mvs in enumerate(EIGHT_MVS):
        if launch == 1:
            st[0, :128] = snaps[1][0, 160:288]
            st[1, :128] = snaps[0][1, 160:288]
        before = st.copy()
        for i in range(5):
            r = st[i]
            fn(vp(r, 0), vp(r, 4 * 128), vp(r, 4 * 132), vp(r, 4 * 133), vp(r, 4 * 137), C.c_uint32(int(mvs[i])), vp(r, 4 * 138))
        out.append((before, st.copy()))
    return out


# ------------------------------------------------------------------------------------------------ svt_hip_interm_var_four8x8_batch_dev
IVAR_STRIDE, IVAR_N = 83, 23


@functools.lru_cache(maxsize=None)
def ivar_case():
    """23 groups of four 8x8 blocks at odd columns and even rows, an all-255 and an all-0 group among them; `other` differs from
    `plane` on the rows the function does not read (the odd ones)"""
    rng = np.random.default_rng(4103)
    plane = rng.integers(0, 256, (48, IVAR_STRIDE)).astype(np.uint8)
    plane[38:46, 3:35] = 255
    plane[38:46, 41:73] = 0
    at = [(38, 3), (38, 41)] + [(2 * int(rng.integers(0, 15)), 1 + 2 * int(rng.integers(0, 25))) for _ in range(IVAR_N - 2)]
    at = at[2:12] + at[:2] + at[12:]
    offs = np.array([y * IVAR_STRIDE + x for y, x in at], np.int32)
    other = plane.copy()
    other[1::2] = rng.integers(0, 256, other[1::2].shape)
    return dict(plane=frozen(plane), other=frozen(other), offs=frozen(offs), at=at)


def ivar_run(ref, plane, offs):
    out = np.zeros((2, 4 * len(offs)), np.uint64)
    f = as_proto(IVAR, ref.svt_compute_interm_var_four8x8_c)
    for i, o in enumerate(offs):
        f(vp(plane, int(o)), IVAR_STRIDE, vp(out[0], 32 * i), vp(out[1], 32 * i))
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------ svt_hip_upsampled_pred_batch_dev
UPS_PITCH = 144   # the md_subpel hook's staged window (integration/svt_hip_md_bridge.c): block + 8 taps + the one-sample spread of the candidates
# (w, h, bank, centre (row, col) in eighth-samples, step, content)
UPS_GROUPS = ((8, 8, 0, (16, 20), 4, "noise"), (16, 16, 3, (9, 10), 1, "checker"), (64, 64, 4, (13, 22), 2, "binary"), (128, 128, 1, (22, 13), 1, "noise"),
              (4, 16, 2, (5, 7), 2, "checker"), (16, 4, 5, (7, 5), 4, "binary"), (64, 16, 0, (10, 3), 1, "checker"), (128, 64, 3, (4, 6), 2, "binary"))


def _content(rng, shape, kind):
    if kind == "noise":
        return rng.integers(0, 256, shape).astype(np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        return (((yy + xx) & 1) * 255).astype(np.uint8)
    return (rng.integers(0, 2, shape) * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def ups_lists():
    """[(name, plane, stride, jobs, dst bytes)]: the eight hook-shaped groups (the eight neighbours of a centre at the round's step, one window of pitch 144,
    ref_off by the hook's formula, dst_off packed by w * h), then 40 mixed jobs on a plane of stride 211 with 3 bytes between their outputs"""
    rng = np.random.default_rng(4104)
    lists = []
    for w, h, bank, (cr, cc), step, kind in UPS_GROUPS:
        window = _content(rng, (128 + 9, UPS_PITCH), kind)
        jobs = (pkg.UpsampledBlk * 8)()
        r0, c0, n = (cr - step) >> 3, (cc - step) >> 3, 0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx or dy:
                    row, col = cr + dy * step, cc + dx * step
                    j = jobs[n]
                    j.ref_off = (((row >> 3) - r0) + 3) * UPS_PITCH + ((col >> 3) - c0) + 3
                    j.dst_off = n * w * h
                    j.w, j.h, j.subpel_x_q3, j.subpel_y_q3, j.bank = w, h, col & 7, row & 7, bank
                    n += 1
        lists.append(("%dx%d" % (w, h), frozen(window), UPS_PITCH, jobs, 8 * w * h))
    plane = np.concatenate([_content(rng, (230, 70), "noise"), _content(rng, (230, 70), "checker"), _content(rng, (230, 71), "binary")], axis=1)
    sizes = [(128, 128), (128, 4), (4, 128), (64, 32)] + [(1 << int(rng.integers(2, 6)), 1 << int(rng.integers(2, 6))) for _ in range(36)]
    jobs = (pkg.UpsampledBlk * 40)()
    off = 5
    for j, (w, h) in zip(jobs, sizes):
        y, x = int(rng.integers(3, 230 - h - 4)), int(rng.integers(3, 211 - w - 4))
        j.ref_off, j.dst_off = y * 211 + x, off
        j.w, j.h, j.subpel_x_q3, j.subpel_y_q3, j.bank = w, h, int(rng.integers(0, 8)), int(rng.integers(0, 8)), int(rng.integers(0, 6))
        if off == 5:
            j.subpel_x_q3 = j.subpel_y_q3 = 0   # the 128 x 128 job is a plain copy
        off += w * h + 3
    lists.append(("mixed", frozen(plane), 211, jobs, off))
    return lists


def ups_run(fn, plane, stride, jobs, nbytes):
    """fn(plane pointer, stride, dst pointer, job) per job into a pre-filled buffer of nbytes + GUARD"""
    dst = np.full(nbytes + GUARD, FILL8, np.uint8)
    for j in jobs:
        fn(vp(plane, j.ref_off), stride, vp(dst, j.dst_off), j)
    return dst


def ups_by_oracle(orc):
    return lambda p, stride, d, j: orc.orc_upsampled_pred(p, stride, d, j.w, j.h, j.subpel_x_q3, j.subpel_y_q3, j.bank)


def ups_by_reference(ref):
    """svt_aom_upsampled_pred_c names its three kernel families by subpel_search (1: bank 3, 2: bank 4, 3: bank 0)"""
    f = as_proto(UPS, ref.svt_aom_upsampled_pred_c)
    return lambda p, stride, d, j: f(None, None, 0, 0, None, d, j.w, j.h, j.subpel_x_q3, j.subpel_y_q3, p, stride, {3: 1, 4: 2, 0: 3}[j.bank])


def ups_numpy(banks, plane, stride, j, clip_between=True):
    """the two passes in numpy; clip_between=False leaves out the 8-bit clip between them (wrong on purpose: the lists must tell the two apart)"""
    y0, x0 = divmod(j.ref_off, stride)
    kx, ky = banks[j.bank][(j.subpel_x_q3 << 1) & 15].astype(np.int64), banks[j.bank][(j.subpel_y_q3 << 1) & 15].astype(np.int64)
    rows = slice(y0 - 3, y0 + j.h + 4) if j.subpel_y_q3 else slice(y0, y0 + j.h)
    a = plane[rows].astype(np.int64)
    if j.subpel_x_q3:
        mid = (sum(a[:, x0 - 3 + k:x0 - 3 + k + j.w] * kx[k] for k in range(8)) + 64) >> 7
        if clip_between or not j.subpel_y_q3:
            mid = np.clip(mid, 0, 255)
    else:
        mid = a[:, x0:x0 + j.w]
    if j.subpel_y_q3:
        mid = np.clip((sum(mid[k:k + j.h] * ky[k] for k in range(8)) + 64) >> 7, 0, 255)
    return mid.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ svt_hip_cdef_filter_block_batch_dev
CDEF_VERY_LARGE = 16384
CDEF_N, CDEF_DST_STRIDE, CDEF_DST_ROWS = 100, 93, 92   # a 10 x 10 grid of 9 x 9 cells in one destination whose stride is no multiple of 8
CDEF_RUNS = ((144, 0, True), (144, 0, False), (144, 2, False), (200, 0, True), (200, 2, False))   # (in_stride, coeff_shift, 8-bit destination)


def cdef_strengths(cs):
    """(pri, sec, pri_damping, sec_damping) as the reference passes them: neither, both (two pairs), secondary only, primary only"""
    return ((0, 0, 3, 3), (4 << cs, 2 << cs, 6 + cs, 5 + cs), (15 << cs, 4 << cs, 5 + cs, 5 + cs), (0, 1 << cs, 4 + cs, 3 + cs), (7 << cs, 0, 3 + cs, 3 + cs))


@functools.lru_cache(maxsize=None)
def cdef_case(stride, cs):
    """100 jobs over one staging image: CDEF_VERY_LARGE in its 6 left columns and 5 top rows, the first jobs against that corner.  `plain` is the same
    image without the marker (its samples replaced by ordinary ones): where the two expectations differ, taps reached marked samples."""
    rng = np.random.default_rng(4105 + stride + cs)
    img = np.clip(rng.normal(100 << cs, 30 << cs, (66, stride)), 0, (256 << cs) - 1).astype(np.uint16)
    plain = img.copy()
    img[:, :6] = CDEF_VERY_LARGE
    img[:5, :] = CDEF_VERY_LARGE
    jobs = (pkg.CdefBlk * CDEF_N)()
    order = rng.permutation(CDEF_N)   # destination cells in another order than the jobs
    st = cdef_strengths(cs)
    for i, j in enumerate(jobs):
        y, x = ((5, 6), (5, 40), (30, 6), (6, 7))[i] if i < 4 else (int(rng.integers(5, 66 - 11)), int(rng.integers(6, stride - 11)))
        cell = int(order[i])
        j.in_off, j.dst_off = y * stride + x, ((cell // 10) * 9 + 1) * CDEF_DST_STRIDE + (cell % 10) * 9 + 1
        j.pri_strength, j.sec_strength, j.pri_damping, j.sec_damping = st[(i + i // 5) % 5]
        j.dir, j.bw_log2, j.bh_log2, j.coeff_shift = (i // 4) % 8, 2 + (i & 1), 2 + ((i >> 1) & 1), cs
    return dict(img=frozen(img), plain=frozen(plain), jobs=jobs)


def cdef_run(fn, img, stride, jobs, dst8):
    """fn(dst8 pointer or None, dst16 pointer or None, image pointer, job) per job into the shared pre-filled destination"""
    dst = np.full((CDEF_DST_ROWS, CDEF_DST_STRIDE), FILL8 if dst8 else FILL16, np.uint8 if dst8 else np.uint16)
    for j in jobs:
        d = vp(dst, j.dst_off * dst.itemsize)
        fn(d if dst8 else None, None if dst8 else d, vp(img, 2 * j.in_off), j)
    return dst


def cdef_by_oracle(orc, stride):
    return lambda d8, d16, p, j: orc.orc_cdef_filter_block(d8, d16, CDEF_DST_STRIDE, p, stride, j.pri_strength, j.sec_strength, j.dir, j.pri_damping, j.sec_damping,
                                                           1 << j.bw_log2, 1 << j.bh_log2, j.coeff_shift)


def cdef_by_reference(ref):
    """svt_cdef_filter_block_c reads its input at CDEF_BSTRIDE = 144 only; bsize: BLOCK_4X4, 4X8, 8X4, 8X8 = 0 .. 3"""
    f = as_proto(CFB, ref.svt_cdef_filter_block_c)
    return lambda d8, d16, p, j: f(d8, d16, CDEF_DST_STRIDE, p, j.pri_strength, j.sec_strength, j.dir, j.pri_damping, j.sec_damping,
                                   2 * (j.bw_log2 - 2) + (j.bh_log2 - 2), j.coeff_shift)


# ------------------------------------------------------------------------------------------------ svt_hip_cdef_search_one_dual_dev
DUAL_SETS = ((1, (0, 64)), (37, (0, 64)), (300, (0, 16)), (90, (2, 40)))   # (sb_count, [start_gi, end_gi)) of test_rtcd_gpu.py


@functools.lru_cache(maxsize=None)
def dual_tables():
    rng = np.random.default_rng(4106)
    out = []
    for sb_count, _ in DUAL_SETS:
        m0 = rng.integers(1000, 1 << 22, (sb_count, 64)).astype(np.uint64)
        m1 = rng.integers(1000, 1 << 21, (sb_count, 64)).astype(np.uint64)
        m0[:, 7] = m0[:, 3]
        m1[:, 9] = m1[:, 5]   # equal totals: the first pair in raster order wins
        out.append(frozen(m0, m1))
    return out


def dual_run(ref):
    """per set: [(lev0[8], lev1[8], total)] after each of the steps nb_strengths = 0 .. 7, by svt_search_one_dual_c; unwritten entries keep -7"""
    f = as_proto(ONEDUAL, ref.svt_search_one_dual_c)
    out = []
    for (sb_count, (start, end)), (m0, m1) in zip(DUAL_SETS, dual_tables()):
        ptrs = (C.c_void_p * 2)(m0.ctypes.data, m1.ctypes.data)
        l0, l1, steps = np.full(8, -7, np.int32), np.full(8, -7, np.int32), []
        for nb in range(8):
            tot = f(vp(l0), vp(l1), nb, C.cast(ptrs, C.c_void_p), sb_count, start, end)
            steps.append((l0.copy(), l1.copy(), tot))
        out.append(steps)
    return out


# ------------------------------------------------------------------------------------------------ single-unit forms
# Every array is larger than the unit, the unit starts inside it, and no two strides of a call are equal.
BIG_SIZES = ((136, 20), (12, 132))   # one size above 128 in each direction (the per-call table delegates these)


@functools.lru_cache(maxsize=None)
def conv8_table():
    """a 256-byte aligned table of 16 kernels that sum to 128, as the reference derives it from its filter pointer"""
    rng = np.random.default_rng(4107)
    raw = np.zeros(256 + 256, np.uint8)
    off = (-raw.ctypes.data) % 256
    table = raw[off:off + 256].view(np.int16).reshape(16, 8)
    for p in range(16):
        t = rng.integers(-20, 40, 8)
        t[3] += 128 - t.sum()
        table[p] = t
    return table, raw


CONV8_SS, CONV8_AT = 337, (5, 7)
CONV8_BIG = {(0, 16): (200, 150), (1, 16): (200, 150), (0, 24): (200, 150), (1, 24): (200, 150), (0, 64): (70, 150), (1, 64): (200, 70)}
CONV8_SMALL = ((7, 5), (33, 17), (64, 8), (1, 1), (20, 3), (3, 20))


@functools.lru_cache(maxsize=None)
def conv8_case():
    """both axes x steps 16 / 24 / 64 x every start phase; phase 5 of each takes the large size"""
    rng = np.random.default_rng(4108)
    src = extreme_plane(rng, (330, CONV8_SS), 255, np.uint8)
    cases = []
    for vert in (0, 1):
        for step in (16, 24, 64):
            for q0 in range(16):
                w, h = CONV8_BIG[(vert, step)] if q0 == 5 else CONV8_SMALL[(q0 + vert) % len(CONV8_SMALL)]
                reach = (((h if vert else w) - 1) * step + q0) // 16 + 4
                assert CONV8_AT[0] + (reach if vert else h) < 330 and CONV8_AT[1] + (w if vert else reach) < CONV8_SS
                cases.append((vert, step, q0, w, h))
    return frozen(src), cases


def conv8_expected(ref, src, case):
    vert, step, q0, w, h = case
    table, _ = conv8_table()
    ds = w + 5
    dst = np.full((h + 2, ds), FILL8, np.uint8)
    f = as_proto(CONV8, ref.svt_aom_convolve8_vert_c if vert else ref.svt_aom_convolve8_horiz_c)
    k = vp(table, 16 * q0)
    f(vp(src, CONV8_AT[0] * CONV8_SS + CONV8_AT[1]), CONV8_SS, vp(dst, ds + 2), ds, k, step, k, step, w, h)
    return dst


WIENER_FORMATS = ((1, 8, 3, 11), (2, 8, 3, 11), (2, 10, 3, 11), (2, 12, 5, 9))   # (pix_bytes, bd, round_0, round_1)
WIENER_SIZES = ((136, 70), (7, 5))
WIENER_SS, WIENER_AT = 163, (4, 5)
# the horizontal taps leave [0, WIENER_CLAMP_LIMIT) on 0 / max stripes in both directions (the ABI takes any taps; the encoder's own are tamer)
WIENER_TAPS = np.array([[-40, 50, -40, 30, -40, 50, -40, 0], [3, -7, 15, -22, 15, -7, 3, 0]], np.int16)


@functools.lru_cache(maxsize=None)
def wiener_plane(pix_bytes, bd):
    rng = np.random.default_rng(4109 + bd + pix_bytes)
    return frozen(extreme_plane(rng, (90, WIENER_SS), (1 << bd) - 1, sample_dtype(pix_bytes)))


def wiener_expected(orc, pix_bytes, bd, r0, r1, w, h):
    src = wiener_plane(pix_bytes, bd)
    ds = w + 9
    dst = np.full((h + 2, ds), FILL8 if pix_bytes == 1 else FILL16, src.dtype)
    orc.orc_wiener_convolve_add_src_rounds(vp(src, (WIENER_AT[0] * WIENER_SS + WIENER_AT[1]) * pix_bytes), WIENER_SS, vp(dst, (ds + 3) * pix_bytes), ds, pix_bytes,
                                           vp(WIENER_TAPS, 0), vp(WIENER_TAPS, 16), w, h, bd, r0, r1)
    return dst


def wiener_by_reference(ref, pix_bytes, bd, r0, r1, w, h):
    """the reference's function keeps its intermediate in a 128-wide buffer: units up to 128 x 128 only; its taps come from a 256-byte aligned table"""
    src = wiener_plane(pix_bytes, bd)
    raw = np.zeros(512, np.uint8)
    off = (-raw.ctypes.data) % 256
    taps = raw[off:off + 256].view(np.int16).reshape(16, 8)
    taps[2], taps[5] = WIENER_TAPS
    ds = w + 9
    dst = np.full((h + 2, ds), FILL8 if pix_bytes == 1 else FILL16, src.dtype)
    cp = ConvParams(0, 0, None, 0, r0, r1, 0, 0, 0, 0, 0, 0)
    s, d = src.ctypes.data + (WIENER_AT[0] * WIENER_SS + WIENER_AT[1]) * pix_bytes, dst.ctypes.data + (ds + 3) * pix_bytes
    if pix_bytes == 1:
        as_proto(WIENER, ref.svt_av1_wiener_convolve_add_src_c)(s, WIENER_SS, d, ds, vp(taps, 32), vp(taps, 80), w, h, C.byref(cp))
    else:   # CONVERT_TO_BYTEPTR
        as_proto(WIENERH, ref.svt_av1_highbd_wiener_convolve_add_src_c)(s >> 1, WIENER_SS, d >> 1, ds, vp(taps, 32), vp(taps, 80), w, h, C.byref(cp), bd)
    return dst


def wiener_unclamped_range(pix_bytes, bd, r0, w, h):
    """(min, max, limit) of the horizontal pass before its clamp, over the rows the vertical pass reads"""
    src = wiener_plane(pix_bytes, bd).astype(np.int64)
    y0, x0 = WIENER_AT
    a = src[y0 - 3:y0 + h + 4]
    s = sum(a[:, x0 - 3 + k:x0 - 3 + k + w] * int(WIENER_TAPS[0, k]) for k in range(8)) + (a[:, x0:x0 + w] << 7) + (1 << (bd + 6))
    v = (s + (1 << (r0 - 1))) >> r0
    return int(v.min()), int(v.max()), (1 << (bd + 8 - r0)) - 1


JNT_FORMATS = ((1, 8), (2, 10), (2, 12))
JNT_SS, JNT_AT = 181, (6, 8)
JNT_WEIGHTS = ((0, 0, 0), (1, 9, 7))   # (use_jnt_comp_avg, fwd_offset, bck_offset)


@functools.lru_cache(maxsize=None)
def jnt_planes(pix_bytes, bd):
    rng = np.random.default_rng(4110 + bd)
    a = extreme_plane(rng, (170, JNT_SS), (1 << bd) - 1, sample_dtype(pix_bytes))
    b = np.clip(a.astype(np.int32) + rng.integers(-30 << (bd - 8), (30 << (bd - 8)) + 1, a.shape), 0, (1 << bd) - 1).astype(a.dtype)
    return frozen(a, b)


@functools.lru_cache(maxsize=None)
def jnt_cases():
    """(pix_bytes, bd, variant, w, h, (bank, phase) x, (bank, phase) y, weights)"""
    rng = np.random.default_rng(4111)
    return [(pb, bd, variant, w, h, (int(rng.integers(0, 6)), int(rng.integers(1, 16))), (int(rng.integers(0, 6)), int(rng.integers(1, 16))), wt)
            for pb, bd in JNT_FORMATS for variant in range(4) for w, h in BIG_SIZES for wt in JNT_WEIGHTS]


def jnt_layout(w, h):
    """compound buffer (h + 2, w + 6) used from (1, 2), pixels (h + 2, w + 3) used from (1, 1): convbuf_stride != dst_stride != w"""
    return (h + 2, w + 6), (w + 6) + 2, (h + 2, w + 3), (w + 3) + 1


def jnt_expected(ref, banks, case):
    """-> (compound buffer after the do_average = 0 call, pixels after the do_average = 1 call); each call leaves the other buffer as it was"""
    pb, bd, variant, w, h, (bx, sx), (by, sy), (jnt, fwd, bck) = case
    name = ("2d", "x", "y", "2d_copy")[variant]
    f = as_proto(CONV, getattr(ref, f"svt_av1_jnt_convolve_{name}_c")) if pb == 1 else as_proto(CONVH, getattr(ref, f"svt_av1_highbd_jnt_convolve_{name}_c"))
    fx, fy = FilterParams(banks[bx].ctypes.data, 8, 16, bx % 4), FilterParams(banks[by].ctypes.data, 8, 16, by % 4)
    cshape, coff, dshape, doff = jnt_layout(w, h)
    cb, out = np.full(cshape, 4321, np.uint16), np.full(dshape, FILL8 if pb == 1 else FILL16, sample_dtype(pb))
    for do_avg, img in enumerate(jnt_planes(pb, bd)):
        cp = ConvParams(0, do_avg, cb.ctypes.data + 2 * coff, cshape[1], 5 if bd == 12 else 3, 7, 0, 1, jnt, fwd, bck, jnt)
        f(img.ctypes.data + (JNT_AT[0] * JNT_SS + JNT_AT[1]) * pb, JNT_SS, out.ctypes.data + doff * pb, dshape[1], w, h, C.byref(fx), C.byref(fy), sx, sy,
          C.byref(cp), *((bd,) if pb == 2 else ()))
        if do_avg == 0:
            first = cb.copy()
            assert (out == out.flat[0]).all()
    assert np.array_equal(cb, first)
    return first, out


def jnt_taps(banks, case):
    (bx, sx), (by, sy) = case[5], case[6]
    return np.concatenate([banks[bx][sx], banks[by][sy]]).astype(np.int16)


MASK_KINDS = (("pixels", 1, 8), ("pixels16", 2, 10), ("pixels16", 2, 12), ("d16", 2, 8), ("d16", 2, 10), ("d16", 2, 12))


def d16_offset(bd):
    r0 = 5 if bd == 12 else 3
    return (1 << (bd + 14 - r0 - 7)) + (1 << (bd + 14 - r0 - 8))


@functools.lru_cache(maxsize=None)
def mask_inputs(kind, bd, w, h):
    """two sources in arrays (h + 2, w + 3) and (h + 2, w + 7), used from (1, 2) and (1, 3)"""
    rng = np.random.default_rng(4112 + bd + w)
    dt = np.uint8 if kind == "pixels" else np.uint16
    if kind == "d16":   # the offset-carrying intermediates of the jnt convolves
        a = d16_offset(bd) + rng.integers(0, 1 << (bd + 3), (h + 2, w + 7))   # half the range above the offset: inside 16 bits at every depth
        b = d16_offset(bd) + rng.integers(0, 1 << (bd + 3), a.shape)
    else:
        a = rng.integers(0, 1 << bd, (h + 2, w + 7))
        b = np.clip(a + rng.integers(-(120 << (bd - 8)), (120 << (bd - 8)) + 1, a.shape), 0, (1 << bd) - 1)
    return frozen(np.ascontiguousarray(a[:, 1:w + 4]).astype(dt), b.astype(dt))   # a's (1, 2) and b's (1, 3) are the same sample


def mask_args(kind, bd):
    """(round, shift) of svt_hip_diffwtd_mask_dev"""
    return (14 - (5 if bd == 12 else 3) - 7 + bd - 8, 0) if kind == "d16" else (0, bd - 8 if kind == "pixels16" else 0)


def mask_expected(ref, kind, bd, w, h, inverse):
    a, b = mask_inputs(kind, bd, w, h)
    mask = np.full(w * h + GUARD, FILL8, np.uint8)
    pa, pb = vp(a, (a.shape[1] + 2) * a.itemsize), vp(b, (b.shape[1] + 3) * b.itemsize)
    if kind == "pixels":
        as_proto(DWM, ref.svt_av1_build_compound_diffwtd_mask_c)(vp(mask), inverse, pa, a.shape[1], pb, b.shape[1], h, w)
    elif kind == "pixels16":
        as_proto(DWMH, ref.svt_av1_build_compound_diffwtd_mask_highbd_c)(vp(mask), inverse, pa, a.shape[1], pb, b.shape[1], h, w, bd)
    else:
        cp = ConvParams(0, 0, None, 0, 5 if bd == 12 else 3, 7, 0, 1, 0, 0, 0, 0)
        as_proto(DWM16, ref.svt_av1_build_compound_diffwtd_mask_d16_c)(vp(mask), inverse, pa, a.shape[1], pb, b.shape[1], h, w, C.byref(cp), bd)
    return mask


@functools.lru_cache(maxsize=None)
def blend_mask(w, h, subw, subh):
    """mask array ((h << subh) + 1, (w << subw) + 6) used from column 1: mask_stride = mask width + 6"""
    rng = np.random.default_rng(4113 + w + 2 * subw + subh)
    return frozen(rng.integers(0, 65, ((h << subh) + 1, (w << subw) + 6)).astype(np.uint8))


def blend_expected(ref, pix_bytes, bd, w, h, subw, subh):
    """pixels (h + 2, w + 4) written from (1, 1); the compound buffers are the d16 mask inputs"""
    c0, c1 = mask_inputs("d16", bd, w, h)
    mk = blend_mask(w, h, subw, subh)
    dst = np.full((h + 2, w + 4), FILL8 if pix_bytes == 1 else FILL16, sample_dtype(pix_bytes))
    cp = ConvParams(0, 0, None, 0, 5 if bd == 12 else 3, 7, 0, 1, 0, 0, 0, 0)
    args = (vp(dst, (w + 4 + 1) * pix_bytes), w + 4, vp(c0, 2 * (c0.shape[1] + 2)), c0.shape[1], vp(c1, 2 * (c1.shape[1] + 3)), c1.shape[1], vp(mk, 1), mk.shape[1], w, h, subw, subh,
            C.byref(cp))
    if pix_bytes == 1:
        as_proto(BLD16, ref.svt_aom_lowbd_blend_a64_d16_mask_c)(*args)
    else:
        as_proto(BLD16H, ref.svt_aom_highbd_blend_a64_d16_mask_c)(*args, bd)
    return dst


SGR_SIZES = ((300, 280), (70, 50))   # 300 x 280: the row loop (256 workgroups) and the column loop (256 lanes) both go round again
SGR_RADII = ((2, 1), (0, 1), (2, 0))
SGR_XQ = np.array([-37, 61], np.int32)


def sgr_ep(orc, radii):
    """a parameter set of the oracle's table with these radii"""
    prm = np.ctypeslib.as_array((C.c_int32 * 4 * 16).in_dll(orc, "orc_sgr_params"))
    return next(ep for ep in range(16) if (int(prm[ep][0]), int(prm[ep][1])) == radii)


@functools.lru_cache(maxsize=None)
def sgr_inputs(pix_bytes, w, h):
    """src (h + 2, w + 6), dat (h + 2, w + 9), flt0 (h + 1, w + 3), flt1 (h + 1, w + 12): four different strides, each used from (1, 2)"""
    bd = 8 if pix_bytes == 1 else 10
    rng = np.random.default_rng(4114 + w + pix_bytes)
    dt = sample_dtype(pix_bytes)
    base = np.clip(rng.normal(100 << (bd - 8), 30 << (bd - 8), (h + 2, w + 12)), 0, (1 << bd) - 1).astype(np.int32)
    near = np.clip(base + rng.integers(-8, 9, base.shape) * (1 << (bd - 8)), 0, (1 << bd) - 1)
    src, dat = np.ascontiguousarray(base[:, :w + 6]).astype(dt), np.ascontiguousarray(near[:, :w + 9]).astype(dt)
    f0 = np.ascontiguousarray((((near + base) << 3) + rng.integers(-200, 201, near.shape))[:h + 1, :w + 3]).astype(np.int32)
    f1 = ((base << 4) + rng.integers(-120, 121, base.shape))[:h + 1].astype(np.int32)
    return frozen(src, dat, f0, f1)


def sgr_pointers(arrays, at=vp):
    """(pointer, stride) of each of the four arrays at its sample (1, 2); `at` maps (array, byte offset) to a pointer"""
    return [(at(a, (a.shape[1] + 2) * a.itemsize), a.shape[1]) for a in arrays]


def sgr_expected(orc, pix_bytes, w, h, radii):
    """-> (sums[5], xq[2] of the solve, squared error of the projection with SGR_XQ); radii (0, 0): the plain squared error alone"""
    arrays = sgr_inputs(pix_bytes, w, h)
    (s, ss), (d, ds), (f0, f0s), (f1, f1s) = sgr_pointers(arrays)
    if radii == (0, 0):
        a, b = (x[1:h + 1, 2:w + 2].astype(np.int64) for x in arrays[:2])
        return None, None, int(((b - a) ** 2).sum())
    ep = sgr_ep(orc, radii)
    sums, xq = np.zeros(5, np.int64), np.zeros(2, np.int32)
    orc.orc_sgr_proj_sums(s, ss, d, ds, pix_bytes, w, h, f0, f0s, f1, f1s, ep, vp(sums))
    orc.orc_sgr_solve(vp(sums), w * h, ep, vp(xq))
    orc.orc_sgr_proj_error.restype = C.c_int64
    return sums, xq, orc.orc_sgr_proj_error(s, ss, d, ds, pix_bytes, w, h, f0, f0s, f1, f1s, vp(SGR_XQ), ep)


def sgr_by_reference(ref, pix_bytes, w, h, radii):
    """-> (xq of svt_get_proj_subspace_c, svt_av1_{lowbd,highbd}_pixel_proj_error_c with SGR_XQ); CONVERT_TO_BYTEPTR for 16-bit samples"""
    arrays = sgr_inputs(pix_bytes, w, h)
    hbd = int(pix_bytes == 2)
    (s, ss), (d, ds), (f0, f0s), (f1, f1s) = sgr_pointers(arrays, lambda a, off: (a.ctypes.data + off) >> 1 if hbd and a.itemsize == 2 else C.c_void_p(a.ctypes.data + off))
    prm = SgrParams((C.c_int32 * 2)(*radii), (C.c_int32 * 2)(140, 3236))
    xq = np.zeros(2, np.int32)
    if radii != (0, 0):
        as_proto(PROJSUB, ref.svt_get_proj_subspace_c)(s, w, h, ss, d, ds, hbd, f0, f0s, f1, f1s, vp(xq), C.byref(prm))
    f = ref.svt_av1_highbd_pixel_proj_error_c if hbd else ref.svt_av1_lowbd_pixel_proj_error_c
    return xq, as_proto(PROJERR, f)(s, w, h, ss, d, ds, f0, f0s, f1, f1s, vp(SGR_XQ), C.byref(prm))
