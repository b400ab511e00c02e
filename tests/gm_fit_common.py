"""Shared by the tests of the global-motion model fit: the named correspondence lists, the reference side (the three fit functions of libsvtav1_ref.so reached
through svt_av1_get_ransac_type, svt_av1_convert_model_to_params, gm_get_params_cost, svt_av1_is_enough_erroradvantage, through ctypes on numpy buffers) and the
composition of the reference's functions in the order of compute_global_motion.  Reference results are computed once per process and never changed.

Everything is compared by bit pattern: doubles travel as their 8 bytes (`bits`), so -0.0 and +0.0 differ and no tolerance exists anywhere."""
import ctypes as C
import functools

import numpy as np

import gm_common as g
import gm_front_common as f

VP = C.c_void_p
TRANSLATION, ROTZOOM, AFFINE = 1, 2, 3
TYPES = (TRANSLATION, ROTZOOM, AFFINE)
TYPE_NAMES = {1: "translation", 2: "rotzoom", 3: "affine"}
MAX_CORNERS = 4096
IDENTITY_PARAMS = (0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
W, H = 352, 288


class MotionModel(C.Structure):
    """MotionModel (Encoder/Codec/global_motion.h:51-55)."""
    _fields_ = [("params", C.c_double * 8), ("inliers", C.POINTER(C.c_int)), ("num_inliers", C.c_int)]


RANSAC = C.CFUNCTYPE(C.c_int, VP, C.c_int, C.POINTER(C.c_int), C.POINTER(MotionModel), C.c_int)
_prepared = set()


def prepare(L):
    if id(L) in _prepared:
        return L
    g.prepare(L); f.prepare(L)
    i = C.c_int
    L.svt_av1_get_ransac_type.argtypes = [i]
    L.svt_av1_get_ransac_type.restype = RANSAC
    L.svt_av1_convert_model_to_params.argtypes = [C.POINTER(C.c_double), C.POINTER(g.WM)]
    L.svt_av1_convert_model_to_params.restype = None
    L.svt_av1_compute_global_motion.argtypes = [i, VP, i, i, i, VP, i, VP, i, i, i, C.POINTER(i), C.POINTER(MotionModel), i]
    L.svt_av1_compute_global_motion.restype = i
    L.gm_get_params_cost.argtypes = [C.POINTER(g.WM), C.POINTER(g.WM), i]
    L.gm_get_params_cost.restype = i
    L.svt_av1_is_enough_erroradvantage.argtypes = [C.c_double, i, i]
    L.svt_av1_is_enough_erroradvantage.restype = i
    _prepared.add(id(L))
    return L


def bits(values):
    """the bit patterns of doubles, as a tuple of ints"""
    return tuple(int(v) for v in np.asarray(values, np.float64).view(np.uint64))


# ------------------------------------------------------------------------------------------------ the lists
RZ = (1.02 * np.cos(0.03), 1.02 * np.sin(0.03), -1.02 * np.sin(0.03), 1.02 * np.cos(0.03), 3.5, -2.25)   # a, b, c, d, tx, ty: rx = a x + b y + tx, ry = c x + d y + ty
AF = (1.015, 0.02, -0.012, 0.99, -4.2, 2.7)
TR = (1.0, 0.0, 0.0, 1.0, 5.25, -3.5)


def _mapped(seed, n, model, noise, outliers):
    """n points of a 352x288 picture mapped by `model`: rounded to integers, Gaussian noise, a share of random outliers"""
    rng = np.random.default_rng(seed)
    x = rng.integers(8, W - 8, n).astype(np.float64)
    y = rng.integers(8, H - 8, n).astype(np.float64)
    a, b, c, d, tx, ty = model
    rx = a * x + b * y + tx + noise * rng.standard_normal(n)
    ry = c * x + d * y + ty + noise * rng.standard_normal(n)
    out = rng.random(n) < outliers
    rx = np.where(out, rng.integers(8, W - 8, n), rx)
    ry = np.where(out, rng.integers(8, H - 8, n), ry)
    return np.stack([x, y, np.floor(rx + 0.5), np.floor(ry + 0.5)], 1).astype(np.int32)


def _list(name, corr, count=None, capacity=None):
    corr = np.ascontiguousarray(corr, np.int32).reshape(-1, 4)
    capacity = capacity or max(len(corr), 1)
    buf = np.full((capacity, 4), -12345, np.int32)   # rows past the list are never to be read
    buf[:len(corr)] = corr
    buf.setflags(write=False)
    count = len(corr) if count is None else count
    return dict(name=name, corr=buf, count=count, capacity=capacity, n=max(0, min(count, capacity)))


@functools.lru_cache(maxsize=None)
def lists():
    """name -> dict(corr int32 [capacity][4], count = what the device-side counter holds, capacity = max_points, n = the count after the clamp)"""
    out = []
    for k, n in enumerate((14, 15, 16, 40, 300, 2500, 4096)):
        out.append(_list(f"rz_{n}", _mapped(SEEDS[f"rz_{n}"], n, RZ, 0.3 + 0.1 * (k & 1), 0.2 + 0.05 * (k % 3))))
        out.append(_list(f"af_{n}", _mapped(SEEDS[f"af_{n}"], n, AF, 0.4 - 0.1 * (k & 1), 0.3 - 0.05 * (k % 3))))
    out.append(_list("tr_300", _mapped(SEEDS["tr_300"], 300, TR, 0.35, 0.25)))
    rng = np.random.default_rng(SEEDS["identity_100"])
    p = np.stack([rng.integers(8, W - 8, 100), rng.integers(8, H - 8, 100)], 1)
    out.append(_list("identity_100", np.concatenate([p, p], 1)))
    out.append(_list("outliers_300", _mapped(SEEDS["outliers_300"], 300, RZ, 0.35, 1.1)))
    # 100 collinear points 3 apart; the reference side moves by 2.5 a point, so that no translation has two of them as inliers
    t = np.arange(100)
    out.append(_list("collinear_100", np.stack([20 + 3 * t, 30 + 2 * t, 25 + 5 * t, 28 + 4 * t], 1)))
    out.append(_list("single_100", np.tile(np.array([[120, 77, 123, 75]]), (100, 1))))
    two = _mapped(SEEDS["two_rows"], 120, RZ, 0.3, 0.2)
    two[:, 1] = 140 + (np.arange(120) & 1)
    two[:, 2] = np.floor(RZ[0] * two[:, 0] + RZ[1] * two[:, 1] + RZ[4] + 0.5)
    two[:, 3] = np.floor(RZ[2] * two[:, 0] + RZ[3] * two[:, 1] + RZ[5] + 0.5)
    out.append(_list("two_rows", two))
    out.append(_list("empty", np.zeros((0, 4), np.int32), capacity=16))
    out.append(_list("count_over_capacity", _mapped(SEEDS["count_over_capacity"], 64, RZ, 0.3, 0.2), count=1000, capacity=64))
    out.append(_list("count_negative", _mapped(SEEDS["count_over_capacity"], 64, RZ, 0.3, 0.2), count=-5, capacity=64))
    out.append(_list("small_capacity", _mapped(SEEDS["small_capacity"], 150, AF, 0.35, 0.25), capacity=200))
    return {l["name"]: l for l in out}


# seeds chosen on the CPU so that the reference gives every list the behaviour its name promises (tests/test_gm_fit_ref_cpu.py holds them to it)
SEEDS = {"rz_14": 101, "rz_15": 102, "rz_16": 103, "rz_40": 104, "rz_300": 105, "rz_2500": 106, "rz_4096": 107,
         "af_14": 201, "af_15": 202, "af_16": 203, "af_40": 204, "af_300": 205, "af_2500": 206, "af_4096": 207,
         "tr_300": 301, "identity_100": 302, "outliers_300": 303, "two_rows": 304, "count_over_capacity": 305, "small_capacity": 306}

LIST_NAMES = ["rz_14", "af_14", "rz_15", "af_15", "rz_16", "af_16", "rz_40", "af_40", "rz_300", "af_300", "rz_2500", "af_2500", "rz_4096", "af_4096", "tr_300",
              "identity_100", "outliers_300", "collinear_100", "single_100", "two_rows", "empty", "count_over_capacity", "count_negative", "small_capacity"]
CASES = [(n, t) for n in LIST_NAMES for t in TYPES]


def case_id(case):
    return f"{case[0]}-{TYPE_NAMES[case[1]]}"


# ------------------------------------------------------------------------------------------------ the reference
def ref_convert(L, params):
    """svt_av1_convert_model_to_params -> (wmmat[8], wmtype)"""
    wm = g.WM()
    prepare(L).svt_av1_convert_model_to_params((C.c_double * 8)(*params), C.byref(wm))
    return [int(v) for v in wm.wmmat], int(wm.wmtype)


def ref_fit_points(L, corr, type_):
    """the reference's fit function of `type_` on corr [n][4], with what compute_global_motion does around it (identity parameters first; the MIN_INLIER_PROB
    rule and the conversion afterwards) -> dict(ret, npoints, num_inliers, num_inliers_kept, params (bit patterns), inliers, wmmat, wmtype)"""
    corr = np.ascontiguousarray(corr, np.int32).reshape(-1, 4)
    n = len(corr)
    mm = MotionModel()
    for k, v in enumerate(IDENTITY_PARAMS):
        mm.params[k] = v
    inl = np.full(2 * MAX_CORNERS, -1, np.int32)
    mm.inliers = inl.ctypes.data_as(C.POINTER(C.c_int))
    mm.num_inliers = 0
    num = C.c_int(-1)
    pts = np.concatenate([corr, np.zeros((1, 4), np.int32)])   # never an empty buffer
    ret = prepare(L).svt_av1_get_ransac_type(type_)(pts.ctypes.data_as(VP), n, C.byref(num), C.byref(mm), 1)
    params = [float(v) for v in mm.params]
    kept = 0 if (num.value < 0.1 * n or n == 0) else num.value
    wmmat, wmtype = ref_convert(L, params)
    return dict(ret=int(ret), npoints=n, num_inliers=num.value, num_inliers_kept=kept, params=bits(params), params_f=params,
                inliers=[int(v) for v in inl[:num.value]] if num.value >= 3 else None, wmmat=wmmat, wmtype=wmtype)


_fits = {}


def ref_fit(L, name, type_):
    """the reference's result for a named list, computed once"""
    if (name, type_) not in _fits:
        l = lists()[name]
        _fits[(name, type_)] = ref_fit_points(L, l["corr"][:l["n"]], type_)
    return _fits[(name, type_)]


def fit_record(fit, inliers=None):
    """an SvtHipGmFit (ctypes) in the shape of ref_fit's result"""
    return dict(ret=fit.ret, npoints=fit.npoints, num_inliers=fit.num_inliers, num_inliers_kept=fit.num_inliers_kept, params=bits(list(fit.params)),
                inliers=[int(v) for v in inliers[:fit.num_inliers]] if inliers is not None and fit.num_inliers >= 3 else None, wmmat=list(fit.wmmat), wmtype=fit.wmtype)


def same_fit(got, want, with_inliers=True):
    keys = ["ret", "npoints", "num_inliers", "num_inliers_kept", "params", "wmmat", "wmtype"] + (["inliers"] if with_inliers else [])
    return [(k, got[k], want[k]) for k in keys if got[k] != want[k]]


def expected_job(want, ref_index, n_refinements):
    """the SvtHipGmJob the fit writes for the refinement: (ref, wmtype, wmmat, n_refinements, best_frame_error)"""
    skip = want["num_inliers_kept"] == 0 or want["wmtype"] == 0
    return (ref_index, -1 if skip else want["wmtype"], want["wmmat"], n_refinements, g.INT64_MAX)


# ------------------------------------------------------------------------------------------------ the decision, composed from the reference's functions
DEFAULT_WM = (0, 0, g.ONE, 0, 0, g.ONE, 0, 0)


def ref_params_cost(L, wmmat, wmtype, allow_hp):
    gm, ref = g.make_wm(wmmat, wmtype), g.make_wm(DEFAULT_WM, 0)
    return prepare(L).gm_get_params_cost(C.byref(gm), C.byref(ref), allow_hp)


def _round_signed(v, n):
    return -((-v + (1 << (n - 1))) >> n) if v < 0 else (v + (1 << (n - 1))) >> n


def ref_decide(L, records, ref_frame_error, rotzoom_model_only, allow_hp):
    """the model loop of compute_global_motion (EbGlobalMotionEstimation.c:303-399) over per-model records dict(num_inliers_kept, fit_wmtype, wmmat, wmtype,
    best_error), every arithmetic step by the reference's own function: svt_get_shear_params, gm_get_params_cost, svt_av1_is_enough_erroradvantage
    -> (wmmat[8], wmtype)"""
    L = prepare(L)
    gm, gm_type = list(DEFAULT_WM), 0
    for model in ((ROTZOOM,) if rotzoom_model_only else (ROTZOOM, AFFINE)):
        rec = records[model - 2]
        best = g.INT64_MAX
        if rec["num_inliers_kept"] != 0 and rec["fit_wmtype"] != 0:
            if rec["best_error"] < best:
                best, gm, gm_type = rec["best_error"], list(rec["wmmat"]), rec["wmtype"]
        wm = g.make_wm(gm, gm_type)
        if not L.svt_get_shear_params(C.byref(wm)):
            gm, gm_type = list(DEFAULT_WM), 0
        if gm_type == TRANSLATION:
            for k in range(2):
                gm[k] = (_round_signed(gm[k], 13) if allow_hp else _round_signed(gm[k], 14) * 2) * (1 << 13)
        if gm_type == 0:
            continue
        if ref_frame_error == 0:
            continue
        adv = C.c_double(best).value / C.c_double(ref_frame_error).value
        if not L.svt_av1_is_enough_erroradvantage(adv, ref_params_cost(L, gm, gm_type, allow_hp), 0):
            gm, gm_type = list(DEFAULT_WM), 0
        if gm_type != 0:
            break
    return gm, gm_type


def ref_estimate(L, src, rf, rotzoom_model_only, allow_hp, n_refinements=5, max_points=MAX_CORNERS):
    """compute_global_motion for one reference plane, composed of the reference's functions in its order: corners of the source, then per model type
    svt_av1_compute_global_motion (corners of the reference, correspondences, the fit, the MIN_INLIER_PROB rule), svt_av1_convert_model_to_params,
    svt_av1_refine_integerized_param, and the decision -> dict(wmmat, wmtype, records, ref_frame_error, num_correspondences)"""
    L = prepare(L)
    h, w = src.shape
    sp = f.ref_corners(L, src, max_points)
    ferr = g.ref_frame_error(L, rf[:h, :w], src)
    records, ncorr = [], 0
    for model in ((ROTZOOM,) if rotzoom_model_only else (ROTZOOM, AFFINE)):
        mm = MotionModel()
        for k, v in enumerate(IDENTITY_PARAMS):
            mm.params[k] = v
        inl = np.zeros(2 * MAX_CORNERS, np.int32)
        mm.inliers = inl.ctypes.data_as(C.POINTER(C.c_int))
        num = C.c_int(0)
        spc = np.ascontiguousarray(np.concatenate([sp, np.zeros((1, 2), np.int32)]))
        L.svt_av1_compute_global_motion(model, f._p(src), w, h, f._stride(src), f._p(spc), len(sp), f._p(rf), f._stride(rf), 8, 0, C.byref(num), C.byref(mm), 1)
        wmmat, wmtype = ref_convert(L, [float(v) for v in mm.params])
        rec = dict(num_inliers_kept=num.value, fit_wmtype=wmtype, wmmat=wmmat, wmtype=-1, best_error=-1)
        if num.value != 0 and wmtype != 0:
            rec["wmmat"], rec["wmtype"], rec["best_error"] = g.ref_refine(L, wmmat, wmtype, rf, src, n_refinements)
        records.append(rec)
    gm, gm_type = ref_decide(L, records, ferr, rotzoom_model_only, allow_hp)
    return dict(wmmat=gm, wmtype=gm_type, records=records, ref_frame_error=ferr)
