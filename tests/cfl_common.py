"""Shared by the CfL / filter-intra tests: the reference side (functions libsvtav1_ref.so exports, called through ctypes on numpy buffers), the seeded input
generators, and the helpers that lay jobs out in planes, run them on the device and build what the planes must hold afterwards.

CfL reference: svt_cfl_luma_subsampling_420_{lbd,hbd}_c -> svt_subtract_average_c -> svt_cfl_predict_{lbd,hbd}_c with pred == dst, the composition of cfl_prediction
(Encoder/Codec/EbProductCodingLoop.c:3085-3180); with dc_from_edges the prediction is the reference's DC predictor (intra_common.ref_predict, mode 0).
Filter-intra reference: svt_av1_filter_intra_predictor_c / highbd_filter_intra_predictor.

A job here is a dict that carries its own data -- luma area [2h][2w], the two chroma blocks the planes hold before the call [2][h][w], two edge records
[2][2][160] -- so that any subset, in any order and any plane layout, is checked against per-job reference results computed once."""
import ctypes as C

import numpy as np

import intra_common as ic

VP = C.c_void_p
EDGE_REC, EDGE_ORG = ic.EDGE_REC, ic.EDGE_ORG
SHAPES = [t for t, (w, h) in enumerate(ic.TX_WH) if w <= 32 and h <= 32]   # the 14 shapes of CFL_SUB_AVG_FN = the shapes filter-intra allows
AC_LINE = 32                                                              # CFL_BUF_LINE
AC_MARK = 0x5A5A
BDS = [(np.uint8, 8), (np.uint16, 10)]

_prepared = set()


def prepare(L):
    ic.prepare(L)
    if id(L) in _prepared:
        return L
    for n in ("lbd", "hbd"):
        f = getattr(L, f"svt_cfl_luma_subsampling_420_{n}_c")
        f.argtypes = [VP, C.c_int32, VP, C.c_int32, C.c_int32]; f.restype = None
        f = getattr(L, f"svt_cfl_predict_{n}_c")
        f.argtypes = [VP, VP, C.c_int32, VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]; f.restype = None
    L.svt_subtract_average_c.argtypes = [VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32]; L.svt_subtract_average_c.restype = None
    L.svt_av1_filter_intra_predictor_c.argtypes = [VP, C.c_ssize_t, C.c_uint8, VP, VP, C.c_int32]; L.svt_av1_filter_intra_predictor_c.restype = None
    L.highbd_filter_intra_predictor.argtypes = [VP, C.c_ssize_t, C.c_uint8, VP, VP, C.c_int, C.c_int]; L.highbd_filter_intra_predictor.restype = None
    _prepared.add(id(L))
    return L


def marker(dtype, which=0):
    return (0x5A, 0xA5)[which] if dtype == np.uint8 else (0x2A5, 0x15A)[which]


# ==================================================================================================== CfL
def cfl_valid(j):
    return j["tx_size"] in SHAPES and all(-16 <= a <= 16 for a in j["alpha"])


def cfl_dims(j):
    """Block size of a job; a job with an unusable tx_size still owns a 32x32 area of the planes (which must stay as it was)."""
    return ic.TX_WH[j["tx_size"]] if j["tx_size"] in SHAPES else (32, 32)


def cfl_job(rng, dtype, bd, tx_size, alpha, kind="random", plane_mask=3, dc_from_edges=0, dc_have=3):
    """kind: what the luma area holds -- "random"; "max" (AC identically 0); "extreme" (every 2x2 luma group all 0 or all maximum: the largest |AC|)."""
    hi = (1 << bd) - 1
    j = dict(tx_size=tx_size, alpha=tuple(alpha), plane_mask=plane_mask, dc_from_edges=dc_from_edges, dc_have=dc_have, kind=kind)
    w, h = cfl_dims(j)
    if kind == "max": luma = np.full((2 * h, 2 * w), hi)
    elif kind == "extreme": luma = np.kron(rng.integers(0, 2, (h, w)) * hi, np.ones((2, 2), np.int64))
    else: luma = rng.integers(0, hi + 1, (2 * h, 2 * w))
    j["luma"] = luma.astype(dtype)
    j["pred"] = rng.integers(0, hi + 1, (2, h, w)).astype(dtype)
    j["recs"] = rng.integers(0, hi + 1, (2, 2, EDGE_REC)).astype(dtype)
    return j


def cfl_basic_jobs(dtype, bd, seed=0):
    """Per shape six kinds of content (three random blocks, two extreme ones with alpha (16, -16) and (-16, 16), one all-maximum block), each as the in-place form and as
    dc_from_edges with the four dc_have values: 14 x 6 x 5 = 420 jobs.  The random alphas walk through -16 .. 16."""
    rng = np.random.default_rng(7000 + bd + seed)
    walk = iter(np.tile(rng.permutation(33) - 16, 17))   # 14 x 4 x 5 x 2 = 560 values
    jobs = []
    for t in SHAPES:
        kinds = [("random", None)] * 3 + [("extreme", (16, -16)), ("extreme", (-16, 16)), ("max", None)]
        for kind, alpha in kinds:
            for v in range(5):
                a = alpha if alpha is not None else (int(next(walk)), int(next(walk)))
                jobs.append(cfl_job(rng, dtype, bd, t, a, kind, 3, int(v > 0), max(v - 1, 0)))
    return jobs


def ref_cfl_job(L, j, bd):
    """-> (pred_buf_q3 [32][32] int16 after the average subtraction, zero outside the block; [cb, cr] blocks after svt_cfl_predict).  Both planes whatever the mask."""
    prepare(L)
    w, h = cfl_dims(j)
    hbd = j["luma"].dtype == np.uint16
    n = "hbd" if hbd else "lbd"
    ac = np.zeros((AC_LINE, AC_LINE), np.int16)
    luma = np.ascontiguousarray(j["luma"])
    getattr(L, f"svt_cfl_luma_subsampling_420_{n}_c")(luma.ctypes.data, 2 * w, ac.ctypes.data, 2 * w, 2 * h)
    L.svt_subtract_average_c(ac.ctypes.data, w, h, (w * h) >> 1, (w * h).bit_length() - 1)
    out = []
    for pl in (0, 1):
        if j["dc_from_edges"]: buf = ic.ref_predict(L, np.ascontiguousarray(j["recs"][pl]), bd, ic.make_job(tx_size=j["tx_size"], mode=0, dc_have=j["dc_have"]))
        else: buf = np.ascontiguousarray(j["pred"][pl]).copy()
        getattr(L, f"svt_cfl_predict_{n}_c")(ac.ctypes.data, buf.ctypes.data, w, buf.ctypes.data, w, j["alpha"][pl], bd, w, h)
        out.append(buf)
    return ac, out


def ref_cfl_jobs(L, jobs, bd):
    return [ref_cfl_job(L, j, bd) if cfl_valid(j) else None for j in jobs]


def _alloc(H, W, fill, dtype, view):
    """A plane, or (view) an offset view with an odd row stride of a larger array: nothing of it is aligned"""
    if not view: return np.full((H, W), fill, dtype)
    root = np.full((H + 3, W + 5 + (W & 1)), fill, dtype)
    return root[2:2 + H, 3:3 + W]


def cfl_layout(jobs, dtype, view=False, cols=16, cell=40, guard=4):
    """Job i gets cell i of a grid: its block `guard` samples inside the cell in both chroma planes, its luma area at twice those coordinates.
    -> (luma, cb, cr, positions)"""
    n = len(jobs)
    rows = max(1, (n + cols - 1) // cols)
    luma, cb, cr = _alloc(2 * rows * cell, 2 * cols * cell, 0, dtype, view), _alloc(rows * cell, cols * cell, marker(dtype, 0), dtype, view), _alloc(rows * cell, cols * cell, marker(dtype, 1), dtype, view)
    pos = []
    for i, j in enumerate(jobs):
        x, y = (i % cols) * cell + guard, (i // cols) * cell + guard
        w, h = cfl_dims(j)
        luma[2 * y:2 * y + 2 * h, 2 * x:2 * x + 2 * w] = j["luma"]; cb[y:y + h, x:x + w] = j["pred"][0]; cr[y:y + h, x:x + w] = j["pred"][1]
        pos.append((x, y))
    return luma, cb, cr, pos


def cfl_job_array(pkg, jobs, pos, order):
    arr = (pkg.CflJob * len(order))()
    for k, i in enumerate(order):
        J, j = arr[k], jobs[i]
        J.luma_x, J.luma_y, J.dst_x, J.dst_y = 2 * pos[i][0], 2 * pos[i][1], pos[i][0], pos[i][1]
        J.edge_off[0], J.edge_off[1] = (2 * i) * 2 * EDGE_REC, (2 * i + 1) * 2 * EDGE_REC
        J.alpha_q3[0], J.alpha_q3[1] = j["alpha"]
        J.tx_size, J.plane_mask, J.dc_from_edges, J.dc_have = j["tx_size"], j["plane_mask"], j["dc_from_edges"], j["dc_have"]
    return arr


def cfl_edges(jobs, dtype):
    return np.ascontiguousarray(np.stack([j["recs"] for j in jobs]).reshape(-1)) if jobs else np.zeros(4, dtype)


def root_of(a):
    while isinstance(a.base, np.ndarray): a = a.base
    return a


def same_plane(got, want):
    """The view and everything of the underlying array around it."""
    return got.shape == want.shape and np.array_equal(root_of(got), root_of(want))


def cfl_expected(jobs, refs, cb0, cr0, pos, order, give=(True, True)):
    """The planes (same layout as cb0 / cr0, what lies around a view included) and the AC buffer the call must leave."""
    def clone(p):
        r = root_of(p).copy()
        return np.ndarray(p.shape, p.dtype, r, p.ctypes.data - root_of(p).ctypes.data, p.strides)
    planes = [clone(cb0), clone(cr0)]
    ac = np.full((len(order), AC_LINE, AC_LINE), AC_MARK, np.int16)
    for k, i in enumerate(order):
        if refs[i] is None: continue
        j, (x, y), (w, h) = jobs[i], pos[i], cfl_dims(jobs[i])
        ac[k, :h, :w] = refs[i][0][:h, :w]
        for pl in (0, 1):
            if give[pl] and (j["plane_mask"] >> pl) & 1: planes[pl][y:y + h, x:x + w] = refs[i][1][pl]
    return planes[0], planes[1], ac


def cfl_check(hip, pkg, jobs, refs, dtype, order=None, view=False, give=(True, True), want_ac=True, what="", bd=None):
    """One launch of jobs[order] on the device against the per-job reference results: both planes whole (guard bands, unselected planes, what surrounds a view) and
    the whole AC buffer (pre-filled: nothing outside a job's W x H corner may change).  bd: default 8 for uint8, 10 for uint16."""
    order = list(range(len(jobs))) if order is None else list(order)
    luma, cb, cr, pos = cfl_layout(jobs, dtype, view)
    arr = cfl_job_array(pkg, jobs, pos, order)
    ac0 = np.full((len(order), AC_LINE, AC_LINE), AC_MARK, np.int16)
    got = hip.cfl_predict_batch(luma, cfl_edges(jobs, dtype), arr, cb if give[0] else None, cr if give[1] else None, want_ac=ac0 if want_ac else False, bd=bd)
    ecb, ecr, eac = cfl_expected(jobs, refs, cb, cr, pos, order, give)
    for pl, (g, e) in enumerate(zip(got[:2], (ecb, ecr))):
        if not give[pl]: assert g is None; continue
        if not same_plane(g, e):
            bad = np.argwhere(g != e)
            where = bad[0].tolist() if len(bad) else "outside the view"
            raise AssertionError(f"{what}: plane {pl} differs at {where} ({len(bad)} samples)")
    if want_ac: assert np.array_equal(got[2], eac), f"{what}: AC buffer differs at {np.argwhere(got[2] != eac)[:3].tolist()}"
    return got


def cfl_preclip(j, ac, bd):
    """alpha * ac and pred + ROUND_POWER_OF_TWO_SIGNED(alpha * ac, 6) before the clip, per plane, from the reference's AC values (in-place jobs only)."""
    w, h = cfl_dims(j)
    out = []
    for pl in (0, 1):
        prod = int(j["alpha"][pl]) * ac[:h, :w].astype(np.int64)
        scaled = np.where(prod < 0, -((-prod + 32) >> 6), (prod + 32) >> 6)
        out.append((prod, j["pred"][pl].astype(np.int64) + scaled))
    return out


def cfl_picture_jobs(dtype, bd, tw, w=352, h=288, seed=0):
    """A w x h 4:2:0 picture (the mixed frame of the intra tests as luma) tiled completely with tw x tw chroma blocks, in-place form, random alphas.
    -> (luma, cb, cr, CflJob fields as a list of dicts without per-job data)"""
    rng = np.random.default_rng(8100 + bd + tw + seed)
    luma = ic.mixed_frame(w, h)[:h, :w].astype(dtype)
    if bd > 8: luma = (luma << (bd - 8)) | rng.integers(0, 1 << (bd - 8), luma.shape).astype(dtype)
    hi = (1 << bd) - 1
    cw, ch = w // 2, h // 2
    yy, xx = np.mgrid[0:ch, 0:cw]
    cb = np.clip((hi / 2 + hi / 3 * np.sin(xx / 9.0) * np.cos(yy / 13.0)) + rng.integers(-3, 4, (ch, cw)), 0, hi).astype(dtype)
    cr = np.clip((hi / 2 + hi / 2.2 * np.cos(xx / 17.0 + yy / 5.0)) + rng.integers(-3, 4, (ch, cw)), 0, hi).astype(dtype)
    tx = {4: 0, 8: 1, 16: 2, 32: 3}[tw]
    tiles = [dict(x=x, y=y, tx_size=tx, alpha=(int(rng.integers(-16, 17)), int(rng.integers(-16, 17)))) for y in range(0, ch, tw) for x in range(0, cw, tw)]
    return np.ascontiguousarray(luma), cb, cr, tiles


def ref_cfl_picture(L, luma, cb, cr, tiles, bd):
    """The reference on the planes, tile by tile, in place."""
    prepare(L)
    n = "hbd" if luma.dtype == np.uint16 else "lbd"
    sz = luma.itemsize
    cb, cr = cb.copy(), cr.copy()
    ac = np.zeros((AC_LINE, AC_LINE), np.int16)
    for t in tiles:
        w, h = ic.TX_WH[t["tx_size"]]
        getattr(L, f"svt_cfl_luma_subsampling_420_{n}_c")(luma.ctypes.data + (2 * t["y"] * luma.shape[1] + 2 * t["x"]) * sz, luma.shape[1], ac.ctypes.data, 2 * w, 2 * h)
        L.svt_subtract_average_c(ac.ctypes.data, w, h, (w * h) >> 1, (w * h).bit_length() - 1)
        for p, a in ((cb, t["alpha"][0]), (cr, t["alpha"][1])):
            at = p.ctypes.data + (t["y"] * p.shape[1] + t["x"]) * sz
            getattr(L, f"svt_cfl_predict_{n}_c")(ac.ctypes.data, at, p.shape[1], at, p.shape[1], a, bd, w, h)
    return cb, cr


def cfl_picture_array(pkg, tiles):
    arr = (pkg.CflJob * len(tiles))()
    for J, t in zip(arr, tiles):
        J.luma_x, J.luma_y, J.dst_x, J.dst_y = 2 * t["x"], 2 * t["y"], t["x"], t["y"]
        J.alpha_q3[0], J.alpha_q3[1] = t["alpha"]
        J.tx_size, J.plane_mask = t["tx_size"], 3
    return arr


# ==================================================================================================== filter-intra
def fi_records(rng, n, dtype, bd, kind="random"):
    """Edge records; "extreme": every sample drawn from {0, maximum, random}, which drives the recursion past both ends of the range."""
    hi = (1 << bd) - 1
    r = rng.integers(0, hi + 1, (n, 2, EDGE_REC))
    if kind == "extreme":
        sel = rng.integers(0, 5, r.shape)   # 0 and the maximum twice as likely as a random value
        r[sel < 2] = 0; r[(sel >= 2) & (sel < 4)] = hi
        # every fourth record a maximum corner over zero edges, the next one the opposite: the first patch leaves the range at either end in every mode
        r[0::4] = 0; r[0::4, 0, EDGE_ORG - 1] = hi
        r[1::4] = hi; r[1::4, 0, EDGE_ORG - 1] = 0
    return r.astype(dtype)


def fi_all_jobs():
    """14 shapes x 5 modes"""
    return [(t, m) for t in SHAPES for m in range(5)]


def fi_valid(job):
    return job[0] in SHAPES and 0 <= job[1] <= 4


def fi_dims(job):
    return ic.TX_WH[job[0]] if job[0] in SHAPES else (32, 32)


def ref_filter_intra(L, rec, bd, tx, mode):
    prepare(L)
    w, h = ic.TX_WH[tx]
    rec = np.ascontiguousarray(rec)
    out = np.zeros((h, w), rec.dtype)
    sz = rec.itemsize
    a, l = rec[0].ctypes.data + EDGE_ORG * sz, rec[1].ctypes.data + EDGE_ORG * sz
    if rec.dtype == np.uint16: L.highbd_filter_intra_predictor(out.ctypes.data, w, tx, a, l, mode, bd)
    else: L.svt_av1_filter_intra_predictor_c(out.ctypes.data, w, tx, a, l, mode)
    return out


def ref_taps(L):
    """eb_av1_filter_intra_taps [5][8][8]"""
    return np.array([[list(row) for row in m] for m in (C.c_int8 * 8 * 8 * 5).in_dll(L, "eb_av1_filter_intra_taps")], np.int64)


def model_filter_intra(taps, rec, bd, tx, mode):
    """The recursion in Python with `taps` ([5][8][>= 7]): -> (block, number of outputs clipped at 0, number clipped at the maximum).  It exists to COUNT clips,
    which the reference's functions do not report; tests/test_cfl_ref_cpu.py first pins it to the reference bit for bit."""
    w, h = ic.TX_WH[tx]
    hi = (1 << bd) - 1
    buf = np.zeros((h + 1, w + 1), np.int64)
    buf[0, :] = rec[0][EDGE_ORG - 1:EDGE_ORG + w]; buf[1:, 0] = rec[1][EDGE_ORG:EDGE_ORG + h]
    lo_n = hi_n = 0
    for r in range(1, h + 1, 2):
        for c in range(1, w + 1, 4):
            p = [buf[r - 1, c - 1], buf[r - 1, c], buf[r - 1, c + 1], buf[r - 1, c + 2], buf[r - 1, c + 3], buf[r, c - 1], buf[r + 1, c - 1]]
            for k in range(8):
                v = sum(int(taps[mode][k][i]) * int(p[i]) for i in range(7))
                v = -((-v + 8) >> 4) if v < 0 else (v + 8) >> 4
                lo_n += v < 0; hi_n += v > hi
                buf[r + (k >> 2), c + (k & 3)] = min(max(v, 0), hi)
    return buf[1:, 1:].astype(rec.dtype), lo_n, hi_n


def fi_layout(jobs, dtype, view=False, cols=16, cell=40, guard=4):
    n = len(jobs)
    rows = max(1, (n + cols - 1) // cols)
    dst = _alloc(rows * cell, cols * cell, marker(dtype), dtype, view)
    return dst, [((i % cols) * cell + guard, (i // cols) * cell + guard) for i in range(n)]


def fi_check(hip, pkg, jobs, recs, refs, order=None, view=False, what="", bd=None):
    """One launch of jobs[order] (job i reads record i and owns cell i) against the per-job reference blocks (None = a job that must write nothing): the whole plane.
    bd: default 8 for uint8 records, 10 for uint16."""
    dtype = recs.dtype
    order = list(range(len(jobs))) if order is None else list(order)
    dst, pos = fi_layout(jobs, dtype, view)
    arr = (pkg.FilterIntraJob * len(order))()
    for k, i in enumerate(order):
        J = arr[k]
        J.edge_off, J.dst_x, J.dst_y, J.tx_size, J.mode = i * 2 * EDGE_REC, pos[i][0], pos[i][1], jobs[i][0], jobs[i][1]
    flat = np.ascontiguousarray(recs.reshape(-1)) if len(recs) else np.zeros(4, dtype)
    got = hip.filter_intra_predict_batch(flat, arr, dst, bd=bd)
    r = root_of(dst).copy()
    exp = np.ndarray(dst.shape, dst.dtype, r, dst.ctypes.data - root_of(dst).ctypes.data, dst.strides)
    for i in order:
        if refs[i] is not None:
            (x, y), (w, h) = pos[i], fi_dims(jobs[i])
            exp[y:y + h, x:x + w] = refs[i]
    if not same_plane(got, exp):
        bad = np.argwhere(got != exp)
        i = next((i for i in order if len(bad) and pos[i][0] - 4 <= bad[0][1] < pos[i][0] + 36 and pos[i][1] - 4 <= bad[0][0] < pos[i][1] + 36), None)
        raise AssertionError(f"{what}: differs at {bad[0].tolist() if len(bad) else 'outside the view'} ({len(bad)} samples), job {i} {jobs[i] if i is not None else ''}")
    return got
