"""Shared by the intra tests: the reference's open-loop intra search composed from functions libsvtav1_ref.so exports, the input generators,
and the reference side of the predictor batch tests (edge conditioning + predictor calls on numpy edge records)."""
import ctypes as C

import numpy as np

VP = C.c_void_p
ANGLE = {1: 90, 2: 180, 3: 45, 4: 135, 5: 113, 6: 157, 7: 203, 8: 67}
# TxSize -> (width, height)
TX_WH = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (4, 8), (8, 4), (8, 16), (16, 8), (16, 32), (32, 16), (32, 64), (64, 32), (4, 16), (16, 4),
         (8, 32), (32, 8), (16, 64), (64, 16)]
EDGE_REC, EDGE_ORG = 160, 16   # one edge of a record; element of sample 0

_prepared = set()


def prepare(L):
    """Once per library handle: the predictor tables the reference fills at start-up, and the prototypes of everything the intra tests call."""
    if id(L) in _prepared:
        return L
    L.init_intra_dc_predictors_c_internal()
    L.init_intra_predictors_internal()
    L.update_neighbor_samples_array_open_loop_mb_recon.argtypes = [VP, VP, VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint8, C.c_uint32, C.c_uint32]
    L.filter_intra_edge.argtypes = [VP, C.c_uint8, C.c_uint16, C.c_uint16, C.c_int32, C.c_int32, C.c_int32, VP, VP]
    L.filter_intra_edge.restype = None
    L.intra_prediction_open_loop_mb.argtypes = [C.c_int32, C.c_uint8, C.c_uint32, C.c_uint32, C.c_uint8, VP, VP, VP, C.c_uint32]
    L.svt_aom_subtract_block_c.argtypes = [C.c_int, C.c_int, VP, C.c_ssize_t, VP, C.c_ssize_t, VP, C.c_ssize_t]
    L.svt_aom_subtract_block_c.restype = None
    L.svt_av1_wht_fwd_txfm.argtypes = [VP, C.c_int, VP, C.c_uint8, C.c_int, C.c_int]
    L.svt_av1_wht_fwd_txfm.restype = None
    L.svt_aom_satd_c.argtypes = [VP, C.c_int]
    L.svt_aom_satd_c.restype = C.c_int
    # predictors and edge operations (the batch tests)
    L.dr_predictor.argtypes = [VP, C.c_ssize_t, C.c_uint8, VP, VP, C.c_int32, C.c_int32, C.c_int32]
    L.dr_predictor.restype = None
    L.highbd_dr_predictor.argtypes = [VP, C.c_ssize_t, C.c_uint8, VP, VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.highbd_dr_predictor.restype = None
    L.svt_av1_filter_intra_edge_c.argtypes = [VP, C.c_int32, C.c_int32]
    L.svt_av1_filter_intra_edge_c.restype = None
    L.svt_av1_filter_intra_edge_high_c.argtypes = [VP, C.c_int32, C.c_int32]
    L.svt_av1_filter_intra_edge_high_c.restype = None
    L.filter_intra_edge_corner.argtypes = [VP, VP]
    L.filter_intra_edge_corner.restype = None
    L.filter_intra_edge_corner_high.argtypes = [VP, VP]
    L.filter_intra_edge_corner_high.restype = None
    L.svt_av1_upsample_intra_edge_c.argtypes = [VP, C.c_int32]
    L.svt_av1_upsample_intra_edge_c.restype = None
    L.svt_av1_upsample_intra_edge_high_c.argtypes = [VP, C.c_int32, C.c_int32]
    L.svt_av1_upsample_intra_edge_high_c.restype = None
    L.use_intra_edge_upsample.argtypes = [C.c_int32] * 4
    L.use_intra_edge_upsample.restype = C.c_int32
    L.intra_edge_filter_strength.argtypes = [C.c_int32] * 4
    L.intra_edge_filter_strength.restype = C.c_int32
    _prepared.add(id(L))
    return L


def ref_ois(L, plane, w, h, mode_end=12, fill=0xAB):
    """open_loop_intra_search_mb (Encoder/Codec/EbMotionEstimation.c:3043-3155) for every macroblock, step by step through the reference's exported functions.
    plane: uint8 view of [>= ceil16(h)][>= ceil16(w)] samples (a strided / offset view works).  The neighbours come from
    update_neighbor_samples_array_open_loop_mb_recon (EbEncIntraPrediction.c:1282): its body is the body of the picture-descriptor variant the search calls
    (:1201), line for line, with `input_ptr->buffer_y + origin` replaced by the plane pointer and input_ptr->width / height by the two extra arguments.
    `fill` models the reference's uninitialised 160-byte stack arrays: the result must not depend on it."""
    prepare(L)
    stride, base = plane.strides[0], plane.ctypes.data
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    mode = np.zeros((mbh, mbw), np.uint8); cost = np.zeros((mbh, mbw), np.int64)
    a0, l0, a, l = (np.empty(160, np.uint8) for _ in range(4))
    pred = np.zeros(256, np.uint8); diff = np.zeros(256, np.int16); coeff = np.zeros(256, np.int32)
    for my in range(mbh):
        for mx in range(mbw):
            x, y = mx * 16, my * 16
            a0[:] = fill; l0[:] = fill
            L.update_neighbor_samples_array_open_loop_mb_recon(a0.ctypes.data + 15, l0.ctypes.data + 15, base, stride, x, y, 16, 16, w, h)
            best, bm = None, 0
            for m in range(mode_end + 1):
                pa = ANGLE.get(m, 0)
                if 1 <= m <= 8:
                    a[:] = a0; l[:] = l0
                    L.filter_intra_edge(None, m, w, h, pa, x, y, a.ctypes.data + 16, l.ctypes.data + 16)
                    ap, lp = a.ctypes.data + 16, l.ctypes.data + 16
                else:
                    ap, lp = a0.ctypes.data + 16, l0.ctypes.data + 16
                L.intra_prediction_open_loop_mb(pa, m, x, y, 2, ap, lp, pred.ctypes.data, 16)
                L.svt_aom_subtract_block_c(16, 16, diff.ctypes.data, 16, base + y * stride + x, stride, pred.ctypes.data, 16)
                L.svt_av1_wht_fwd_txfm(diff.ctypes.data, 16, coeff.ctypes.data, 2, 8, 0)
                c = L.svt_aom_satd_c(coeff.ctypes.data, 256)
                if best is None or c < best: best, bm = c, m
            mode[my, mx] = bm; cost[my, mx] = best
    return mode, cost


def mixed(rng, w, h):
    """64x64 tiles of oriented gratings, ramps, flat areas and a smooth texture, plus a little noise; beyond the picture its last column / row repeats."""
    H, W = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64); p = np.zeros((H, W))
    for ty in range(0, H, 64):
        for tx in range(0, W, 64):
            k = int(rng.integers(0, 11)); sl = (slice(ty, ty + 64), slice(tx, tx + 64))
            if k < 8:
                th = np.deg2rad([0, 90, 45, 135, 113, 157, 23, 67][k]); per = float(rng.uniform(9, 40))
                p[sl] = 128 + 90 * np.sin(2 * np.pi * (xx[sl] * np.cos(th) + yy[sl] * np.sin(th)) / per)
            elif k == 8: p[sl] = 40 + 1.5 * (xx[sl] - tx) + 1.2 * (yy[sl] - ty)
            elif k == 9: p[sl] = float(rng.integers(30, 220))
            else: p[sl] = 128 + 60 * np.sin(xx[sl] / 7.0) * np.cos(yy[sl] / 11.0)
    p = np.clip(np.rint(p + rng.normal(0, 2.0, (H, W))), 0, 255).astype(np.uint8)
    p[:, w:] = p[:, w - 1:w]; p[h:, :] = p[h - 1:h, :]
    return np.ascontiguousarray(p)


def noise(rng, w, h):
    H, W = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    p = rng.integers(0, 256, (H, W)).astype(np.uint8)
    p[:, w:] = p[:, w - 1:w]; p[h:, :] = p[h - 1:h, :]
    return np.ascontiguousarray(p)


def mixed_frame(w, h):
    return mixed(np.random.default_rng(20260 + w), w, h)


def device_ois(hip, plane, w, h, mode_end=12):
    """The product on the same samples: `plane` may be a strided / offset view; its base array is uploaded whole and the view's address handed over."""
    assert plane.dtype == np.uint8
    with hip.scope() as s:
        p = s.plane(plane)
        return hip.intra_ois_picture(p.ptr, p.stride, w, h, mode_end)


# ---------------------------------------------------------------------------------------------------- predictor batch: the reference side
def ref_condition(L, rec, hbd, bd, job):
    """The conditioning a job asks for, by the reference's functions, on a copy of the record `rec` ([2][160] samples)."""
    e = rec.copy()
    a, l = e[0].ctypes.data, e[1].ctypes.data
    sz = e.itemsize
    if job["corner_filter"]:
        (L.filter_intra_edge_corner_high if hbd else L.filter_intra_edge_corner)(a + EDGE_ORG * sz, l + EDGE_ORG * sz)
    flt = L.svt_av1_filter_intra_edge_high_c if hbd else L.svt_av1_filter_intra_edge_c
    start = EDGE_ORG - (1 if job["start_m1"] else 0)
    if job["strength_above"]: flt(a + start * sz, job["npx_above"], job["strength_above"])
    if job["strength_left"]: flt(l + start * sz, job["npx_left"], job["strength_left"])
    for base, on, n in ((a, job["upsample_above"], job["up_npx_above"]), (l, job["upsample_left"], job["up_npx_left"])):
        if on:
            if hbd: L.svt_av1_upsample_intra_edge_high_c(base + EDGE_ORG * sz, n, bd)
            else: L.svt_av1_upsample_intra_edge_c(base + EDGE_ORG * sz, n)
    return e


_NONDIR = {9: "smooth", 10: "smooth_v", 11: "smooth_h", 12: "paeth"}
_DC = {0: "dc_128", 1: "dc_left", 2: "dc_top", 3: "dc"}


def ref_predict(L, rec, bd, job):
    """The block a job describes ([h][w], the record's dtype) by the reference: conditioning, then the predictor of the mode."""
    prepare(L)
    hbd = rec.dtype == np.uint16
    e = ref_condition(L, rec, hbd, bd, job)
    sz = e.itemsize
    w, h = TX_WH[job["tx_size"]]
    out = np.zeros((h, w), rec.dtype)
    a, l = e[0].ctypes.data + EDGE_ORG * sz, e[1].ctypes.data + EDGE_ORG * sz
    m = job["mode"]
    if 1 <= m <= 8:
        ang = ANGLE[m] + 3 * job["angle_delta"]
        if hbd: L.highbd_dr_predictor(out.ctypes.data, w, job["tx_size"], a, l, job["upsample_above"], job["upsample_left"], ang, bd)
        else: L.dr_predictor(out.ctypes.data, w, job["tx_size"], a, l, job["upsample_above"], job["upsample_left"], ang)
        return out
    name = _DC[job["dc_have"]] if m == 0 else _NONDIR[m]
    f = getattr(L, f"svt_aom_{'highbd_' if hbd else ''}{name}_predictor_{w}x{h}_c")
    f.restype = None
    if hbd:
        f.argtypes = [VP, C.c_ssize_t, VP, VP, C.c_int32]
        f(out.ctypes.data, w, a, l, bd)
    else:
        f.argtypes = [VP, C.c_ssize_t, VP, VP]
        f(out.ctypes.data, w, a, l)
    return out


JOB_DEFAULT = dict(tx_size=0, mode=0, angle_delta=0, dc_have=3, corner_filter=0, strength_above=0, strength_left=0, npx_above=0, npx_left=0, start_m1=0,
                   upsample_above=0, upsample_left=0, up_npx_above=0, up_npx_left=0)


def make_job(**kw):
    j = dict(JOB_DEFAULT); j.update(kw)
    return j


def run_batch(hip, pkg, recs, jobs, bd):
    """One launch of all `jobs` (dicts; job i uses record i), each block at its own place of a destination plane pre-filled with a marker.
    Returns the list of predicted blocks ([h][w]) and the whole plane."""
    dt = recs.dtype
    n = len(jobs)
    cols = 16
    W, Hh = cols * 64, ((n + cols - 1) // cols) * 64 if n else 64
    marker = 0x5A if dt == np.uint8 else 0x2A5
    dst = np.full((Hh, W), marker, dt)
    arr = (pkg.IntraJob * max(n, 1))()
    for i, j in enumerate(jobs):
        J = arr[i]
        J.edge_off = i * 2 * EDGE_REC; J.dst_x = (i % cols) * 64; J.dst_y = (i // cols) * 64
        for k in JOB_DEFAULT: setattr(J, k, j[k])
    if n == 0:
        arr = (pkg.IntraJob * 0)()
    flat = np.ascontiguousarray(recs.reshape(-1)) if n else np.zeros(4, dt)
    out = hip.intra_predict_batch(flat, arr, dst, bd=bd)
    blocks = []
    for i, j in enumerate(jobs):
        if j["tx_size"] > 18:
            blocks.append(out[(i // cols) * 64:(i // cols) * 64 + 64, (i % cols) * 64:(i % cols) * 64 + 64]); continue
        w, h = TX_WH[j["tx_size"]]
        y0, x0 = (i // cols) * 64, (i % cols) * 64
        blocks.append(out[y0:y0 + h, x0:x0 + w])
        cell = out[y0:y0 + 64, x0:x0 + 64].copy(); cell[:h, :w] = marker
        assert (cell == marker).all(), f"job {i} wrote outside its block"
    return blocks, out


def random_records(rng, n, dtype, bd, kind="random"):
    hi = (1 << bd) - 1
    if kind == "zero": return np.zeros((n, 2, EDGE_REC), dtype)
    if kind == "max": return np.full((n, 2, EDGE_REC), hi, dtype)
    return rng.integers(0, hi + 1, (n, 2, EDGE_REC)).astype(dtype)
