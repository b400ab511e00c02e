"""Shared by the TPL dispenser tests: the reference's tpl_mc_flow_dispenser (Encoder/Codec/EbRateControlProcess.c:344-816) composed from functions
libsvtav1_ref.so exports, the seeded input generator, and the device side on the same inputs.

tpl_mc_flow_dispenser takes encoder objects, so -- as intra_common.ref_ois does for the intra search -- only its loop and the integer glue between the calls
are restated here; every computation is the reference's own function."""
import ctypes as C
import math

import numpy as np

import intra_common as ic

VP = C.c_void_p
PAD = 96                 # border the generated planes carry
INT64_MAX = 2 ** 63 - 1
N_SLOTS = 7              # MAX_PA_ME_MV: slots 0..3 list 0, 4..6 list 1
QINDEXES = (40, 140, 230)
STAT_FIELDS = ("srcrf_dist", "recrf_dist", "srcrf_rate", "recrf_rate", "mv_row", "mv_col", "rf_idx", "is_inter", "mode", "eob")
# SvtHipTplMbStats as the C compiler lays it out: 44 bytes of members, 8-byte alignment
STATS_DTYPE = np.dtype(dict(names=["srcrf_dist", "recrf_dist", "srcrf_rate", "recrf_rate", "mv_row", "mv_col", "rf_idx", "is_inter", "mode", "pad0", "eob", "pad1"],
                            formats=["<i8", "<i8", "<i8", "<i8", "<i2", "<i2", "i1", "u1", "u1", "u1", "<u2", "<u2"],
                            offsets=[0, 8, 16, 24, 32, 34, 36, 37, 38, 39, 40, 42], itemsize=48))

_prepared = set()


def prepare(L):
    if id(L) in _prepared:
        return L
    ic.prepare(L)
    L.svt_av1_quantize_fp_c.argtypes = [VP, C.c_ssize_t, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP]
    L.svt_av1_quantize_fp_c.restype = None
    L.svt_av1_block_error_c.argtypes = [VP, VP, C.c_ssize_t, VP]
    L.svt_av1_block_error_c.restype = C.c_int64
    L.av1_inv_transform_recon8bit.argtypes = [VP, VP, C.c_uint32, VP, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint8]
    L.svt_nxm_sad_kernel_helper_c.argtypes = [VP, C.c_uint32, VP, C.c_uint32, C.c_uint32, C.c_uint32]
    L.svt_nxm_sad_kernel_helper_c.restype = C.c_uint32
    L.generate_padding.argtypes = [VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    L.generate_padding.restype = None
    L.ref_shim_qparams.argtypes = [C.c_int, C.c_int, C.c_int, VP]
    _prepared.add(id(L))
    return L


def scan16(L):
    """av1_scan_orders[TX_16X16][DCT_DCT]: (scan, iscan)."""
    s, i = C.POINTER(C.c_int16)(), C.POINTER(C.c_int16)()
    n = L.ref_shim_scan(2, 0, C.byref(s), C.byref(i))
    assert n == 256
    return np.ctypeslib.as_array(s, (n,)).copy(), np.ctypeslib.as_array(i, (n,)).copy()


def qparams(L, qindex):
    """The 8-bit luma tables of a qindex, rows zbin, round, quant, quant_shift, dequant, round_fp, quant_fp, columns (dc, ac)."""
    out = np.zeros((7, 2), np.int16)
    prepare(L).ref_shim_qparams(8, qindex, 0, out.ctypes.data)
    return out


def zorder(mbw, mbh):
    """The reference's visiting order: superblocks in raster order, the sixteen 16x16 blocks of a 64x64 superblock in z-order."""
    out = []
    for sy in range(0, mbh, 4):
        for sx in range(0, mbw, 4):
            for k in range(16):
                x = sx + ((k & 1) | ((k >> 1) & 2)); y = sy + (((k >> 1) & 1) | ((k >> 2) & 2))
                if x < mbw and y < mbh: out.append((x, y))
    return out


def raster(mbw, mbh):
    return [(x, y) for y in range(mbh) for x in range(mbw)]


def wavefront(mbw, mbh):
    """x + 2y order, the device's."""
    return sorted(raster(mbw, mbh), key=lambda p: (p[0] + 2 * p[1], -p[1]))


def padded(pic, w, h, pad=PAD):
    """generate_padding's result for the w x h picture in `pic`: [h + 2 pad][w + 2 pad], every border sample the nearest picture sample."""
    return np.pad(pic[:h, :w], pad, mode="edge")


def mv_word(dx, dy, fx=0, fy=0):
    """The ME kernels' word for a full-sample vector (dx, dy) with quarter-sample fractions fx, fy (0..3): (y_mv << 16) | x_mv, int16 halves."""
    return ((((4 * dy + fy) & 0xFFFF) << 16) | ((4 * dx + fx) & 0xFFFF)) & 0xFFFFFFFF


def mv_offsets(word):
    """The reference's arithmetic: x_curr_mv = (int16_t)(x_mv << 1); offset = x_curr_mv >> 3.  Returns (dx, dy, mv_col, mv_row)."""
    def s16(v): return ((v & 0xFFFF) ^ 0x8000) - 0x8000
    col, row = s16(s16(word) << 1), s16(s16(word >> 16) << 1)
    return col >> 3, row >> 3, col, row


def make_case(w, h, seed, intra_tiles=0.25):
    """Current picture, three references in slots 0..2 (source and reconstruction planes, all with PAD samples of border), MV words [7][mbh][mbw], masks.
    The references are the padded current picture shifted by (3, -2), (-7, 5), (0, 0) plus uniform noise in +-3, a quarter of their 32x32 tiles replaced by
    unrelated content (there intra wins); reconstruction = source +-2 noise for slots 0 and 2, the source itself for slot 1; MVs = the true shift, 20 %
    jittered by +-2, 5 % drawn from +-64 (these leave the picture and read the border); mask = all slots for 70 % of the macroblocks, random 3-bit otherwise."""
    rng = np.random.default_rng(seed)
    pic = ic.mixed(rng, w, h); H, W = pic.shape
    mbw, mbh = W // 16, H // 16
    cur = padded(pic, w, h)
    refs = [None] * N_SLOTS
    mv = np.zeros((N_SLOTS, mbh, mbw), np.uint32)
    for r, (sx, sy) in enumerate([(3, -2), (-7, 5), (0, 0)]):
        big = np.roll(np.roll(cur, sy, 0), sx, 1).astype(np.int32) + rng.integers(-3, 4, cur.shape)
        src = np.clip(big, 0, 255).astype(np.uint8)[PAD:PAD + h, PAD:PAD + w].copy()
        other = ic.mixed(rng, w, h)[:h, :w]
        for ty in range(0, h, 32):
            for tx in range(0, w, 32):
                if rng.random() < intra_tiles: src[ty:ty + 32, tx:tx + 32] = other[ty:ty + 32, tx:tx + 32]
        sp = padded(src, w, h)
        recp = padded(np.clip(src.astype(np.int32) + rng.integers(-2, 3, src.shape), 0, 255).astype(np.uint8), w, h) if r != 1 else sp
        refs[r] = (sp, recp)
        m = np.zeros((mbh, mbw, 2), np.int64); m[..., 0] = sx; m[..., 1] = sy
        j = rng.random((mbh, mbw)) < 0.2; m[j] += rng.integers(-2, 3, (int(j.sum()), 2))
        far = rng.random((mbh, mbw)) < 0.05; m[far] = rng.integers(-64, 65, (int(far.sum()), 2))
        frac = rng.integers(0, 4, (mbh, mbw, 2))
        mv[r] = ((((4 * m[..., 1] + frac[..., 1]) & 0xFFFF) << 16) | ((4 * m[..., 0] + frac[..., 0]) & 0xFFFF)).astype(np.uint32)
    mask = (rng.integers(0, 8, (mbh, mbw)) | ((rng.random((mbh, mbw)) < 0.7) * 7)).astype(np.uint8)
    return dict(w=w, h=h, cur=cur, refs=refs, mv=mv, mask=mask)


def case_seed(w, h):
    return 7 + w + h


def cur_plane(case):
    """The view intra_common.ref_ois / device_ois take: sample (0, 0) of the current picture, readable over ceil16(w) x ceil16(h)."""
    return case["cur"][PAD:, PAD:]


def move_slots(case, mapping):
    """The same case with slot `a` moved to slot `b` for every (a, b) in mapping; slots not named disappear."""
    out = dict(case); out["refs"] = [None] * N_SLOTS; out["mv"] = np.zeros_like(case["mv"]); out["mask"] = np.zeros_like(case["mask"])
    for a, b in mapping.items():
        out["refs"][b] = case["refs"][a]; out["mv"][b] = case["mv"][a]
        out["mask"] |= (((case["mask"] >> a) & 1) << b).astype(np.uint8)
    return out


def clamp_case(case, pad, seed=5):
    """For the clamp test: the vectors of the outermost macroblocks point outwards by pad + 1 .. 64 samples, and every reference sample further than `pad`
    from the picture is noise instead of replication -- a border of `pad` samples is all the caller declares.  (On replicated planes a block wholly inside the
    border has the same content wherever it lies, and the clamp could not be observed.)"""
    rng = np.random.default_rng(seed)
    w, h = case["w"], case["h"]
    out = dict(case)
    mbh, mbw = case["mask"].shape
    m = np.zeros((N_SLOTS, mbh, mbw, 2), np.int64)
    for r in range(N_SLOTS): m[r] = np.array([mv_offsets(int(v))[:2] for v in case["mv"][r].ravel()]).reshape(mbh, mbw, 2)
    far = lambda n: rng.integers(pad + 1, 65, n)
    m[:, 0, :, 1] = -far((N_SLOTS, mbw)); m[:, -1, :, 1] = far((N_SLOTS, mbw)); m[:, :, 0, 0] = -far((N_SLOTS, mbh)); m[:, :, -1, 0] = far((N_SLOTS, mbh))
    out["mv"] = ((((4 * m[..., 1]) & 0xFFFF) << 16) | ((4 * m[..., 0]) & 0xFFFF)).astype(np.uint32)
    keep = np.zeros(case["cur"].shape, bool); keep[PAD - pad:PAD + h + pad, PAD - pad:PAD + w + pad] = True
    noisy = lambda p: np.where(keep, p, rng.integers(0, 256, p.shape).astype(np.uint8))
    refs = []
    for ref in case["refs"]:
        if ref is None: refs.append(None); continue
        sp = noisy(ref[0])
        refs.append((sp, sp if ref[1] is ref[0] else noisy(ref[1])))
    out["refs"] = refs
    return out


def all_intra(case):
    return move_slots(case, {})


def load_golden(path):
    """tests/golden/tpl_dispenser_200x136.npz (tests/golden/make_tpl_golden.py) -> (case, arrays): the borders re-created by replication."""
    g = np.load(path)
    h, w = g["cur"].shape
    refs = [None] * N_SLOTS
    for r in range(3):
        sp = padded(g[f"src{r}"], w, h)
        refs[r] = (sp, padded(g[f"rec{r}"], w, h) if f"rec{r}" in g.files else sp)
    mv = np.zeros((N_SLOTS,) + g["mask"].shape, np.uint32); mv[:3] = g["mv"]
    return dict(w=w, h=h, cur=padded(g["cur"], w, h), refs=refs, mv=mv, mask=g["mask"]), g


def golden_recon(g, name, w, h):
    """The stored reconstruction area with its PAD border (generate_padding = replication)."""
    return padded(g[name], w, h)


def stats_equal(a, b):
    """Every member of every record (the record's alignment padding carries nothing)."""
    return all((a[f] == b[f]).all() for f in STAT_FIELDS)


def rate_of(q, eob, scan):
    """rate_estimator (:114-128), with the interpreter's log1p / log."""
    r = 1
    for k in range(eob):
        r += int(math.log1p(abs(int(q[scan[k]]))) / math.log(2.0)) + 1
    return r << 9


def ref_dispenser(L, case, ois_mode, ois_cost, qp, order=None, use_ois=1, add_residual=1, rate=1, best_ref_only=0, pad=PAD):
    """The dispenser for one picture.  `pad` is the border the caller DECLARES (the planes carry PAD): a block position is kept inside
    [-pad, w + pad - 16] x [-pad, h + pad - 16] as the entry point documents, and the reconstruction gets `pad` samples of border.
    Returns (stats [mbh][mbw] STATS_DTYPE, reconstruction [h + 2 PAD][w + 2 PAD] whose samples beyond `pad` stay 0)."""
    prepare(L)
    w, h, cur = case["w"], case["h"], case["cur"]
    SCAN, ISCAN = scan16(L)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    S = cur.shape[1]
    rec = np.zeros_like(cur)
    stats = np.zeros((mbh, mbw), STATS_DTYPE)
    diff = np.zeros(256, np.int16); coeff = np.zeros(256, np.int32)
    a = np.empty(160, np.uint8); l = np.empty(160, np.uint8)
    zb, rnd, qnt, qsh, deq, rfp, qfp = [np.ascontiguousarray(np.repeat(r[[0, 1]], [1, 7])) for r in qp]   # SIMD-width layout, as txfm_common.ref_quant
    p = lambda arr: arr.ctypes.data
    org = lambda buf, x, y: buf.ctypes.data + (PAD + y) * S + PAD + x

    def quantize_error(c):   # get_quantize_error (:86-112)
        q = np.zeros(256, np.int32); dq = np.zeros(256, np.int32); eob = C.c_uint16(0); sse = C.c_int64(0)
        L.svt_av1_quantize_fp_c(p(c), 256, p(zb), p(rfp), p(qfp), p(qsh), p(q), p(dq), p(deq), C.addressof(eob), p(SCAN), p(ISCAN))
        err = L.svt_av1_block_error_c(p(c), p(dq), 256, C.addressof(sse)) >> 2
        return max(err, 1), q, dq, eob.value

    def position(word, x, y):
        dx, dy, col, row = mv_offsets(int(word))
        return min(max(x + dx, -pad), w + pad - 16), min(max(y + dy, -pad), h + pad - 16), col, row

    for (mx, my) in (order if order is not None else zorder(mbw, mbh)):
        x, y = mx * 16, my * 16
        best_intra, mode = (int(ois_cost[my, mx]), int(ois_mode[my, mx])) if use_ois else (INT64_MAX, 0)
        if mode > 12: mode = 0
        slots = [r for r in range(N_SLOTS) if case["refs"][r] is not None and (case["mask"][my, mx] >> r) & 1]
        if best_ref_only:   # get_best_reference (:287-339); without a valid slot best_reference stays 0, which is then not valid either
            best_sad, win = 2 ** 32 - 1, None
            for r in slots:
                bx, by, _, _ = position(case["mv"][r, my, mx], x, y)
                sad = L.svt_nxm_sad_kernel_helper_c(org(cur, x, y), S, org(case["refs"][r][0], bx, by), S, 16, 16)
                if sad < best_sad: best_sad, win = sad, r
            slots = [win] if win is not None else []
        best_inter, rf, bcoeff, bpos = INT64_MAX, -1, None, None
        for r in slots:
            bx, by, col, row = position(case["mv"][r, my, mx], x, y)
            L.svt_aom_subtract_block_c(16, 16, p(diff), 16, org(cur, x, y), S, org(case["refs"][r][0], bx, by), S)
            L.svt_av1_wht_fwd_txfm(p(diff), 16, p(coeff), 2, 8, 0)
            c = L.svt_aom_satd_c(p(coeff), 256)
            if c < best_inter: best_inter, rf, bcoeff, bpos = c, r, coeff.copy(), (bx, by, col, row)
        inter = best_inter < best_intra
        err, srate = 1, 0
        if inter:
            err, q, dq, eob = quantize_error(bcoeff)
            srate = rate_of(q, eob, SCAN) if rate else 0
        srcrf_dist, srcrf_rate = err << 4, srate << 4
        dst = org(rec, x, y)
        if inter:
            bx, by = bpos[:2]
            rec[PAD + y:PAD + y + 16, PAD + x:PAD + x + 16] = case["refs"][rf][1][PAD + by:PAD + by + 16, PAD + bx:PAD + bx + 16]
        else:
            a[:] = 0xAB; l[:] = 0xAB
            L.update_neighbor_samples_array_open_loop_mb_recon(p(a) + 15, p(l) + 15, org(rec, 0, 0), S, x, y, 16, 16, w, h)
            pa = ic.ANGLE.get(mode, 0)
            if 1 <= mode <= 8: L.filter_intra_edge(None, mode, w, h, pa, x, y, p(a) + 16, p(l) + 16)
            L.intra_prediction_open_loop_mb(pa, mode, x, y, 2, p(a) + 16, p(l) + 16, dst, S)
        L.svt_aom_subtract_block_c(16, 16, p(diff), 16, org(cur, x, y), S, dst, S)
        L.svt_av1_wht_fwd_txfm(p(diff), 16, p(coeff), 2, 8, 0)
        err, q, dq, eob = quantize_error(coeff)
        rrate = rate_of(q, eob, SCAN) if rate else 0
        if add_residual and eob: L.av1_inv_transform_recon8bit(p(dq), dst, S, dst, S, 2, 0, 0, eob, 0)
        recrf_dist, recrf_rate = err << 4, rrate << 4
        if not inter: srcrf_dist, srcrf_rate = recrf_dist, recrf_rate
        recrf_dist, recrf_rate = max(srcrf_dist, recrf_dist), max(srcrf_rate, recrf_rate)
        st = stats[my, mx]
        st["srcrf_dist"], st["recrf_dist"] = max(1, srcrf_dist // 16), max(1, recrf_dist // 16)
        st["srcrf_rate"], st["recrf_rate"] = max(1, srcrf_rate // 16), max(1, recrf_rate // 16)
        st["rf_idx"] = rf; st["is_inter"] = inter; st["mode"] = mode; st["eob"] = eob
        if rf >= 0: st["mv_col"], st["mv_row"] = bpos[2], bpos[3]
    L.generate_padding(org(rec, -pad, -pad), S, w, h, pad, pad)
    return stats, rec


def chain(stats):
    """Longest dependency chain among intra macroblocks (left, above, above-left, and (1, y - 1) for column 0)."""
    mbh, mbw = stats.shape; lv = np.zeros((mbh, mbw), np.int32)
    for y in range(mbh):
        for x in range(mbw):
            if stats["is_inter"][y, x]: continue
            d = [(x - 1, y), (x, y - 1), (x - 1, y - 1)] + ([(1, y - 1)] if x == 0 else [])
            lv[y, x] = 1 + max([lv[b, a_] for a_, b in d if 0 <= a_ < mbw and 0 <= b < mbh] + [0])
    return int(lv.max())


def summary(case, stats):
    """What the generator conditions are stated on, from the reference's result alone."""
    w, h = case["w"], case["h"]
    n = stats.size
    inter = stats["is_inter"] != 0
    wins = [int((inter & (stats["rf_idx"] == r)).sum()) for r in range(N_SLOTS)]
    leave = 0
    for my, mx in np.argwhere(inter):
        dx, dy, _, _ = mv_offsets(int(case["mv"][stats["rf_idx"][my, mx], my, mx]))
        x, y = 16 * mx + dx, 16 * my + dy
        leave += x < 0 or y < 0 or x + 16 > w or y + 16 > h
    return dict(n=n, inter_share=float(inter.sum()) / n, dir_intra_share=float((~inter & (stats["mode"] >= 1) & (stats["mode"] <= 8)).sum()) / n, chain=chain(stats),
                inter_eob0=int((inter & (stats["eob"] == 0)).sum()), inter_eobp=int((inter & (stats["eob"] > 0)).sum()),
                intra_eob0=int((~inter & (stats["eob"] == 0)).sum()), intra_eobp=int((~inter & (stats["eob"] > 0)).sum()), wins=wins, leave=int(leave))


# ---------------------------------------------------------------------------------------------------- the device side
def device_qparams(pkg, qp):
    """SvtHipQuantParams for svt_av1_quantize_fp from the table rows: round = round_fp, quant = quant_fp."""
    q = pkg.QuantParams()
    for k in range(2):
        q.zbin[k], q.round[k], q.quant[k], q.quant_shift[k], q.dequant[k] = int(qp[0, k]), int(qp[5, k]), int(qp[6, k]), int(qp[3, k]), int(qp[4, k])
    q.log_scale, q.variant, q.coeff_shape = 0, 2, 0
    return q


def _place(arr, extra_stride, offset):
    """`arr` inside a wider buffer: its rows `extra_stride` bytes longer, its first sample `offset` bytes into the buffer."""
    if not extra_stride and not offset:
        return np.ascontiguousarray(arr), arr.shape[1], 0
    stride = arr.shape[1] + extra_stride
    buf = np.full(arr.shape[0] * stride + offset + 64, 0x3C, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[offset:], arr.shape, (stride, 1))
    view[:] = arr
    return buf, stride, offset


GUARD = 24   # samples of marker around the area the entry point may write
MARK = 0xC3


def device_dispenser(hip, pkg, case, ois_mode, ois_cost, qp, use_ois=1, add_residual=1, rate=1, best_ref_only=0, pad=PAD, extra_stride=0, offset=0,
                     d_ois=None, calls=1):
    """The product on the same inputs.  Returns (stats, reconstruction [h + 2 pad][w + 2 pad], the whole destination buffer with its guard band).
    extra_stride / offset put every plane into a wider buffer at a byte offset (odd strides, unaligned bases).  d_ois = (d_mode, d_cost) uses tables already
    on the device.  calls > 1 repeats the call on a fresh destination and asserts identical bytes."""
    w, h = case["w"], case["h"]

    def up(arr, es, off):
        buf, stride, o = _place(arr, es, off)
        return s.upload(buf), stride, o

    with hip.scope() as s:
        d_cur, cs, co = up(case["cur"], extra_stride, offset)
        origin = lambda d, stride, o: C.c_void_p(d.value + o + PAD * stride + PAD)
        refs = [pkg.TplRef() for _ in range(N_SLOTS)]
        for r in range(N_SLOTS):
            if case["refs"][r] is None: continue
            sp, rp = case["refs"][r]
            ds, ss, so = up(sp, extra_stride + (r if extra_stride else 0), offset)
            refs[r].d_src, refs[r].src_stride = origin(ds, ss, so).value, ss
            if rp is sp:
                refs[r].d_rec, refs[r].rec_stride = refs[r].d_src, ss
            else:
                dr, rs, ro = up(rp, extra_stride, offset + (1 if offset else 0))
                refs[r].d_rec, refs[r].rec_stride = origin(dr, rs, ro).value, rs
        any_ref = any(x is not None for x in case["refs"])
        d_mv = s.upload(case["mv"]) if any_ref else None
        d_mask = s.upload(case["mask"]) if any_ref else None
        if d_ois is not None:
            d_mode, d_cost = d_ois
        elif use_ois or ois_mode is not None:
            d_mode, d_cost = s.upload(ois_mode.astype(np.uint8)), s.upload(ois_cost.astype(np.int32))
        else:
            d_mode = d_cost = None
        P = pkg.TplParams()
        P.w, P.h, P.pad, P.q = w, h, pad, device_qparams(pkg, qp)
        P.use_ois, P.add_residual, P.rate, P.best_ref_only = use_ois, add_residual, rate, best_ref_only
        rh, rw = h + 2 * (pad + GUARD), w + 2 * (pad + GUARD)
        result = None
        for _ in range(calls):
            host, rs, ro = _place(np.full((rh, rw), MARK, np.uint8), extra_stride + (5 if extra_stride else 0), offset)
            d_rec = s.upload(host)
            d_recon = C.c_void_p(d_rec.value + ro + (pad + GUARD) * rs + pad + GUARD)
            stats = hip.tpl_dispenser_picture(P, origin(d_cur, cs, co), cs, refs, d_mv, d_mask, d_mode, d_cost, d_recon, rs)
            whole = hip.to_host(d_rec, (host.size,), np.uint8)
            area = np.lib.stride_tricks.as_strided(whole[ro:], (rh, rw), (rs, 1))
            inner = area[GUARD:rh - GUARD, GUARD:rw - GUARD].copy()
            assert (hip.tpl_recon_to_host(d_recon, rs, w, h, pad) == inner).all()
            area[GUARD:rh - GUARD, GUARD:rw - GUARD] = MARK   # what is left must be the buffer as it was uploaded
            untouched = bool((whole == host.ravel()).all())
            got = (stats.view(STATS_DTYPE).copy(), inner, untouched)
            if result is not None:
                assert stats_equal(got[0], result[0]) and (got[1] == result[1]).all(), "two calls on the same inputs differ"
            result = got
        return result


def compare(dev_stats, dev_recon, ref_stats, ref_recon, pad=PAD):
    """Every field of every macroblock and every sample of the padded reconstruction, bit for bit."""
    for f in STAT_FIELDS:
        bad = np.argwhere(dev_stats[f] != ref_stats[f])
        assert bad.size == 0, f"{f}: {len(bad)} of {ref_stats.size} macroblocks differ; first (row, col) {bad[0].tolist()}: device {dev_stats[tuple(bad[0])]} " \
                              f"reference {ref_stats[tuple(bad[0])]}"
    o = PAD - pad
    want = ref_recon[o:ref_recon.shape[0] - o, o:ref_recon.shape[1] - o]
    bad = np.argwhere(dev_recon != want)
    assert bad.size == 0, f"reconstruction: {len(bad)} samples differ; first (row, col, border included) {bad[0].tolist()}: device {dev_recon[tuple(bad[0])]} " \
                          f"reference {want[tuple(bad[0])]}"
