"""The dual interpolation filter search (interpolation_filter_search, Encoder/Codec/EbEncInterPrediction.c:3047-3297 of the reference) restated in numpy and Python
integers, the job lists the CPU and GPU tests share, and record <-> ctypes helpers.  Nothing here calls the library under test.

A case is a dict: "src" the source luma plane (a view, its stride is no multiple of 64), "ref" [array, array] the two reference pictures WITH their border -- exactly
REACH_LO samples left and above and REACH_HI right and below of the W x H picture, so a read outside the contract leaves the array --, "bd", "jobs" a list of dicts with
the members of SvtHipIfsJob (rate_tab a 2 x 3 list) plus "page": jobs of one page have disjoint destination rectangles."""
import ctypes as C
import functools
import os

import numpy as np

from conftest import ROOT
from scaled_common import taps

GOLDEN = os.path.join(ROOT, "tests", "golden", "ifs_search.npz")

BLOCK_W = [4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64]
BLOCK_H = [4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16]
SIZES = [b for b in range(22) if BLOCK_W[b] >= 8 and BLOCK_H[b] >= 8]   # the 17 shapes
REACH_LO, REACH_HI = 3, 4
W = H = 256
NCAND = 9
FILTER_SETS = [(y, x) for y in range(3) for x in range(3)]   # filter_sets[i] = {y filter, x filter}
QUANT_DIST = [(9, 7), (11, 5), (12, 4), (13, 3)]             # quant_dist_lookup_table
MAX_XSQ_Q10 = 245727
JOB_FIELDS = ("bsize", "x", "y", "ref0_x", "ref0_y", "ref1_x", "ref1_y", "subpel0_x", "subpel0_y", "subpel1_x", "subpel1_y", "type", "fwd_offset", "bck_offset", "order", "dual",
              "quantizer", "full_lambda", "dst_x", "dst_y")

# model_rd_norm's three tables (EbEncInterPrediction.c:2808-2844)
RATE_TAB_Q10 = [65536, 6086, 5574, 5275, 5063, 4899, 4764, 4651, 4553, 4389, 4255, 4142, 4044, 3958, 3881, 3811, 3748, 3635, 3538, 3453, 3376, 3307, 3244, 3186, 3133, 3037,
                2952, 2877, 2809, 2747, 2690, 2638, 2589, 2501, 2423, 2353, 2290, 2232, 2179, 2130, 2084, 2001, 1928, 1862, 1802, 1748, 1698, 1651, 1608, 1530, 1460, 1398,
                1342, 1290, 1243, 1199, 1159, 1086, 1021, 963, 911, 864, 821, 781, 745, 680, 623, 574, 530, 490, 455, 424, 395, 345, 304, 269, 239, 213, 190, 171, 154, 126,
                104, 87, 73, 61, 52, 44, 38, 28, 21, 16, 12, 10, 8, 6, 5, 3, 2, 1, 1, 1, 0, 0]
DIST_TAB_Q10 = [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5, 5, 6, 7, 7, 8, 9, 11, 12, 13, 15, 16, 17, 18, 21, 24, 26, 29, 31, 34, 36, 39, 44, 49, 54, 59, 64, 69, 73, 78, 88, 97, 106, 115,
                124, 133, 142, 151, 167, 184, 200, 215, 231, 245, 260, 274, 301, 327, 351, 375, 397, 418, 439, 458, 495, 528, 559, 587, 613, 637, 659, 680, 717, 749, 777, 801,
                823, 842, 859, 874, 899, 919, 936, 949, 960, 969, 977, 983, 994, 1001, 1006, 1010, 1013, 1015, 1017, 1018, 1020, 1022, 1022, 1023, 1023, 1023, 1024]
XSQ_IQ_Q10 = [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 72, 80, 88, 96, 112, 128, 144, 160, 176, 192, 208, 224, 256, 288, 320, 352, 384, 416, 448, 480, 544, 608, 672,
              736, 800, 864, 928, 992, 1120, 1248, 1376, 1504, 1632, 1760, 1888, 2016, 2272, 2528, 2784, 3040, 3296, 3552, 3808, 4064, 4576, 5088, 5600, 6112, 6624, 7136, 7648,
              8160, 9184, 10208, 11232, 12256, 13280, 14304, 15328, 16352, 18400, 20448, 22496, 24544, 26592, 28640, 30688, 32736, 36832, 40928, 45024, 49120, 53216, 57312,
              61408, 65504, 73696, 81888, 90080, 98272, 106464, 114656, 122848, 131040, 147424, 163808, 180192, 196576, 212960, 229344, 245728]
assert len(RATE_TAB_Q10) == len(DIST_TAB_Q10) == len(XSQ_IQ_Q10) == 104


# ------------------------------------------------------------------------------------------------------------------ the model
def model_xsq(var, n_log2, qstep):
    """the clamped abscissa of svt_av1_model_rd_from_var_lapndz (var > 0) and whether the clamp was reached"""
    x = ((qstep * qstep << (n_log2 + 10)) + (var >> 1)) // var
    return min(x, MAX_XSQ_Q10), x >= MAX_XSQ_Q10


def model_xq(xsq):
    tmp = (xsq >> 2) + 8
    k = tmp.bit_length() - 1 - 3
    return (k << 3) + ((tmp >> k) & 7), k


def model_lapndz(var, n_log2, qstep):
    """svt_av1_model_rd_from_var_lapndz -> (rate, dist)"""
    if var == 0:
        return 0, 0
    xsq, _ = model_xsq(var, n_log2, qstep)
    xq, k = model_xq(xsq)
    a = ((xsq - XSQ_IQ_Q10[xq]) << 10) >> (2 + k)
    b = 1024 - a
    r = (RATE_TAB_Q10[xq] * b + RATE_TAB_Q10[xq + 1] * a) >> 10
    d = (DIST_TAB_Q10[xq] * b + DIST_TAB_Q10[xq + 1] * a) >> 10
    return ((r << n_log2) + 1) >> 1, (var * d + 512) >> 10


def model_from_sse(bsize, quantizer, bd, sse):
    """model_rd_from_sse with simple_model_rd_from_var = 0 -> (rate, dist)"""
    rate, dist = model_lapndz(sse, (BLOCK_W[bsize] * BLOCK_H[bsize]).bit_length() - 1, quantizer >> (bd - 5))
    return rate, dist << 4


def rdcost(rm, rate, dist):
    return ((rate * rm + 256) >> 9) + dist * 128


def model_points():
    """(var, n_log2, qstep) whose abscissa is every value of xsq_iq_q10, the value before it, and the clamp: every segment boundary of model_rd_norm from both sides"""
    out = [(1, 6, 0), (12345, 14, 0), (0, 8, 77)]
    n_log2, qstep = 14, 4095
    num = qstep * qstep << (n_log2 + 10)
    for t in sorted({v for x in XSQ_IQ_Q10[1:] for v in (x - 1, x) if v <= MAX_XSQ_Q10} | {1, 2, 3, MAX_XSQ_Q10 - 1}):   # the last entry is beyond the clamp
        var = num // t
        while model_xsq(var, n_log2, qstep)[0] > t:
            var += 1
        assert model_xsq(var, n_log2, qstep) == (t, t == MAX_XSQ_Q10), t
        out.append((var, n_log2, qstep))
    out += [(num // MAX_XSQ_Q10, n_log2, qstep), (1, n_log2, qstep), (7, 6, 3), (1 << 40, 12, 1)]
    return out


# ------------------------------------------------------------------------------------------------------------------ the predictions
def rp2(v, n):
    return v if n == 0 else (v + (1 << (n - 1))) >> n


def d16_offset(bd):
    ob = bd + 14 - 3
    return (1 << (ob - 7)) + (1 << (ob - 8))


def ref_block(win, bw, bh, sx, sy, fy, fx, bd, comp, lowbd):
    """one reference's block from its (bh + 7) x (bw + 7) window: the pixels of svt_av1_[highbd_]convolve_*_sr (comp False) or the 16-bit values of
    svt_av1_[highbd_]jnt_convolve_* before the average (comp True).  -> (values, the branch taken 0 copy / 1 x / 2 y / 3 2-D)"""
    T = taps()
    win = win.astype(np.int64)
    assert win.shape == (bh + 7, bw + 7)
    core, off, top = win[3:3 + bh, 3:3 + bw], d16_offset(bd), (1 << bd) - 1
    if not sx and not sy:
        return ((core << 4) + off if comp else core), 0
    if not sy:
        res = sum(int(T[fx][sx][k]) * win[3:3 + bh, k:k + bw] for k in range(8))
        return (rp2(res, 3) + off if comp else np.clip(rp2(rp2(res, 3), 4), 0, top)), 1
    if not sx:
        res = sum(int(T[fy][sy][k]) * win[k:k + bh, 3:3 + bw] for k in range(8))
        return (rp2(res * 16, 7) + off if comp else np.clip(rp2(res, 7), 0, top)), 2
    im = rp2(sum(int(T[fx][sx][k]) * win[:, k:k + bw] for k in range(8)) + (1 << (bd + 6)), 3).astype(np.int16).astype(np.int64)
    s = sum(int(T[fy][sy][k]) * im[k:k + bh] for k in range(8))
    ob = bd + 14 - 3
    if comp:
        return rp2(s + (1 << ob), 7).astype(np.uint16).astype(np.int64), 3
    res = rp2(s + (1 << ob), 11) - ((1 << (ob - 11)) + (1 << (ob - 12)))
    if lowbd:
        res = res.astype(np.int16).astype(np.int64)
    return np.clip(res, 0, top), 3


def window(case, r, j):
    """the (bh + 7) x (bw + 7) window of reference r of job j; it must lie inside the array: that is the border contract"""
    bw, bh = BLOCK_W[j["bsize"]], BLOCK_H[j["bsize"]]
    x, y = j["ref%d_x" % r], j["ref%d_y" % r]
    a = case["ref"][r]
    assert 0 <= x <= W - bw and 0 <= y <= H - bh
    w = a[y:y + bh + 7, x:x + bw + 7]   # the array's (0, 0) is the picture's (-3, -3)
    assert w.shape == (bh + 7, bw + 7)
    return w


def predict(case, j, i, info=None):
    """the luma prediction of job j under filter pair i"""
    bw, bh, bd = BLOCK_W[j["bsize"]], BLOCK_H[j["bsize"]], case["bd"]
    fy, fx = FILTER_SETS[i]
    lowbd = case["src"].itemsize == 1
    if j["type"] < 0:
        p, br = ref_block(window(case, 0, j), bw, bh, j["subpel0_x"], j["subpel0_y"], fy, fx, bd, False, lowbd)
        if info is not None:
            info.setdefault("branches", set()).add((1, br))
        return p
    d0, b0 = ref_block(window(case, 0, j), bw, bh, j["subpel0_x"], j["subpel0_y"], fy, fx, bd, True, lowbd)
    d1, b1 = ref_block(window(case, 1, j), bw, bh, j["subpel1_x"], j["subpel1_y"], fy, fx, bd, True, lowbd)
    if info is not None:
        info.setdefault("branches", set()).update({(2, b0), (3, b1)})
    tmp = (d0 * j["fwd_offset"] + d1 * j["bck_offset"]) >> 4 if j["type"] else (d0 + d1) >> 1
    return np.clip(rp2(tmp - d16_offset(bd), 4), 0, (1 << bd) - 1)


def evaluated(j, i):
    return not (j["order"] == 1 and not j["dual"] and FILTER_SETS[i][0] != FILTER_SETS[i][1])


def run_job(case, j, info=None):
    """-> (result (best, interp_filters, switchable_rate, regular_last, rd), [9 x (rate, sse, dist, rd)], the winner's prediction)"""
    bw, bh, bd = BLOCK_W[j["bsize"]], BLOCK_H[j["bsize"]], case["bd"]
    s = case["src"][j["y"]:j["y"] + bh, j["x"]:j["x"] + bw].astype(np.int64)
    assert s.shape == (bh, bw)
    cands, preds = [], {}
    for i, (fy, fx) in enumerate(FILTER_SETS):
        if not evaluated(j, i):
            cands.append((-1, 0, 0, 0))
            continue
        preds[i] = predict(case, j, i, info)
        sse = int(((s - preds[i]) ** 2).sum())
        rounded = (sse + ((1 << (2 * (bd - 8))) >> 1)) >> (2 * (bd - 8))
        rate, dist = model_from_sse(j["bsize"], j["quantizer"], bd, rounded)
        if info is not None and rounded:
            xsq, clamped = model_xsq(rounded, (bw * bh).bit_length() - 1, j["quantizer"] >> (bd - 5))
            info.setdefault("clamp", set()).add(clamped)
        rate += j["rate_tab"][0][fy] + j["rate_tab"][1][fx]
        cands.append((rate, sse, dist, rdcost(j["full_lambda"], rate, dist)))
    rd, best = (1 << 64) - 1, 0
    for i in (range(NCAND) if j["order"] == 0 else range(NCAND - 1, -1, -1)):
        if evaluated(j, i) and cands[i][3] < rd:
            rd, best = cands[i][3], i
    fy, fx = FILTER_SETS[best]
    res = (best, fy | fx << 16, j["rate_tab"][0][fy] + j["rate_tab"][1][fx], (int(best == 0) if j["order"] == 1 else -1), rd)
    return res, cands, preds[best]


def run_case(case, infos=None):
    return [run_job(case, j, infos[k] if infos is not None else None) for k, j in enumerate(case["jobs"])]


# ------------------------------------------------------------------------------------------------------------------ pictures and job lists
@functools.lru_cache(None)
def pictures(bd, dtype_name):
    """(source view, [reference 0, reference 1] with their 3 / 4 border): a smooth texture with edges and noise; the references are the source moved by a sample or two
    plus noise, equal to the source in the top-left 64 x 64; flat patches at 0 and at the top value"""
    rng = np.random.default_rng(1234)
    top = (1 << bd) - 1
    n = W + 16
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    base = 0.5 + 0.22 * np.sin(xx / 5.1 + yy / 9.3) + 0.18 * np.sin(xx / 2.3 - yy / 3.7) + 0.12 * ((xx // 13 + yy // 11) % 2) + 0.05 * rng.standard_normal((n, n))
    img = np.clip(np.rint(base * top), 0, top).astype(np.int64)
    pic = img[8:8 + H, 8:8 + W]   # a view: the patches are in picture coordinates
    pic[100:140, 60:120] = top
    pic[150:200, 150:230] = 0
    pic[30:40, 200:240] = rng.integers(0, 2, (10, 40)) * top   # full-swing noise: the filters over- and undershoot
    store = np.zeros((H, W + 8), dtype_name)
    src = store[:, :W]
    src[:] = img[8:8 + H, 8:8 + W]
    refs = []
    for r, (dy, dx) in enumerate(((1, -2), (-1, 1))):
        a = img[8 - REACH_LO + dy:8 + H + REACH_HI + dy, 8 - REACH_LO + dx:8 + W + REACH_HI + dx] + rng.integers(-3 - 3 * r, 4 + 3 * r, (H + 7, W + 7))
        a = np.clip(a, 0, top)
        a[REACH_LO:REACH_LO + 64, REACH_LO:REACH_LO + 64] = img[8:8 + 64, 8:8 + 64]
        refs.append(np.ascontiguousarray(a.astype(dtype_name)))
    return src, refs


def ref_view(a):
    """the W x H picture inside a reference array"""
    return a[REACH_LO:REACH_LO + H, REACH_LO:REACH_LO + W]


QUANTIZERS = [1, 8, 37, 120, 500, 1400, 5000, 32767]
LAMBDAS = [1, 150, 3000, 52000, 1 << 20]


def job(bsize, x, y, mv0=(0, 0), ph0=(0, 0), mv1=(0, 0), ph1=(0, 0), type=-1, w=(8, 8), order=0, dual=1, q=120, lam=3000, rates=None):
    bw, bh = BLOCK_W[bsize], BLOCK_H[bsize]
    cl = lambda v, hi: min(max(v, 0), hi)
    return dict(bsize=bsize, x=x, y=y, ref0_x=cl(x + mv0[0], W - bw), ref0_y=cl(y + mv0[1], H - bh), ref1_x=cl(x + mv1[0], W - bw), ref1_y=cl(y + mv1[1], H - bh),
                subpel0_x=ph0[0], subpel0_y=ph0[1], subpel1_x=ph1[0], subpel1_y=ph1[1], type=type, fwd_offset=w[0], bck_offset=w[1], order=order, dual=dual, quantizer=q,
                full_lambda=lam, rate_tab=[list(r) for r in (rates or ((0, 0, 0), (0, 0, 0)))], dst_x=0, dst_y=0, page=0)


def steer(t, big=40000):
    """rates under which pair t is the cheapest by far"""
    fy, fx = FILTER_SETS[t]
    return [[0 if f == fy else big for f in range(3)], [0 if f == fx else big for f in range(3)]]


@functools.lru_cache(None)
def job_list():
    rng = np.random.default_rng(77)
    ri = lambda lo, hi: int(rng.integers(lo, hi))
    pos = lambda b: (ri(0, W - BLOCK_W[b] + 1), ri(0, H - BLOCK_H[b] + 1))
    mv = lambda: (ri(-3, 4), ri(-3, 4))
    ph = lambda: (ri(1, 16), ri(1, 16))
    anyph = lambda: (ri(0, 16) * ri(0, 2), ri(0, 16) * ri(0, 2))
    rates = lambda: [[ri(0, 3000) for _ in range(3)] for _ in range(2)]
    weights = [w for a, b in QUANT_DIST for w in ((a, b), (b, a))]
    jobs = []
    # every shape: one reference with both phases, two references of either type
    for k, b in enumerate(SIZES):
        jobs.append(job(b, *pos(b), mv0=mv(), ph0=ph(), order=k & 1, q=QUANTIZERS[k % 8], lam=LAMBDAS[k % 5], rates=rates()))
        jobs.append(job(b, *pos(b), mv0=mv(), ph0=anyph() if k % 3 else ph(), mv1=mv(), ph1=ph(), type=k & 1, w=weights[k % 8], order=(k >> 1) & 1, q=QUANTIZERS[(k + 3) % 8],
                        lam=LAMBDAS[(k + 2) % 5], rates=rates()))
    # every dispatch branch: one reference, and each reference of two
    branch = [(0, 0), (5, 0), (0, 11), (7, 13)]
    for b in (3, 6):
        for p in branch:
            jobs.append(job(b, *pos(b), mv0=mv(), ph0=p, order=ri(0, 2), rates=rates()))
    for k, (p0, p1) in enumerate((a, c) for a in branch for c in branch):
        jobs.append(job((6, 4)[k & 1], *pos(6), mv0=mv(), ph0=p0, mv1=mv(), ph1=p1, type=(k >> 1) & 1, w=weights[k % 8], order=k & 1, rates=rates()))
    # every pair winning: the rates decide
    for t in range(NCAND):
        jobs.append(job((6, 8, 4)[t % 3], *pos(8), mv0=mv(), ph0=ph(), order=0, rates=steer(t)))
        jobs.append(job((5, 7, 3)[t % 3], *pos(7), mv0=mv(), ph0=ph(), mv1=mv(), ph1=ph(), type=t & 1, w=weights[t % 8], order=1, dual=1, rates=steer(t)))
    for t in (0, 4, 8):
        jobs.append(job(6, *pos(6), mv0=mv(), ph0=ph(), order=1, dual=0, rates=steer(t)))
        jobs.append(job(9, *pos(9), mv0=mv(), ph0=ph(), order=1, dual=0, rates=rates()))
    # ties: the two orders on one job.  One direction filtered (pairs tie in threes), whole-sample with distinct rates, whole-sample with equal rates
    for p, r in (((9, 0), None), ((0, 6), None), ((0, 0), [[700, 20, 300], [41, 900, 5]]), ((0, 0), [[64, 64, 64], [9, 9, 9]]), ((0, 0), None)):
        x, y = pos(6)
        m = mv()
        for order in (0, 1):
            jobs.append(job(6, x, y, mv0=m, ph0=p, order=order, rates=r))
    # sse == 0: the references equal the source in the top-left 64 x 64
    jobs.append(job(6, 16, 24, order=0, rates=rates()))
    jobs.append(job(8, 8, 40, type=0, order=1, rates=rates()))
    jobs.append(job(3, 40, 8, type=1, w=(11, 5), order=0, rates=rates()))
    # the quantizer's ends; a small and a large lambda
    for q in (1, 32767):
        for lam in (1, 1 << 20):
            jobs.append(job(6, *pos(6), mv0=mv(), ph0=ph(), q=q, lam=lam, order=ri(0, 2), rates=rates()))
    # the whole border at every picture edge, strips included: 128x128 in two corners, 64x128, 32x32 and 8x8 in all four
    for b in (15, 13, 9, 3):
        bw, bh = BLOCK_W[b], BLOCK_H[b]
        for cx, cy in ((0, 0), (W - bw, H - bh)) if b == 15 else ((0, 0), (W - bw, 0), (0, H - bh), (W - bw, H - bh)):
            two = (cx + cy + b) % 3 == 0
            jobs.append(job(b, cx, cy, ph0=ph(), ph1=ph(), type=ri(0, 2) if two else -1, w=weights[ri(0, 8)], order=ri(0, 2), q=QUANTIZERS[ri(0, 8)], rates=rates()))
    # the flat patches and the checker noise
    for b, x, y in ((6, 70, 110), (6, 160, 160), (8, 200, 26), (5, 208, 30), (9, 56, 96), (9, 140, 140)):
        jobs.append(job(b, x, y, mv0=mv(), ph0=ph(), order=ri(0, 2), rates=rates()))
        jobs.append(job(b, x, y, mv0=mv(), ph0=anyph(), mv1=mv(), ph1=ph(), type=ri(0, 2), w=weights[ri(0, 8)], order=ri(0, 2), rates=rates()))
    # a random tail of small blocks
    for _ in range(70):
        b = (3, 4, 5, 6, 7, 8, 9, 18, 19)[ri(0, 9)]
        two = ri(0, 3) == 0
        jobs.append(job(b, *pos(b), mv0=mv(), ph0=anyph(), mv1=mv(), ph1=anyph(), type=ri(0, 2) if two else -1, w=weights[ri(0, 8)], order=ri(0, 2), dual=ri(0, 2),
                        q=QUANTIZERS[ri(0, 8)], lam=LAMBDAS[ri(0, 5)], rates=rates()))
    # destination rectangles: shelves of a W x H plane, a new page when it is full
    page, sx, sy, sh = 0, 0, 0, 0
    for j in sorted(jobs, key=lambda j: -BLOCK_H[j["bsize"]]):
        bw, bh = BLOCK_W[j["bsize"]], BLOCK_H[j["bsize"]]
        if sx + bw > W:
            sx, sy, sh = 0, sy + sh, 0
        if sy + bh > H:
            page, sx, sy, sh = page + 1, 0, 0, 0
        j["dst_x"], j["dst_y"], j["page"] = sx, sy, page
        sx, sh = sx + bw, max(sh, bh)
    return jobs


def build_case(bd, dtype):
    src, refs = pictures(bd, np.dtype(dtype).name)
    return {"src": src, "ref": refs, "bd": bd, "jobs": job_list()}


def job_ok(j, have_ref1=True):
    """what the library refuses of a job (ifs::job_ok)"""
    b = j["bsize"]
    if not (0 <= b < 22) or BLOCK_W[b] < 8 or BLOCK_H[b] < 8:
        return False
    if not (0 <= j["x"] <= W - BLOCK_W[b] and 0 <= j["y"] <= H - BLOCK_H[b]) or j["type"] not in (-1, 0, 1) or (j["type"] >= 0 and not have_ref1):
        return False
    ph = [j["subpel0_x"], j["subpel0_y"]] + ([j["subpel1_x"], j["subpel1_y"]] if j["type"] >= 0 else [])
    if any(not 0 <= p <= 15 for p in ph) or (j["type"] == 1 and (min(j["fwd_offset"], j["bck_offset"]) < 0 or j["fwd_offset"] + j["bck_offset"] != 16)):
        return False
    return j["order"] in (0, 1) and 1 <= j["quantizer"] <= 32767


# ------------------------------------------------------------------------------------------------------------------ the recorded calls
def golden_calls(bd):
    """the calls of tests/golden/ifs_search.npz at one depth -> [(case of one job, what the reference did)]: the job sits at (0, 0) of its own source block, its two
    reference arrays are the recorded windows; the record is (interp_filters, switchable_rate, ifs_is_regular_last or 7 where the reference left it alone,
    [(pair, tmp_rd), ...] in evaluation order)"""
    g = np.load(GOLDEN)
    fields = g["fields"].tolist()
    src, win, so, wo, out = g["src_%d" % bd], g["win_%d" % bd], 0, 0, []
    for row, o, ev, rd in zip(g["calls_%d" % bd].tolist(), g["out_%d" % bd].tolist(), g["eval_%d" % bd].tolist(), g["tmp_rd_%d" % bd].tolist()):
        j = dict(zip(fields, row))
        j["rate_tab"] = [[j.pop("rate_y%d" % f) for f in range(3)], [j.pop("rate_x%d" % f) for f in range(3)]]
        bw, bh = BLOCK_W[j["bsize"]], BLOCK_H[j["bsize"]]
        n, m = bw * bh, (bw + 7) * (bh + 7)
        case = {"src": src[so:so + n].reshape(bh, bw), "ref": [win[wo:wo + m].reshape(bh + 7, bw + 7), win[wo + m:wo + 2 * m].reshape(bh + 7, bw + 7)], "bd": bd, "jobs": [j]}
        so, wo = so + n, wo + 2 * m
        out.append((case, (o[0], o[1], o[2], list(zip(ev[:o[3]], rd[:o[3]])))))
    assert so == src.size and wo == win.size
    return out


# ------------------------------------------------------------------------------------------------------------------ records <-> ctypes
def c_jobs(pkg, jobs):
    arr = (pkg.IfsJob * max(len(jobs), 1))()
    for a, j in zip(arr, jobs):
        for f in JOB_FIELDS:
            setattr(a, f, j[f])
        for d in range(2):
            for f in range(3):
                a.rate_tab[d][f] = j["rate_tab"][d][f]
    return arr


def result_tuple(r):
    return (r.best, r.interp_filters, r.switchable_rate, r.regular_last, r.rd)


def cand_tuples(c, k):
    return [(c[k * NCAND + i].rate, c[k * NCAND + i].sse, c[k * NCAND + i].dist, c[k * NCAND + i].rd) for i in range(NCAND)]


def fill_words_left(buf, fill):
    """how many aligned 4-byte words of a ctypes array still hold four `fill` bytes"""
    a = np.frombuffer(bytes(buf), np.uint8).reshape(-1, 4)
    return int((a == fill).all(axis=1).sum())


# ------------------------------------------------------------------------------------------------------------------ the refusals
POISON = 0x10   # not NULL, not mapped: a refusal must come before anything is read


def refusals():
    """(name, the job's changes, the arguments' changes): one per rule"""
    return [("null source", {}, {"src": None}), ("null reference 0", {}, {"ref0": None}), ("null jobs", {}, {"jobs": None}), ("null results", {}, {"results": None}),
            ("two references without d_ref1", {"type": 0}, {"ref1": None}), ("a 4-wide size", {"bsize": 1}, {}), ("a 16x4 size", {"bsize": 17}, {}), ("no such size", {"bsize": 22}, {}),
            ("outside on the right", {"x": W - 15}, {}), ("outside below", {"y": H - 15}, {}), ("a negative position", {"x": -1}, {}), ("a phase of 16", {"subpel0_y": 16}, {}),
            ("a phase of 16 on reference 1", {"type": 0, "subpel1_x": 16}, {}), ("type 2", {"type": 2}, {}), ("type -2", {"type": -2}, {}), ("order 2", {"order": 2}, {}),
            ("offsets that sum to 15", {"type": 1, "fwd_offset": 9, "bck_offset": 6}, {}), ("quantizer 0", {"quantizer": 0}, {}), ("quantizer 32768", {"quantizer": 32768}, {}),
            ("12 bits", {}, {"bd": 12}), ("one byte at 10 bits", {}, {"pix_bytes": 1, "bd": 10}), ("four bytes", {}, {"pix_bytes": 4}), ("njobs -1", {}, {"njobs": -1}),
            ("njobs above 2^24", {}, {"njobs": (1 << 24) + 1})]


def refusal_args(pkg, change_job, change_args):
    """the argument list of svt_hip_ifs_search_host for one refusal: every plane and output pointer poisoned, a good job but for `change_job`"""
    j = job(6, 32, 32, ph0=(3, 5), ph1=(1, 2), w=(9, 7))
    j.update(change_job)
    jobs = c_jobs(pkg, [j])
    a = dict(pix_bytes=2, bd=10, src=POISON, src_stride=W, width=W, height=H, ref0=POISON, ref0_stride=W + 7, ref1=POISON, ref1_stride=W + 7, dst=POISON, dst_stride=W,
             jobs=C.cast(jobs, C.c_void_p), njobs=1, results=POISON, cand=POISON)
    a.update(change_args)
    return jobs, [a[k] for k in ("pix_bytes", "bd", "src", "src_stride", "width", "height", "ref0", "ref0_stride", "ref1", "ref1_stride", "dst", "dst_stride", "jobs", "njobs", "results",
                                 "cand")]
