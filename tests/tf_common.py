"""Shared inputs for the temporal-filter tests: the MeContext TF fields of every 64x64 block (OrcTfBlk64 == SvtHipTfBlk64 layout),
synthetic central / motion-compensated pictures, and the reference-test style extremes
(/root/reference/test/TemporalFilterTestPlanewise.cc:200-330: random pixels, random block errors, random noise levels)."""
import ctypes as C

import numpy as np


from conftest import load_package

_pkg = load_package()
TfBlk64, TfRef = _pkg.TfBlk64, _pkg.TfRef
BLK_DTYPE = np.dtype(TfBlk64)
assert BLK_DTYPE.itemsize == C.sizeof(TfBlk64) == 256


def make_blocks(rng, n, bd, big_mv=False, err_max=60):
    b = np.zeros(n, BLK_DTYPE)
    sc = 16 if bd > 8 else 1
    b["err16"] = rng.integers(0, 256 * err_max + 1, (n, 16)) * sc          # mean squared error up to err_max per pixel
    b["err32"] = rng.integers(0, 1024 * err_max + 1, (n, 4)) * sc
    hi = 700 if big_mv else 40
    for k in ("mv16_x", "mv16_y"): b[k] = rng.integers(-hi, hi + 1, (n, 16))
    for k in ("mv32_x", "mv32_y"): b[k] = rng.integers(-hi, hi + 1, (n, 4))
    b["split"] = rng.integers(0, 2, (n, 4))
    if n > 2:
        b["err16"][1] = 0; b["err32"][1] = 0; b["mv16_x"][1] = 0; b["mv16_y"][1] = 0; b["mv32_x"][1] = 0; b["mv32_y"][1] = 0   # perfect match
        b["err16"][2] = np.uint64(1) << np.uint64(40); b["err32"][2] = np.uint64(1) << np.uint64(40)                          # hopeless block
    return b


def plant(plane, mx):
    """all max, all 0, a 0 / max checkerboard and binary 0 / max noise in the top left 64 x 64 block of a plane (in place): what the cases of 8-bit samples in 16-bit
    planes carry"""
    yy, xx = np.mgrid[0:32, 0:32]
    plane[:32, :16] = mx; plane[:32, 16:32] = 0; plane[:32, 32:64] = mx * ((yy + xx) & 1)
    plane[32:64, :32] = mx * np.random.default_rng(9).integers(0, 2, (32, 32))


def make_pictures(rng, w, h, bd, ss_x, ss_y, n_refs, noise=6.0, dtype=None, wide=False):
    """Central picture + n_refs 'motion compensated' pictures (central + noise of varying strength, a few saturated / flat regions).
    dtype: sample type (default uint8 at bd 8, uint16 above); wide: plant() in the central luma plane and, out of step, in every second predictor."""
    dt = dtype or (np.uint8 if bd == 8 else np.uint16)
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    base = (110 + 70 * np.sin(xx / 23.0) * np.cos(yy / 17.0) + 25 * (((xx // 16) + (yy // 16)) % 2)) * (1 << (bd - 8))
    planes = [base, base[::1 << ss_y, ::1 << ss_x] * 0.5 + 60 * (1 << (bd - 8)), 200 * (1 << (bd - 8)) - base[::1 << ss_y, ::1 << ss_x] * 0.4]
    src = [np.ascontiguousarray(np.clip(p + rng.normal(0, 2 * (1 << (bd - 8)), p.shape), 0, mx).astype(dt)) for p in planes]
    src[0][:40, :40] = mx; src[0][40:64, :64] = 0
    preds = []
    for f in range(n_refs):
        sg = noise * (0.3 + f) * (1 << (bd - 8))
        pr = [np.ascontiguousarray(np.clip(s.astype(np.float64) + rng.normal(0, sg, s.shape), 0, mx).astype(dt)) for s in src]
        if f == 0: pr[0][:32, :32] = 0                     # maximum squared differences in one 32x32 block
        if wide and f % 2: plant(pr[0][8:, 8:], mx)
        preds.append(pr)
    if wide: plant(src[0], mx)
    return src, preds


# SvtHipTfSubpelBlk (include/svt_hip.h): one (64x64 block, frame) pair of the TF sub-pel stage
SUBPEL_DTYPE = np.dtype(_pkg.TfSubpelBlk)
assert SUBPEL_DTYPE.itemsize == 100


def mv_word(mx, my):
    """the ME table's vector word: (y << 16) | x, quarter-pel int16 halves of an integer vector"""
    return ((np.asarray(my, np.int64) * 4 & 0xffff) << 16 | (np.asarray(mx, np.int64) * 4 & 0xffff)).astype(np.uint32)


def make_subpel_case(rng, w, h, bd, pad, max_mv=9, noise=3.0, edge_mv=True, dtype=None, wide=False):
    """A central picture and a padded reference picture (the central one shifted by a smooth sub-pel field + noise), 4:2:0, and one job per 64x64 block
    whose integer vectors point near the true motion; blocks on the picture border get vectors that push the clamp of clamp_mv_to_umv_border_sb."""
    dt = dtype or (np.uint8 if bd == 8 else np.uint16)
    mx = (1 << bd) - 1
    sc = 1 << (bd - 8)

    def tex(hh, ww, ox, oy, k):
        yy, xx = np.mgrid[0:hh, 0:ww].astype(np.float64)
        xx = xx + ox; yy = yy + oy
        return (120 + 60 * np.sin(xx / (7.0 + k)) * np.cos(yy / (5.0 + k)) + 30 * np.sin((xx + 2 * yy) / 3.1)) * sc

    src, ref = [], []
    for p in range(3):
        s = 0 if p == 0 else 1
        ww, hh, pd = w >> s, h >> s, pad >> s
        src.append(np.ascontiguousarray(np.clip(tex(hh, ww, 0, 0, p) + rng.normal(0, noise * sc, (hh, ww)), 0, mx).astype(dt)))
        full = np.clip(tex(hh + 2 * pd, ww + 2 * pd, -pd + 2.3 / (1 + s), -pd - 1.6 / (1 + s), p) + rng.normal(0, noise * sc, (hh + 2 * pd, ww + 2 * pd)), 0, mx).astype(dt)
        ref.append(np.ascontiguousarray(full))
    if wide:      # interior blocks (border vectors are pushed to the clamp): the interpolation overshoots the range on the binary regions
        plant(src[0][64:, 64:], mx); plant(ref[0][pad + 64 + 2:, pad + 64 - 3:], mx)
    bc, br = w // 64, h // 64
    jobs = np.zeros(bc * br, SUBPEL_DTYPE)
    for r in range(br):
        for c in range(bc):
            j = jobs[r * bc + c]
            j["x"], j["y"], j["dst_x"], j["dst_y"], j["blk_index"] = c * 64, r * 64, c * 64, r * 64, r * bc + c
            m32x = rng.integers(-max_mv, max_mv + 1, 4); m32y = rng.integers(-max_mv, max_mv + 1, 4)
            m16x = rng.integers(-max_mv, max_mv + 1, 16); m16y = rng.integers(-max_mv, max_mv + 1, 16)
            if edge_mv and (r == 0 or c == 0 or r == br - 1 or c == bc - 1):   # far outside the picture: the clamp decides
                far = pad - 8
                m32x[:] = -far if c == 0 else (far if c == bc - 1 else m32x); m32y[:] = -far if r == 0 else (far if r == br - 1 else m32y)
                m16x[:8] = m32x[0]; m16y[:8] = m32y[0]
            j["mv32"] = mv_word(m32x, m32y); j["mv16"] = mv_word(m16x, m16y)
    return src, ref, jobs


# =====================================================================================================================================
# Edge cases of the three temporal-filter kernels: wraps, ties and plane edges.  tests/test_tf_ref_cpu.py proves on the CPU what each case
# contains and checks the oracle against the plain restatements below; tests/test_tf_gpu.py runs the same cases on the device.
# =====================================================================================================================================
import math
import struct

FILTER_FMTS = ((np.uint8, 8), (np.uint16, 8), (np.uint16, 9), (np.uint16, 10), (np.uint16, 11), (np.uint16, 12))
NOISE_FMTS = ((np.uint8, 8), (np.uint16, 8), (np.uint16, 10), (np.uint16, 12))
SUBPEL_FMTS = ((np.uint8, 8), (np.uint16, 8), (np.uint16, 10))
P3, I3 = C.c_void_p * 3, C.c_int * 3


def fmt_id(f):
    return "u%d-%d" % (8 * np.dtype(f[0]).itemsize, f[1])


def sentinel(dt):
    """what the padding of every plane is pre-filled with; no 16-bit sample of any depth can equal it"""
    return 0xA5 if np.dtype(dt).itemsize == 1 else 0xA5A5


def padded(content, stride, dt, rows_after=0):
    """content in an allocation of its own with row stride `stride` (> width), the padding pre-filled with the sentinel"""
    h, w = content.shape
    assert stride > w
    buf = np.full((h + rows_after, stride), sentinel(dt), dt)
    buf[:h, :w] = content
    return buf


_libm = C.CDLL("libm.so.6")
for _n in ("expf", "powf", "sqrtf"):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float] * (2 if _n == "powf" else 1)


def libm_expf(x):
    """the host libm's expf -- the function the reference and the oracle call -- on a float32 array"""
    x = np.asarray(x, np.float32)
    u, inv = np.unique(x, return_inverse=True)
    return np.array([_libm.expf(float(v)) for v in u], np.float32)[inv].reshape(x.shape)


def recip_ok(y):
    """tfilter.hip's host-side test of a launch constant: positive, exponent field inside 524 .. 1522, significand not all ones"""
    b = struct.unpack("<Q", struct.pack("<d", y))[0]
    ex = (b >> 52) & 0x7ff
    return (b >> 63) == 0 and 523 < ex < 1523 and (b & 0xFFFFFFFFFFFFF) != 0xFFFFFFFFFFFFF


def launch_constants(noise, decay, mfs):
    """(2 n_decay^2 per plane, distance threshold) as svt_hip_tf_filter_frame_dev computes them"""
    den = []
    for p in range(3):
        n_decay = float(decay) * (0.7 + (math.log1p(noise[p]) if noise[p] > -1.0 else -math.inf))
        den.append(2 * n_decay * n_decay)
    thr = mfs * 0.1
    return den, (thr if thr > 1 else 1.0)


# ------------------------------------------------------------------------------------------------------------------------ the filter
def edge_blocks(n, k):
    """Block records of window frame k for n 64x64 blocks: both split values in every record, vectors 0, (+-32767, +-32767) and (-32768, -32768), errors 0, 1,
    15 (0 after the 16-bit path's >> 4), 2^40 and 2^63.  The fields a quadrant's split value makes unused hold values that would change the picture if they were read."""
    b = np.zeros(n, BLK_DTYPE)
    quads = [
        dict(split=0, err32=0, mv32=(0, 0), err16=[1 << 63] * 4, mv16=[(32767, 32767)] * 4),
        dict(split=1, err32=1 << 63, mv32=(32767, 32767), err16=[1, 15, 1 << 40, 1 << 63], mv16=[(0, 0), (32767, -32767), (3, -4), (-32768, -32768)]),
        dict(split=0, err32=15, mv32=(-32767, 32767), err16=[0] * 4, mv16=[(0, 0)] * 4),
        dict(split=1, err32=0, mv32=(0, 0), err16=[0, 16, 4800, 1 << 40], mv16=[(0, 0), (5, 12), (-40, 9), (700, -700)]),
    ]
    for i in range(n):
        for q in range(4):
            r = quads[(q + k + 2 * i) % 4]
            b["split"][i, q] = r["split"] ^ (i & 1 & (q >> 1)); b["err32"][i, q] = r["err32"]; b["mv32_x"][i, q], b["mv32_y"][i, q] = r["mv32"]
            for s in range(4):
                b["err16"][i, 4 * q + s] = r["err16"][s]; b["mv16_x"][i, 4 * q + s], b["mv16_y"][i, 4 * q + s] = r["mv16"][s]
    return b


def _content(name, rng, h, w, mx, plane, sh, cw=32, ch=32):
    """(central, predictor) content `name` of one plane, int64; (cw, ch) = the size of the plane's share of a 32x32 luma block"""
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "max_vs_0": return np.full((h, w), mx), np.zeros((h, w), np.int64)
    if name == "0_vs_max": return np.zeros((h, w), np.int64), np.full((h, w), mx)
    if name == "checker": s = mx * ((yy + xx) & 1); return s, mx - s
    if name == "binary": return mx * rng.integers(0, 2, (h, w)), mx * rng.integers(0, 2, (h, w))
    s = np.clip((mx // 2) + rng.integers(-6 << sh, (6 << sh) + 1, (h, w)), 0, mx)
    d = rng.integers(1, (24 << sh) + 1, (h, w)) * rng.choice([-1, 1], (h, w))
    if name == "border":        # squared differences only in the 2-sample border of every block, where the 5x5 window's clamp binds
        ring = (yy % ch < 2) | (yy % ch >= ch - 2) | (xx % cw < 2) | (xx % cw >= cw - 2)
        return s, np.clip(s + d * ring, 0, mx)
    if name == "luma_only":     # chroma identical, luma not: the chroma weights move with the co-located luma samples alone
        return s, (np.clip(s + d, 0, mx) if plane == 0 else s.copy())
    raise KeyError(name)


class FilterCase:
    """One picture, its window and everything svt_hip_tf_filter_frame_dev / orc_tf_filter_frame take.  Window: the content's predictor, a copy of the central picture
    (weight 1000 wherever the block record has error 0 and no motion), a near copy (weights in between) and the central picture itself at slot `center`."""

    def __init__(self, name, content, dt, bd, w, h, ss, tf_chroma, decay, mfs, center, noise=(1.7, 0.9, 2.4), seed=1, window=("content", "same", "near")):
        self.name, self.dt, self.bd, self.w, self.h, (self.ss_x, self.ss_y) = name, np.dtype(dt).type, bd, w, h, ss
        self.tf_chroma, self.decay, self.mfs, self.center, self.noise = tf_chroma, decay, mfs, center, np.asarray(noise, np.float64)
        rng = np.random.default_rng(seed)
        mx, sh = (1 << bd) - 1, bd - 8
        self.dims = [(h, w), (h >> ss[1], w >> ss[0]), (h >> ss[1], w >> ss[0])]
        k = [0]

        def alloc(a):    # every plane of every role: an allocation of its own, a stride of its own (odd and even ones), wider than the plane
            k[0] += 1
            return padded(a.astype(dt), a.shape[1] + 2 + k[0], dt)
        pairs = [_content(content, rng, hh, ww, mx, p, sh, 32 >> (ss[0] if p else 0), 32 >> (ss[1] if p else 0)) for p, (hh, ww) in enumerate(self.dims)]
        self.src = [alloc(s) for s, _ in pairs]
        self.dst = [alloc(np.full(d, sentinel(dt) & mx)) for d in self.dims]
        self.preds = []
        for kind in window:
            if kind == "content": pl = [q for _, q in pairs]
            elif kind == "same": pl = [s for s, _ in pairs]
            else: pl = [np.clip(s + rng.integers(-5 << sh, (5 << sh) + 1, s.shape), 0, mx) for s, _ in pairs]
            self.preds.append([alloc(q) for q in pl])
        self.blocks = [edge_blocks((w // 64) * (h // 64), f) for f in range(len(window))]
        self.n_refs = len(window) + 1
        strides = [b.shape[1] for b in self.src + self.dst + [q for pr in self.preds for q in pr]]
        assert len(set(strides)) == len(strides) and any(s & 1 for s in strides)

    def order(self):
        """window slot -> predictor index, None for the central picture"""
        o = list(range(len(self.preds))); o.insert(self.center, None)
        return o

    def refs(self, struct_t, pred_ptr, blk_ptr):
        r = (struct_t * self.n_refs)()
        for f, k in enumerate(self.order()):
            if k is None: r[f].blocks = None; continue
            for p in range(3):
                r[f].pred[p] = pred_ptr(k, p); r[f].pred_stride[p] = self.preds[k][p].shape[1]
            r[f].blocks = blk_ptr(k)
        return r

    def planes(self):
        return 3 if self.tf_chroma else 1

    def oracle(self, orc, in_place=False):
        """(destination planes with their padding, sse) of orc_tf_filter_frame; in place, the destination is a copy of the central picture with its strides"""
        src = [b.copy() for b in self.src]
        dst = src if in_place else [b.copy() for b in self.dst]
        refs = self.refs(TfRef, lambda k, p: self.preds[k][p].ctypes.data, lambda k: self.blocks[k].ctypes.data)
        sse = np.zeros(2, np.uint64)
        orc.orc_tf_filter_frame(src[0].itemsize, self.bd, P3(*[b.ctypes.data for b in src]), I3(*[b.shape[1] for b in src]), P3(*[b.ctypes.data for b in dst]),
                                I3(*[b.shape[1] for b in dst]), self.w, self.h, self.ss_x, self.ss_y, self.tf_chroma, refs, self.n_refs,
                                self.noise.ctypes.data_as(C.c_void_p), self.decay, self.mfs, sse.ctypes.data_as(C.c_void_p))
        return dst, sse

    def view(self, bufs, p):
        return bufs[p][:self.dims[p][0], :self.dims[p][1]]


def filter_edge_cases(fmt):
    dt, bd = fmt
    T = [  # name, content, w, h, (ss_x, ss_y), tf_chroma, decay, min_frame_size, slot of the central picture
        ("max_vs_0", "max_vs_0", 64, 64, (1, 1), 1, 4, 64, 1),
        ("0_vs_max", "0_vs_max", 64, 64, (0, 0), 1, 1, 1, 0),
        ("checker", "checker", 64, 64, (1, 0), 1, 4, 2160, 3),
        ("binary", "binary", 64, 64, (1, 1), 0, 1, 2160, 2),
        ("border", "border", 64, 64, (0, 0), 1, 4, 1, 1),
        ("luma_only", "luma_only", 64, 64, (1, 0), 1, 1, 64, 0),
        ("border_420", "border", 64, 64, (1, 1), 1, 1, 64, 2),
        ("two_columns", "binary", 128, 64, (1, 1), 1, 4, 1, 2),
    ]
    return [FilterCase(n, c, dt, bd, w, h, ss, ch, dec, mfs, ctr, seed=10 + i) for i, (n, c, w, h, ss, ch, dec, mfs, ctr) in enumerate(T)]


def slow_division_case(fmt, v_noise=-1.0):
    """V-plane noise level -1: log1p(-1) = -inf, 2 n_decay^2 = +inf, which recip_ok refuses, so the whole launch takes the IEEE-division instance; every V weight is 1000.
    v_noise = 2.4 gives the same pictures to the three-operation instance."""
    dt, bd = fmt
    return FilterCase("slow_division", "luma_only", dt, bd, 64, 64, (1, 1), 1, 4, 64, 1, noise=(1.7, 0.9, v_noise), seed=77, window=("content", "near", "near"))


def rounded_mean_of_window(case, p):
    """the filtered plane when every weight is 1000: (1000 S + 500 n) // (1000 n) = (S + n // 2) // n for even n, floor(S / n + 1 / 2) in general"""
    n = case.n_refs
    s = case.view(case.src, p).astype(np.int64) + sum(case.view(pr, p).astype(np.int64) for pr in case.preds)
    return (1000 * s + 500 * n) // (1000 * n)


def _box5(d):
    """5x5 sums of a block with the window clamped to the block"""
    e = np.pad(d, 2, mode="edge")
    h, w = d.shape
    return sum(e[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5))


def numpy_filter(case, weights_out=None):
    """Plain restatement of the plane-wise filter on a FilterCase: float64 as the reference writes it (EbTemporalFiltering.c:643-813), powf / sqrtf / expf from the
    host's libm.  -> (filtered planes, sse).  weights_out (a set per plane) collects every weight."""
    c = case
    den, thr = launch_constants(c.noise, c.decay, c.mfs)
    hbd = c.src[0].itemsize == 2
    sq = (c.bd - 8) * 2 if hbd else 0
    S = [c.view(c.src, p).astype(np.int64) for p in range(3)]
    acc = [1000 * s for s in S]; cnt = [np.full(s.shape, 1000, np.int64) for s in S]
    cw, ch = 32 >> c.ss_x, 32 >> c.ss_y
    bc = c.w // 64
    for k, pr in enumerate(c.preds):
        Pp = [c.view(pr, p).astype(np.int64) for p in range(3)]
        for by in range(c.h // 32):
            for bx in range(c.w // 32):
                rec = c.blocks[k][(by >> 1) * bc + (bx >> 1)]
                idx32 = (bx & 1) + (by & 1) * 2
                be, df = np.zeros(4), np.zeros(4)
                for sub in range(4):
                    if rec["split"][idx32]: err, mvx, mvy, div = int(rec["err16"][idx32 * 4 + sub]), int(rec["mv16_x"][idx32 * 4 + sub]), int(rec["mv16_y"][idx32 * 4 + sub]), 256.0
                    else: err, mvx, mvy, div = int(rec["err32"][idx32]), int(rec["mv32_x"][idx32]), int(rec["mv32_y"][idx32]), 1024.0
                    if hbd: err >>= 4
                    be[sub] = float(err) / div
                    dist = _libm.sqrtf(float(np.float32(_libm.powf(float(mvy), 2.0)) + np.float32(_libm.powf(float(mvx), 2.0))))
                    df[sub] = max(float(dist) / thr, 1.0)
                ys, xs = slice(by * 32, by * 32 + 32), slice(bx * 32, bx * 32 + 32)
                yd = (S[0][ys, xs] - Pp[0][ys, xs]) ** 2
                ii, jj = np.mgrid[0:32, 0:32]
                sub = (ii >= 16) * 2 + (jj >= 16)

                def weight(sums, num, sub, d):
                    with np.errstate(all="ignore"):
                        combined = (5 * (sums.astype(np.float64) / num) + be[sub]) / 6
                        scaled = combined * df[sub] / d
                    scaled = np.where(scaled < 7, scaled, 7.0)
                    return (libm_expf((-scaled).astype(np.float32)) * np.float32(1000)).astype(np.int64)
                wy = weight(_box5(yd) >> sq, 25, sub, den[0])
                acc[0][ys, xs] += wy * Pp[0][ys, xs]; cnt[0][ys, xs] += wy
                if weights_out is not None: weights_out[0].update(np.unique(wy).tolist())
                if not c.tf_chroma: continue
                cys, cxs = slice(by * ch, by * ch + ch), slice(bx * cw, bx * cw + cw)
                ysum = sum(yd[dy::1 << c.ss_y, dx::1 << c.ss_x] for dy in range(1 << c.ss_y) for dx in range(1 << c.ss_x))
                csub = sub[::1 << c.ss_y, ::1 << c.ss_x]
                for p in (1, 2):
                    cd = (S[p][cys, cxs] - Pp[p][cys, cxs]) ** 2
                    wc = weight((ysum + _box5(cd)) >> sq, 25 + (1 << c.ss_x) * (1 << c.ss_y), csub, den[p])
                    acc[p][cys, cxs] += wc * Pp[p][cys, cxs]; cnt[p][cys, cxs] += wc
                    if weights_out is not None: weights_out[p].update(np.unique(wc).tolist())
    assert max(int(a.max()) for a in acc) < 1 << 32 and max(int(n.max()) for n in cnt) < 1 << 16       # neither the accumulator nor the counter can wrap in a window this short
    out = [(a + (n >> 1)) // n for a, n in zip(acc, cnt)]
    sse = [int(((S[0] - out[0]) ** 2).sum()), int(sum(((S[p] - out[p]) ** 2).sum() for p in (1, 2))) if c.tf_chroma else 0]
    return out[:c.planes()], np.array(sse, np.uint64)


# ------------------------------------------------------------------------------------------------------------------------ the noise estimate
def numpy_noise(img, bd, smooth=lambda ga: ga < 50):
    """(Laplacian sum, smooth-sample count) of estimate_noise(_highbd) on a 2-D array of samples; 16-bit samples round both magnitudes to the 8-bit scale.  smooth: the
    edge test, replaceable to show that a case notices another one"""
    a = img.astype(np.int64)
    sh = bd - 8 if img.itemsize == 2 else 0
    rnd = (1 << sh) >> 1
    h, w = a.shape
    if h < 3 or w < 3: return 0, 0
    n = lambda dy, dx: a[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    gx = (n(-1, -1) - n(-1, 1)) + (n(1, -1) - n(1, 1)) + 2 * (n(0, -1) - n(0, 1))
    gy = (n(-1, -1) - n(1, -1)) + (n(-1, 1) - n(1, 1)) + 2 * (n(-1, 0) - n(1, 0))
    ga = (np.abs(gx) + np.abs(gy) + rnd) >> sh
    v = 4 * n(0, 0) - 2 * (n(0, -1) + n(0, 1) + n(-1, 0) + n(1, 0)) + (n(-1, -1) + n(-1, 1) + n(1, -1) + n(1, 1))
    lap = (np.abs(v) + rnd) >> sh
    return int(lap[smooth(ga)].sum()), int(smooth(ga).sum())


def sigma_of(s, n):
    return -1.0 if n < 16 else float(s) / (6 * n) * 1.25331413732


def ga_pair(bd, dt):
    """The two raw gradient magnitudes on either side of the edge threshold, as top-left sample values m of an otherwise empty 3x3 patch (gx = gy = m, magnitude 2 m).
    gx + gy = 2 (a - k) + ..., so the raw magnitude |gx| + |gy| is always EVEN: 49 at 8 bits, (49 << sh) + rnd - 1 above, are odd and no picture produces them.  The
    pair is the largest reachable magnitude that is still smooth and the smallest that is not: 48 / 50 at 8 bits, 196 / 198 at 10, 790 / 792 at 12 (49 and 50 after rounding)."""
    sh = bd - 8 if np.dtype(dt).itemsize == 2 else 0
    rnd = (1 << sh) >> 1
    at = (50 << sh) - rnd                 # the smallest raw magnitude that rounds to 50; even
    assert at % 2 == 0 and (at + rnd) >> sh == 50 and (at - 2 + rnd) >> sh == (49 if sh else 48)
    return (at - 2) // 2, at // 2


def noise_edge_cases(fmt):
    """[(name, plane with a stride wider than its width, width, height, closed form (sum, count) or None)]"""
    dt, bd = fmt
    mx = (1 << bd) - 1
    sh = bd - 8 if np.dtype(dt).itemsize == 2 else 0
    rnd = (1 << sh) >> 1
    rng = np.random.default_rng(31 + bd)
    out = []

    def add(name, a, closed=None):
        a = np.asarray(a)
        out.append((name, padded(a.astype(dt), a.shape[1] + 5 + len(out), dt), a.shape[1], a.shape[0], closed))
    smooth = lambda h, w: np.clip(((100 + 30 * np.sin(np.arange(w) / 11.0)[None, :] + rng.normal(0, 1.5, (h, w))) * (1 << (bd - 8))), 0, mx)
    add("rows_past_2048", smooth(2100, 24))
    add("2x2", smooth(2, 2), (0, 0)); add("3x3", smooth(3, 3)); add("2x40", smooth(40, 2), (0, 0)); add("40x2", smooth(2, 40), (0, 0))
    add("flat_17x3", np.full((3, 17), mx // 3), (0, 15)); add("flat_18x3", np.full((3, 18), mx // 3), (0, 16))
    add("259x5", smooth(5, 259)); add("261x5", smooth(5, 261))
    lo, hi = ga_pair(bd, dt)
    for name, m in (("ga_smooth", lo), ("ga_edge", hi)):
        a = np.zeros((3, 3), np.int64); a[0, 0] = m
        add(name, a, ((m + rnd) >> sh, 1) if m == lo else (0, 0))      # the Laplacian of the patch is the sample itself
    strip = np.zeros((3, 32), np.int64); strip[0, 3::8] = [lo, hi, hi, lo]
    add("ga_strip", strip)
    yy, xx = np.mgrid[0:21, 0:37]
    add("checker", mx * ((yy + xx) & 1), (((8 * mx + rnd) >> sh) * 35 * 19, 35 * 19))
    return out


# ------------------------------------------------------------------------------------------------------------------------ the sub-pel stage
def i16(v):
    return ((int(v) + 32768) & 0xffff) - 32768


def i32(v):
    return ((int(v) + (1 << 31)) & 0xffffffff) - (1 << 31)


def qpel_word(qx, qy):
    """the ME table's vector word from quarter-pel int16 halves"""
    return np.uint32(((qy & 0xffff) << 16) | (qx & 0xffff))


def variance_u8(sse, s, n):
    """svt_aom_variance{W}x{H}_c: sse - (int64) sum^2 / n"""
    return (sse - (s * s) // n) & 0xffffffff


def variance_u16(sse, s, n, wide=False):
    """variance_highbd_c: `sad * sad` is an int product (two's-complement wrap, as the compiled C does), divided as an int (truncating), subtracted in uint32_t.
    wide = the 64-bit arithmetic it does NOT have."""
    if wide: return (sse - (s * s) // n) & 0xffffffff
    p = i32((s * s) & 0xffffffff)
    q = abs(p) // n * (1 if p >= 0 else -1)
    return (sse - q) & 0xffffffff


def split_flag(err32, err16, wide=False):
    """derive_tf_32x32_block_split_flag in int arithmetic with two's-complement wrap; wide = the arithmetic it does not have"""
    w = (lambda v: v) if wide else i32
    be = w(err32); e = [w(x) for x in err16]
    s = 0
    for x in e: s = w(s + x)
    b15, b14, s16 = w(be * 15), w(be * 14), w(s * 16)
    d = max(e) - min(e)
    return 0 if ((b15 < s16 and d < 12000) or (b14 < s16 and d < 6000)) else 1


class SubpelCase:
    """Central picture (a crop: picture sample (X, Y) sits at plane sample (X + ox, Y + oy)), padded reference, predictor planes with the crop's origin, all with
    different strides; jobs with a permuted, sparse blk_index into a pre-filled block array."""
    OX, OY = 8, 16        # multiples of 8: the chroma origin is ((lx >> 3) << 3) / 2

    def __init__(self, name, dt, bd, w, h, src, ref, jobs, th16, tf_hp, tf_chroma, pad=64):
        """src: 3 picture-sized arrays; ref: 3 arrays with `pad` (luma) / pad / 2 (chroma) samples around the picture; jobs: [(x, y, blk_index, mv32 words, mv16 words)]"""
        self.name, self.dt, self.bd, self.w, self.h, self.pad = name, np.dtype(dt).type, bd, w, h, pad
        self.th16, self.tf_hp, self.tf_chroma = th16, tf_hp, tf_chroma
        mx = (1 << bd) - 1
        self.org = [(self.OX, self.OY), (self.OX // 2, self.OY // 2), (self.OX // 2, self.OY // 2)]
        self.pads = [pad, pad // 2, pad // 2]
        self.src, self.pred, self.ref = [], [], []
        for p in range(3):
            ox, oy = self.org[p]
            hh, ww = src[p].shape
            a = np.full((hh + oy, ww + ox), sentinel(dt) & mx, np.int64); a[oy:, ox:] = src[p]
            self.src.append(padded(a.astype(dt), ww + ox + 3 + p, dt, rows_after=2))
            self.pred.append(np.full((hh + oy + 2, ww + ox + 10 + p), sentinel(dt), dt))
            assert ref[p].shape == (hh + 2 * self.pads[p], ww + 2 * self.pads[p])
            self.ref.append(padded(np.asarray(ref[p]).astype(dt), ref[p].shape[1] + 17 + p, dt))
        self.jobs = np.zeros(len(jobs), SUBPEL_DTYPE)
        for j, (x, y, bi, m32, m16) in zip(self.jobs, jobs):
            j["x"], j["y"], j["dst_x"], j["dst_y"], j["blk_index"] = x, y, x + self.OX, y + self.OY, bi
            j["mv32"] = m32; j["mv16"] = m16
        self.n_blocks = max(j[2] for j in jobs) + 3
        assert len({j[2] for j in jobs}) == len(jobs) and (len(jobs) == 1 or [j[2] for j in jobs] != sorted(j[2] for j in jobs))   # permuted, and sparse by the three spare records
        self.blocks0 = np.frombuffer(bytes([0x5A]) * (256 * self.n_blocks), BLK_DTYPE).copy()
        s = [self.src[0].shape[1], self.pred[0].shape[1], self.ref[0].shape[1]]
        assert len(set(s)) == 3

    def ref_offset(self, p):
        """bytes from the reference allocation to picture sample (0, 0)"""
        return (self.pads[p] * self.ref[p].shape[1] + self.pads[p]) * self.ref[p].itemsize

    def with_th16(self, th16):
        c = SubpelCase.__new__(SubpelCase); c.__dict__.update(self.__dict__); c.th16 = th16
        return c

    def oracle(self, orc):
        """(block array, predictor planes) of orc_tf_subpel_frame"""
        pb = self.src[0].itemsize
        pred = [b.copy() for b in self.pred]; blk = self.blocks0.copy()
        orc.orc_tf_subpel_frame.argtypes = [C.c_int, C.c_int, P3, I3, P3, I3, P3, I3, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        orc.orc_tf_subpel_frame(pb, self.bd, P3(*[b.ctypes.data for b in self.src]), I3(*[b.shape[1] for b in self.src]),
                                P3(*[self.ref[p].ctypes.data + self.ref_offset(p) for p in range(3)]), I3(*[b.shape[1] for b in self.ref]),
                                P3(*[b.ctypes.data for b in pred]), I3(*[b.shape[1] for b in pred]), self.w // 4, self.h // 4, self.th16, self.tf_hp, self.tf_chroma,
                                self.jobs.ctypes.data, len(self.jobs), blk.ctypes.data)
        return blk, pred


def python_subpel(orc, case, probe=None, mutate=()):
    """The sub-pel stage's control flow in Python over the oracle's orc_convolve_sr for each prediction: nine candidates per round, i (x) outer, j (y) inner, the first
    strictly smaller distortion wins; the 8-bit variance in 64 bits, the 16-bit one with its 32-bit wrap; the threshold; the split decision with its wrap; the final
    MULTITAP_SHARP predictions.  -> (block array, predictor planes).  Every prediction's reads -- with the margin of the device's shared window -- are asserted to lie
    inside the reference allocation.  probe (a dict) receives: "round0" [(bs, quadrant or 16x16 index, nine distortions)], "split" [(err32, err16, wrapped, wide)],
    "dist_wide" (whether 64-bit variance arithmetic would have changed any distortion), "clamps" {branch: [below 0 seen, above max seen]}.
    mutate: names of deliberate mistakes ("scan_le": `<=` in the candidate scan, "th_le": `err32 <= th16` skips the 16x16 rounds), for showing that a case notices them."""
    c = case
    pb, bd, mx = c.src[0].itemsize, c.bd, (1 << c.bd) - 1
    mi_cols, mi_rows = c.w // 4, c.h // 4
    pred = [b.copy() for b in c.pred]; blk = c.blocks0.copy()
    taps = np.ctypeslib.as_array((C.c_int16 * 8 * 16 * 6).in_dll(orc, "orc_interp_kernels")).astype(np.int64)
    if probe is not None: probe.update(round0=[], split=[], dist_wide=False, clamps={"x": [False, False], "y": [False, False], "xy": [False, False]})
    rp2 = lambda v, n: (v + (1 << (n - 1))) >> n

    def params(mvx, mvy, px, py, bs, bw, ss, pre_x, pre_y):
        micol, mirow, mi = px >> 2, py >> 2, bs >> 2
        to_left, to_right, to_top, to_bottom = -(micol * 32), (mi_cols - mi - micol) * 32, -(mirow * 32), (mi_rows - mi - mirow) * 32
        sl, st = (4 + bw) << 4, (4 + bw) << 4
        m = 1 << (1 - ss)
        col, row = i16(mvx * m), i16(mvy * m)
        col = i16(min(max(col, to_left * m - sl), to_right * m + sl - 16)); row = i16(min(max(row, to_top * m - st), to_bottom * m + st - 16))
        return ((pre_x << 4) + col) >> 4, ((pre_y << 4) + row) >> 4, col & 15, row & 15

    def predict(p, pos_x, pos_y, sx, sy, bank, bw, out, out_stride_elems, out_off_elems):
        R, pd = c.ref[p], c.pads[p]
        ww, hh = c.w >> (p > 0), c.h >> (p > 0)
        # the furthest read: 3 / 4 taps around the block, and up to two more samples for the window the device's nine candidates share
        assert -pd <= pos_x - 6 and pos_x + bw + 6 <= ww + pd and -pd <= pos_y - 6 and pos_y + bw + 6 <= hh + pd, (c.name, p, pos_x, pos_y, bw)
        orc.orc_convolve_sr(C.c_void_p(R.ctypes.data + ((pos_y + pd) * R.shape[1] + pos_x + pd) * pb), R.shape[1], C.c_void_p(out.ctypes.data + out_off_elems * pb),
                            out_stride_elems, pb, bw, bw, bank, bank, sx, sy, bd)
        if probe is not None and (sx or sy):
            W = R[pos_y + pd - 3:pos_y + pd + bw + 4, pos_x + pd - 3:pos_x + pd + bw + 4].astype(np.int64)
            xf, yf = taps[bank][sx], taps[bank][sy]
            if sy == 0: v = rp2(rp2(sum(xf[k] * W[3:3 + bw, k:k + bw] for k in range(8)), 3), 4); br = "x"
            elif sx == 0: v = rp2(sum(yf[k] * W[k:k + bw, 3:3 + bw] for k in range(8)), 7); br = "y"
            else:
                im = rp2(sum(xf[k] * W[:, k:k + bw] for k in range(8)) + (1 << (bd + 6)), 3)
                assert im.min() >= -32768 and im.max() <= 32767       # the 16-bit intermediate holds
                probe["im_max"] = max(probe.get("im_max", 0), int(np.abs(im).max()))
                v = rp2(sum(yf[k] * im[k:k + bw] for k in range(8)) + (1 << (bd + 11)), 11) - ((1 << bd) + (1 << (bd - 1))); br = "xy"
            probe["clamps"][br][0] |= bool((v < 0).any()); probe["clamps"][br][1] |= bool((v > mx).any())
            flat = out.reshape(-1)
            got = np.stack([flat[out_off_elems + r * out_stride_elems:out_off_elems + r * out_stride_elems + bw] for r in range(bw)])
            assert np.array_equal(got, np.clip(v, 0, mx)), (c.name, br)

    def search(bs, px, py, word, tag):
        n = bs * bs
        lx, ly = px + c.OX, py + c.OY
        s = c.src[0][ly:ly + bs, lx:lx + bs].astype(np.int64)
        mv_x, mv_y = i16(i16(int(word) & 0xffff) * 2), i16(i16(int(word) >> 16) * 2)
        bx, by, best = mv_x, mv_y, 0x7fffffff
        tmp = np.zeros((bs, bs), c.dt)
        for rnd in range(3 if c.tf_hp else 2):
            step = 4 >> rnd
            dists = []
            for i in (-step, 0, step):
                for j in (-step, 0, step):
                    cx, cy = i16(mv_x + i), i16(mv_y + j)
                    pos_x, pos_y, sx, sy = params(cx, cy, px, py, bs, bs, 0, px, py)
                    predict(0, pos_x, pos_y, sx, sy, 0, bs, tmp, bs, 0)
                    d = tmp.astype(np.int64) - s
                    sse, sm = int((d * d).sum()), int(d.sum())
                    dist = variance_u8(sse, sm, n) if pb == 1 else variance_u16(sse, sm, n)
                    if probe is not None and pb == 2 and dist != variance_u16(sse, sm, n, wide=True): probe["dist_wide"] = True
                    dists.append(dist)
                    if dist < best or ("scan_le" in mutate and dist == best): best, bx, by = dist, cx, cy
            if probe is not None and rnd == 0: probe["round0"].append((bs, tag, dists))
            mv_x, mv_y = bx, by
        return bx, by, best

    def final(bs, px, py, mvx, mvy):
        lx, ly = px + c.OX, py + c.OY
        pos_x, pos_y, sx, sy = params(mvx, mvy, px, py, bs, bs, 0, px, py)
        predict(0, pos_x, pos_y, sx, sy, 2, bs, pred[0], pred[0].shape[1], ly * pred[0].shape[1] + lx)
        if not c.tf_chroma: return
        cb, cpx, cpy, clx, cly = bs >> 1, ((px >> 3) << 3) // 2, ((py >> 3) << 3) // 2, ((lx >> 3) << 3) // 2, ((ly >> 3) << 3) // 2
        pos_x, pos_y, sx, sy = params(mvx, mvy, px, py, bs, cb, 1, cpx, cpy)
        for p in (1, 2):
            predict(p, pos_x, pos_y, sx, sy, 2, cb, pred[p], pred[p].shape[1], cly * pred[p].shape[1] + clx)

    for J in c.jobs:
        B = blk[J["blk_index"]]
        for q in range(4):
            qx, qy = int(J["x"]) + 32 * (q & 1), int(J["y"]) + 32 * (q >> 1)
            m32x, m32y, e32 = search(32, qx, qy, J["mv32"][q], q)
            B["mv32_x"][q], B["mv32_y"][q], B["err32"][q] = m32x, m32y, e32
            offs = [(qx + 16 * (k & 1), qy + 16 * (k >> 1)) for k in range(4)]
            m16, e16 = [(0, 0)] * 4, [0] * 4
            split = 0
            if not (e32 < c.th16 or ("th_le" in mutate and e32 == c.th16)):
                for k in range(4):
                    x16, y16, e16[k] = search(16, offs[k][0], offs[k][1], J["mv16"][4 * q + k], 4 * q + k)
                    m16[k] = (x16, y16)
                split = split_flag(e32, e16)
                if probe is not None: probe["split"].append((e32, list(e16), split, split_flag(e32, e16, wide=True)))
            for k in range(4):
                B["mv16_x"][4 * q + k], B["mv16_y"][4 * q + k] = m16[k]; B["err16"][4 * q + k] = e16[k]
            B["split"][q] = split
            if split:
                for k in range(4): final(16, offs[k][0], offs[k][1], m16[k][0], m16[k][1])
            else: final(32, qx, qy, m32x, m32y)
    return blk, pred


# distortion of a flat block of 0 against a flat prediction of max (or the inverse): (32x32, 16x16) per format.  The 8-bit variance is computed in 64 bits and is 0; the
# 16-bit one wraps in 32 bits, so the (u16, 8) result is NOT the widened (u8, 8) result on such content.
FLAT_DIST = {(1, 8): (0, 0), (2, 8): (1 << 26, 1 << 24), (2, 10): (1 << 30, 1 << 28)}


def _sp_planes(w, h, pad, f_src, f_ref):
    """three picture planes and three padded reference planes from functions of (plane, X, Y) in the plane's own picture coordinates"""
    src, ref = [], []
    for p in range(3):
        s = p > 0
        ww, hh, pd = w >> s, h >> s, pad >> s
        yy, xx = np.mgrid[0:hh, 0:ww]
        src.append(np.asarray(f_src(p, xx, yy), np.int64))
        yy, xx = np.mgrid[-pd:hh + pd, -pd:ww + pd]
        ref.append(np.asarray(f_ref(p, xx, yy), np.int64))
    return src, ref


def subpel_edge_cases(fmt):
    """{name: SubpelCase}; case.expect, where present, holds the closed forms: the offset of every chosen vector from its start vector (1/8 pel) and the distortions"""
    dt, bd = fmt
    pb = np.dtype(dt).itemsize
    mx, sc = (1 << bd) - 1, 1 << (bd - 8)
    rng = np.random.default_rng(100 + bd + pb)
    full = lambda v: (lambda p, xx, yy: np.full(xx.shape, v))
    words = lambda n: np.array([qpel_word(int(a), int(b)) for a, b in rng.integers(-24, 25, (n, 2))], np.uint32)
    z4, z16 = np.zeros(4, np.uint32), np.zeros(16, np.uint32)
    cases = {}

    def add(name, w, h, planes, jobs, th16, tf_hp, tf_chroma, expect=None):
        cases[name] = SubpelCase(name, dt, bd, w, h, planes[0], planes[1], jobs, th16, tf_hp, tf_chroma)
        cases[name].expect = expect
    # split: 15 err32 < 16 sum(err16) holds for the 16-bit distortions (15 < 16) and not for the 8-bit ones (0 < 0)
    tie = dict(offset=(-4, -4), err32=FLAT_DIST[(pb, bd)][0], err16=FLAT_DIST[(pb, bd)][1], split=int(pb == 1))
    two = lambda: [(0, 0, 4, words(4), words(16)), (64, 0, 1, words(4), words(16))]
    # all nine candidates of every round tie: the first one of round 0 wins and nothing after it is strictly smaller
    add("flat_0_vs_max", 128, 64, _sp_planes(128, 64, 64, full(0), full(mx)), two(), 0, 1, 1, tie)
    add("flat_max_vs_0", 128, 64, _sp_planes(128, 64, 64, full(mx), full(0)), two(), 0, 1, 0, tie)
    add("flat_0_vs_max_hp0", 64, 64, _sp_planes(64, 64, 64, full(0), full(mx)), [(0, 0, 2, words(4), words(16))], 0, 0, 1, tie)
    add("flat_max_vs_0_hp0", 64, 64, _sp_planes(64, 64, 64, full(mx), full(0)), [(0, 0, 0, words(4), words(16))], 0, 0, 0, tie)
    # every row the same: the three candidates of one horizontal offset (one i, three j) tie, the first of the best column wins
    row = np.clip(rng.integers(0, 256, 64 + 2 * 64 + 8) * sc, 0, mx)
    add("rows_equal", 64, 64, _sp_planes(64, 64, 64, lambda p, xx, yy: row[xx + 64], lambda p, xx, yy: row[xx + 64 + 3] if p == 0 else row[xx + 32 + 1]),
        [(0, 0, 1, words(4), words(16))], 0, 1, 1)
    # 0 / max in cells of two samples (a cell of one sample is the Nyquist pattern, which no AV1 kernel overshoots on): at half a sample the two large taps meet
    # max and the negative ones 0 -- or the inverse -- so both clamps of every filtered branch bind; the central picture is binary noise, so no position matches
    cells = lambda p, xx, yy: mx * (((xx >> 1) + (yy >> 1)) & 1)
    noise01 = [mx * rng.integers(0, 2, (64 >> (p > 0), 64 >> (p > 0))) for p in range(3)]
    half = np.array([qpel_word(2, 2), qpel_word(2, 0), qpel_word(0, 2), qpel_word(-6, 10)], np.uint32)
    add("overshoot", 64, 64, _sp_planes(64, 64, 64, lambda p, xx, yy: noise01[p], cells), [(0, 0, 2, half, np.repeat(half, 4))], 0, 1, 1)
    # the split decision's wrap: quadrant 0 of job 0 is all 0, its 32x32 vector points into the all-max part of the reference (err32 = 2^30 at bd 10), its 16x16
    # vectors into the all-0 part (err16 = 0): 15 * 2^30 wraps to -2^30 < 0 = 16 * sum -> no split; in 64 bits 15 * 2^30 < 0 is false -> split
    edge = lambda p, xx, yy: mx * (xx >= (72 >> (p > 0)))
    far = z4.copy(); far[0] = qpel_word(88 * 4, 0)
    add("split_wrap", 128, 64, _sp_planes(128, 64, 64, full(0), edge), [(0, 0, 3, far, z16), (64, 0, 0, z4, z16)], 0, 1, 1)
    # texture + noise: every quadrant has an error of its own -- the threshold-equality runs take one of them as th16
    def tex(p, xx, yy, ox=0.0, oy=0.0):
        return np.clip((120 + 60 * np.sin((xx + ox) / (7.0 + p)) * np.cos((yy + oy) / (5.0 + p)) + 30 * np.sin((xx + ox + 2 * (yy + oy)) / 3.1) + rng.normal(0, 3, xx.shape)) * sc, 0, mx)
    add("texture", 64, 64, _sp_planes(64, 64, 64, tex, lambda p, xx, yy: tex(p, xx, yy, 2.3 / (1 + (p > 0)), -1.6 / (1 + (p > 0)))), [(0, 0, 1, words(4), words(16))], 1 << 40, 1, 1)
    # start vectors at the int16 edges: quarter-pel halves of +-16383 / -16384 double to +-32766 / -32768, and the candidates around them wrap
    e32 = np.array([qpel_word(16383, 5), qpel_word(-16383, -16383), qpel_word(7, 16383), qpel_word(-16384, 16383)], np.uint32)
    e16 = words(16); e16[[0, 5, 10, 15]] = e32; e16[3] = qpel_word(-16384, -16384)
    rnd_planes = _sp_planes(64, 64, 64, lambda p, xx, yy: rng.integers(0, mx + 1, xx.shape), lambda p, xx, yy: rng.integers(0, mx + 1, xx.shape))
    add("int16_edge", 64, 64, rnd_planes, [(0, 0, 2, e32, e16)], 0, 1, 1)
    return cases


def check_tie_closed_forms(c, blk):
    """every chosen vector = its start vector - (4, 4) in 1/8 pel and nothing else; the distortions are the closed forms; no split"""
    e = c.expect
    for J in c.jobs:
        B = blk[int(J["blk_index"])]
        for q in range(4):
            assert (int(B["mv32_x"][q]), int(B["mv32_y"][q])) == (i16(i16(int(J["mv32"][q]) & 0xffff) * 2) + e["offset"][0], i16(i16(int(J["mv32"][q]) >> 16) * 2) + e["offset"][1])
            assert int(B["err32"][q]) == e["err32"] and int(B["split"][q]) == e["split"]
        for k in range(16):
            assert (int(B["mv16_x"][k]), int(B["mv16_y"][k])) == (i16(i16(int(J["mv16"][k]) & 0xffff) * 2) + e["offset"][0], i16(i16(int(J["mv16"][k]) >> 16) * 2) + e["offset"][1])
            assert int(B["err16"][k]) == e["err16"]


def threshold_equality_runs(run, case):
    """run(case) -> block array.  With a huge th16 no quadrant is searched at 16x16; with th16 = one quadrant's err32 that quadrant is (do16 = !(err32 < th16)), with
    th16 one more it is not.  -> the three block arrays"""
    base = run(case)
    B = base[int(case.jobs["blk_index"][0])]
    assert not B["err16"].any() and len(set(int(v) for v in B["err32"])) == 4
    q = int(np.argsort(B["err32"])[2]); e = int(B["err32"][q])
    at, above = run(case.with_th16(e)), run(case.with_th16(e + 1))
    A, Z = at[int(case.jobs["blk_index"][0])], above[int(case.jobs["blk_index"][0])]
    assert int(A["err32"][q]) == e == int(Z["err32"][q])           # err32 == th16 occurs
    assert A["err16"][4 * q:4 * q + 4].all() and not Z["err16"][4 * q:4 * q + 4].any()
    assert sum(bool(A["err16"][4 * k:4 * k + 4].any()) for k in range(4)) == 2 and sum(bool(Z["err16"][4 * k:4 * k + 4].any()) for k in range(4)) == 1
    return base, at, above
