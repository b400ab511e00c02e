"""What the super-resolution tests share: ctypes prototypes of the reference's exported upscale functions, a function-for-function Python restatement of the
reference's scaler (Encoder/Codec/EbResize.c:186-765) that counts which range of each filter a case takes, a restatement of the tile-column loop of
svt_av1_upscale_normative_rows (Common/Codec/EbSuperRes.c:220-294), a reader of svt-av1_amd/csrc/resize_filters.h, and the case lists."""
import collections
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_planes.npz")
FILTER_NAMES = ["NORMATIVE", "875", "750", "625", "500"]


# ---------------------------------------------------------------- svt-av1_amd/csrc/resize_filters.h as numbers
def header_tables():
    """{"NORMATIVE" | "875" | "750" | "625" | "500": int [64][8], "EVEN" | "ODD": [4]} as resize_filters.h defines them"""
    txt = open(os.path.join(ROOT, "svt-av1_amd", "csrc", "resize_filters.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S).replace("\\\n", " ")
    out = {}
    for name, body in re.findall(r"^#define\s+SVT_RESIZE_(\w+)\s+(\{.*\})\s*$", txt, flags=re.M):
        vals = [int(v) for v in re.findall(r"-?\d+", body)]
        if name.startswith("FILTER_"):
            out[name[len("FILTER_"):]] = np.array(vals, np.int64).reshape(64, 8)
        else:
            out[{"DOWN2_SYMEVEN_HALF": "EVEN", "DOWN2_SYMODD_HALF": "ODD"}[name]] = vals
    assert sorted(out) == sorted(FILTER_NAMES + ["EVEN", "ODD"])
    return out


TABLES = header_tables()


# ---------------------------------------------------------------- the reference's exported functions (oracle/_ref/libsvtav1_ref.so, fixture `ref`)
MARGIN = 8   # the rect functions write 5 columns left and right of their input for the time of the call


def prepare(ref):
    i = C.c_int
    ref.upscale_normative_rect.restype, ref.upscale_normative_rect.argtypes = None, [C.c_void_p, i, i, i, C.c_void_p, i, i, i, i, i, i, i]
    ref.highbd_upscale_normative_rect.restype, ref.highbd_upscale_normative_rect.argtypes = None, [C.c_void_p, i, i, i, C.c_void_p, i, i, i, i, i, i, i, i]
    ref.get_upscale_convolve_x0.restype, ref.get_upscale_convolve_x0.argtypes = C.c_int32, [i, i, C.c_int32]
    ref.calculate_scaled_size_helper.restype, ref.calculate_scaled_size_helper.argtypes = None, [C.POINTER(C.c_uint16), C.c_uint8]
    return ref


def ref_scaled_dim(ref, dim, denom):
    v = C.c_uint16(dim)
    ref.calculate_scaled_size_helper(C.byref(v), denom)
    return v.value


def cdiv(a, b):
    """C's division: towards zero"""
    return -((-a) // b) if (a < 0) != (b < 0) else a // b


def upscale_step(in_w, out_w):
    """av1_get_upscale_convolve_step (static in the reference)"""
    return ((in_w << 14) + out_w // 2) // out_w


def upscale_x0(in_w, out_w, step):
    """get_upscale_convolve_x0"""
    err = out_w * step - (in_w << 14)
    return (cdiv(-((out_w - in_w) << 13) + out_w // 2, out_w) + 128 - cdiv(err, 2)) & 0x3fff


def ref_rect(ref, plane, x_first, src_w, dst_w, step, x0_qn, pad_left, pad_right, bd, sentinel):
    """One call of [highbd_]upscale_normative_rect on columns x_first .. x_first + src_w of `plane`, which sits in a buffer with MARGIN columns of `sentinel`
    either side (the call may write 5 of them and must put them back)."""
    rows, w = plane.shape
    buf = np.full((rows, w + 2 * MARGIN), sentinel, plane.dtype)
    buf[:, MARGIN:MARGIN + w] = plane
    before = buf.copy()
    out = np.zeros((rows, dst_w), plane.dtype)
    src = buf.ctypes.data + (MARGIN + x_first) * plane.itemsize
    if plane.dtype == np.uint8:
        ref.upscale_normative_rect(src, rows, src_w, buf.shape[1], out.ctypes.data, rows, dst_w, dst_w, step, x0_qn, pad_left, pad_right)
    else:
        ref.highbd_upscale_normative_rect(src, rows, src_w, buf.shape[1], out.ctypes.data, rows, dst_w, dst_w, step, x0_qn, pad_left, pad_right, bd)
    assert np.array_equal(buf, before), "the reference did not restore its input"
    return out


def ref_upscale(ref, plane, out_w, bd, sentinel=0):
    """the whole plane in one call: one tile column, padded on both sides"""
    step = upscale_step(plane.shape[1], out_w)
    return ref_rect(ref, plane, 0, plane.shape[1], out_w, step, ref.get_upscale_convolve_x0(plane.shape[1], out_w, step), 1, 1, bd, sentinel)


def ref_upscale_tiled(ref, plane, out_w, denom, bounds, bd):
    """svt_av1_upscale_normative_rows' loop: tile columns at the source positions `bounds` (ascending, inside the plane; the reference's are multiples of 4
    luma samples).  Interior columns are NOT padded: they read their neighbours' samples."""
    in_w = plane.shape[1]
    step = upscale_step(in_w, out_w)
    x0_qn = ref.get_upscale_convolve_x0(in_w, out_w, step)
    edges = [0] + list(bounds) + [in_w]
    out = np.zeros((plane.shape[0], out_w), plane.dtype)
    for j in range(len(edges) - 1):
        d0, d1 = edges[j], edges[j + 1]
        u0 = (d0 * denom) // 8
        u1 = out_w if j == len(edges) - 2 else (d1 * denom) // 8
        out[:, u0:u1] = ref_rect(ref, plane, d0, d1 - d0, u1 - u0, step, x0_qn, int(j == 0), int(j == len(edges) - 2), bd, 0)
        x0_qn += (u1 - u0) * step - ((d1 - d0) << 14)
    return out


def numpy_upscale(plane, out_w, bd):
    """the normative upscale as the device computes it: position x0 + x * step for the whole row, source indices clamped to the row"""
    in_w = plane.shape[1]
    step = upscale_step(in_w, out_w)
    q = upscale_x0(in_w, out_w, step) + np.arange(out_w, dtype=np.int64) * step
    idx = np.clip((q >> 14)[:, None] - 4 + np.arange(8)[None, :], 0, in_w - 1)
    taps = TABLES["NORMATIVE"][(q & 0x3fff) >> 8]
    s = (plane.astype(np.int64)[:, idx] * taps[None]).sum(axis=2)
    return np.clip((s + 64) >> 7, 0, (1 << bd) - 1).astype(plane.dtype)


def upscale_phases(in_w, out_w):
    step = upscale_step(in_w, out_w)
    return {((upscale_x0(in_w, out_w, step) + x * step) & 0x3fff) >> 8 for x in range(out_w)}


# ---------------------------------------------------------------- EbResize.c:186-765, function for function (lines are lists of ints)
TAKEN = collections.Counter()   # (function, range) and ("filter", name): what the restatement went through since the last TAKEN.clear()


def clip_pixel(v, bd):
    return 0 if v < 0 else (1 << bd) - 1 if v > (1 << bd) - 1 else v


def get_down2_length(length, steps):
    for _ in range(steps):
        length = (length + 1) >> 1
    return length


def get_down2_steps(in_length, out_length):
    steps = 0
    while True:
        proj = get_down2_length(in_length, 1)
        if proj < out_length:
            break
        steps += 1
        in_length = proj
        if in_length == 1:
            break
    return steps


def down2_symeven(inp, length, bd):
    f = TABLES["EVEN"]
    half = len(f)
    out = []
    l1, l2 = half, length - half
    l1 += l1 & 1
    l2 += l2 & 1

    def one(i, lo, hi):
        s = 64
        for j in range(half):
            a = max(i - j, 0) if lo else i - j
            b = min(i + 1 + j, length - 1) if hi else i + 1 + j
            assert 0 <= a < length and 0 <= b < length
            s += (inp[a] + inp[b]) * f[j]
        return clip_pixel(s >> 7, bd)
    if l1 > l2:
        TAKEN["down2_symeven", "short"] += 1
        out = [one(i, True, True) for i in range(0, length, 2)]
    else:
        for i in range(0, length, 2):
            rng = "initial" if i < l1 else "middle" if i < l2 else "end"
            TAKEN["down2_symeven", rng] += 1
            out.append(one(i, rng == "initial", rng == "end"))
    return out


def down2_symodd(inp, length, bd):
    f = TABLES["ODD"]
    half = len(f)
    out = []
    l1, l2 = half - 1, length - half + 1
    l1 += l1 & 1
    l2 += l2 & 1

    def one(i, lo, hi):
        s = 64 + inp[i] * f[0]
        for j in range(1, half):
            a = max(i - j, 0) if lo else i - j
            b = min(i + j, length - 1) if hi else i + j
            assert 0 <= a < length and 0 <= b < length
            s += (inp[a] + inp[b]) * f[j]
        return clip_pixel(s >> 7, bd)
    if l1 > l2:
        TAKEN["down2_symodd", "short"] += 1
        out = [one(i, True, True) for i in range(0, length, 2)]
    else:
        for i in range(0, length, 2):
            rng = "initial" if i < l1 else "middle" if i < l2 else "end"
            TAKEN["down2_symodd", rng] += 1
            out.append(one(i, rng == "initial", rng == "end"))
    return out


def choose_interp_filter(in_length, out_length):
    o16 = out_length * 16
    name = ("NORMATIVE" if o16 >= in_length * 16 else "875" if o16 >= in_length * 13 else "750" if o16 >= in_length * 11 else "625" if o16 >= in_length * 9
            else "500")
    TAKEN["filter", name] += 1
    return name


def interpolate_core(inp, in_length, out_length, bd, filters):
    taps = 8
    delta = ((in_length << 14) + out_length // 2) // out_length
    offset = ((((in_length - out_length) << 13) + out_length // 2) // out_length if in_length > out_length
              else -((((out_length - in_length) << 13) + out_length // 2) // out_length))
    x, y = 0, offset + 128
    while (y >> 14) < taps // 2 - 1:
        x += 1
        y += delta
    x1 = x
    x = out_length - 1
    y = delta * x + offset + 128
    while (y >> 14) + taps // 2 >= in_length:
        x -= 1
        y -= delta
    x2 = x

    def one(x, lo, hi):
        y = offset + 128 + x * delta
        int_pel, sub_pel = y >> 14, (y >> 8) & 63
        s = 0
        for k in range(taps):
            pk = int_pel - taps // 2 + 1 + k
            if hi: pk = min(pk, in_length - 1)
            if lo: pk = max(pk, 0)
            assert 0 <= pk < in_length
            s += int(filters[sub_pel][k]) * inp[pk]
        return clip_pixel((s + 64) >> 7, bd)
    if x1 > x2:
        TAKEN["interpolate_core", "short"] += 1
        return [one(x, True, True) for x in range(out_length)]
    out = []
    for x in range(out_length):
        rng = "initial" if x < x1 else "middle" if x <= x2 else "end"
        TAKEN["interpolate_core", rng] += 1
        out.append(one(x, rng == "initial", rng == "end"))
    return out


def interpolate(inp, in_length, out_length, bd):
    return interpolate_core(inp, in_length, out_length, bd, TABLES[choose_interp_filter(in_length, out_length)])


def resize_multistep(inp, length, olength, bd):
    if length == olength:
        return list(inp)
    steps = get_down2_steps(length, olength)
    if steps > 0:
        out, filteredlength = inp, length
        for _ in range(steps):
            out = down2_symodd(out, filteredlength, bd) if filteredlength & 1 else down2_symeven(out, filteredlength, bd)
            filteredlength = get_down2_length(filteredlength, 1)
        assert len(out) == filteredlength
        return interpolate(out, filteredlength, olength, bd) if filteredlength != olength else out
    return interpolate(inp, length, olength, bd)


def resize_plane(plane, height2, width2, bd):
    """av1_resize_plane / av1_highbd_resize_plane: rows first into the intermediate plane (clipped to samples), then columns"""
    height, width = plane.shape
    intbuf = [resize_multistep([int(v) for v in plane[i]], width, width2, bd) for i in range(height)]
    out = np.zeros((height2, width2), plane.dtype)
    for i in range(width2):
        out[:, i] = resize_multistep([intbuf[r][i] for r in range(height)], height, height2, bd)
    return out


def numpy_multistep(a, olength, bd):
    """resize_multistep along axis 1 of the int64 array `a`, every filter written once with both clamps (what the device computes; proven equal to the
    function-for-function form on the golden planes by tests/test_resize_ref_cpu.py)"""
    maxv = (1 << bd) - 1
    if a.shape[1] == olength:
        return a
    for _ in range(get_down2_steps(a.shape[1], olength)):
        n = a.shape[1]
        i = np.arange(0, n, 2)
        if n & 1:
            f = TABLES["ODD"]
            s = 64 + a[:, i] * f[0] + sum((a[:, np.maximum(i - j, 0)] + a[:, np.minimum(i + j, n - 1)]) * f[j] for j in range(1, 4))
        else:
            f = TABLES["EVEN"]
            s = 64 + sum((a[:, np.maximum(i - j, 0)] + a[:, np.minimum(i + 1 + j, n - 1)]) * f[j] for j in range(4))
        a = np.clip(s >> 7, 0, maxv)
    n = a.shape[1]
    if n != olength:
        delta = ((n << 14) + olength // 2) // olength
        offset = (((n - olength) << 13) + olength // 2) // olength if n > olength else -((((olength - n) << 13) + olength // 2) // olength)
        y = offset + 128 + np.arange(olength, dtype=np.int64) * delta
        o16 = olength * 16
        name = "NORMATIVE" if o16 >= n * 16 else "875" if o16 >= n * 13 else "750" if o16 >= n * 11 else "625" if o16 >= n * 9 else "500"
        idx = np.clip((y >> 14)[:, None] - 3 + np.arange(8)[None, :], 0, n - 1)
        s = (a[:, idx] * TABLES[name][(y >> 8) & 63][None]).sum(axis=2)
        a = np.clip((s + 64) >> 7, 0, maxv)
    return a


def numpy_resize_plane(plane, height2, width2, bd):
    mid = numpy_multistep(plane.astype(np.int64), width2, bd)
    return numpy_multistep(mid.T, height2, bd).T.astype(plane.dtype)


# ---------------------------------------------------------------- case lists
SUPERRES_DENOMS = list(range(9, 17))
UPSCALE_WIDTHS = [16, 17, 33, 90, 129, 352]
UPSCALE_ROWS = [1, 2, 5, 70]


def scaled_dim(dim, denom):
    """calculate_scaled_size_helper"""
    return dim if denom == 8 else max((dim * 8 + denom // 2) // denom, min(16, dim))


def golden_shapes():
    """[(name, in_h, in_w, out_h, out_w, content)]: the cases of tests/golden/resize_planes.npz.  An axis pair a -> b is run along a row (2 rows high) and
    down a column (2 columns wide)."""
    pairs = [(1, 1), (2, 1), (3, 2), (5, 3), (6, 3), (7, 4), (16, 16), (100, 25), (64, 15), (65, 16), (16, 24), (5, 4), (4, 6)]   # the last two: interpolate_core's short range
    pairs += [(w, scaled_dim(w, d)) for w in (16, 17, 64, 353) for d in SUPERRES_DENOMS]
    cases = []
    for a, b in pairs:
        cases.append((f"row_{a}_{b}", 2, a, 2, b, "random"))
        if a != 353 or b in (scaled_dim(353, 9), scaled_dim(353, 16)):
            cases.append((f"col_{a}_{b}", a, 2, b, 2, "random"))
    cases += [("both_48x40_30x25", 40, 48, 25, 30, "random"), ("rows_48x40_48x25", 40, 48, 25, 48, "random"), ("checker_24x20_15x11", 20, 24, 11, 15, "checker")]
    out, seen = [], set()
    for c in cases:   # denominators can give one size twice
        if c[0] not in seen:
            seen.add(c[0]); out.append(c)
    return out


def make_plane(name, h, w, content, dtype, bd):
    maxv = (1 << bd) - 1
    if content == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return ((((yy >> 2) + (xx >> 2)) & 1) * maxv).astype(dtype)   # 4 x 4 fields: a finer one is filtered to grey
    rng = np.random.default_rng(abs(hash_name(name)) + bd)
    return rng.integers(0, maxv + 1, (h, w)).astype(dtype)


def hash_name(name):
    v = 0
    for ch in name.encode():
        v = (v * 131 + ch) % 1000003
    return v


def load_golden():
    """{(name, "u8" | "u16"): (input plane, expected plane)}; 16-bit planes hold 10-bit samples"""
    z = np.load(GOLDEN)   # four flat arrays (in_u8, out_u8, in_u16, out_u16): the planes of golden_shapes() one after the other
    out, off = {}, {"in_u8": 0, "out_u8": 0, "in_u16": 0, "out_u16": 0}
    for n, ih, iw, oh, ow, _ in golden_shapes():
        for t in ("u8", "u16"):
            pair = []
            for k, h, w in (("in_" + t, ih, iw), ("out_" + t, oh, ow)):
                pair.append(z[k][off[k]:off[k] + h * w].reshape(h, w))
                off[k] += h * w
            out[n, t] = tuple(pair)
    assert all(off[k] == len(z[k]) for k in off)
    return out
