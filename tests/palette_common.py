"""What the palette tests share: search_palette_luma (Encoder/Codec/palette.c:320-496) and is_screen_content (Encoder/Codec/EbPictureAnalysisProcess.c:3519-3601)
restated line for line in Python around a backend of four functions -- the reference's own exports (`ref_search`, `ref_screen_content`) or plain numpy
(`numpy_search`, which also records what the case list has to prove about itself: reseeds, iterations, ties, the restore branch) -- and the case lists, built by
loops.  A search result is {"colors", "cands": [{"size", "colors", "raw", "n", "kind", "color_cost", "map"}]} with the candidates in the reference's order."""
import ctypes as C

import numpy as np

SHAPES = [(8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]
FORMATS = [(np.uint8, 8), (np.uint16, 8), (np.uint16, 10)]   # (sample type, bit depth)
MAX_CANDS = 14


# ------------------------------------------------------------------------------------------------------------------ the two backends
class PaletteModeInfo(C.Structure):   # 24 uint16_t + 2 uint8_t
    _fields_ = [("palette_colors", C.c_uint16 * 24), ("palette_size", C.c_uint8 * 2)]


def _lcg_rand16(state):
    state[0] = (state[0] * 1103515245 + 12345) & 0xFFFFFFFF
    return state[0] // 65536 % 32768


def _ceil_log2(n):
    if n < 2: return 0
    i, p = 1, 2
    while p < n:
        i += 1; p <<= 1
    return i


class NumpyBackend:
    """count_colors, k_means, calc_indices and palette_color_cost_y in numpy / plain Python; `stats` collects one record per k_means call"""

    def __init__(self):
        self.stats = []          # per k_means call: dict(k, n, iterations, reseeds per iteration, restored)
        self.equidistant = 0     # samples that had two nearest centroids, over every calc_indices

    def count_colors(self, block, bd):
        if int(block.max()) >= 1 << bd: return 0, None   # svt_av1_count_colors_highbd's early return
        counts = np.bincount(block.ravel().astype(np.int64), minlength=1 << bd)
        return int((counts != 0).sum()), counts

    def calc_indices(self, data, centroids):
        d = (data[:, None].astype(np.int64) - np.asarray(centroids, np.int64)[None, :]) ** 2
        idx = d.argmin(axis=1)   # the first minimum
        self.equidistant += int(((d == d.min(axis=1)[:, None]).sum(axis=1) > 1).sum())
        return idx.astype(np.uint8), int(d.min(axis=1).sum())

    def k_means(self, data, centroids, k):
        cent = list(centroids[:k])
        n = len(data)
        rec = dict(k=k, n=n, iterations=0, reseeds=[], restored=False)
        idx, this_dist = self.calc_indices(data, cent)
        for _ in range(50):
            pre_dist, pre = this_dist, list(cent)
            rec["iterations"] += 1
            state, reseeds = [int(data[0]) & 0xFFFFFFFF], 0
            count = np.bincount(idx, minlength=k)
            sums = np.bincount(idx, weights=data.astype(np.float64), minlength=k).astype(np.int64)   # < 2^53: exact
            for j in range(k):
                if count[j] == 0:
                    cent[j] = int(data[_lcg_rand16(state) % n]); reseeds += 1
                else:
                    cent[j] = int((sums[j] + (count[j] >> 1)) // count[j])
            rec["reseeds"].append(reseeds)
            idx, this_dist = self.calc_indices(data, cent)
            if this_dist > pre_dist:
                cent = pre; rec["restored"] = True
                break
            if cent == pre: break
        self.stats.append(rec)
        return cent

    def color_cost(self, colors, cache, bd):
        n, n_cache = len(colors), len(cache)
        if n_cache <= 0:
            out = list(colors)
        else:
            flags, n_in = [0] * 8, 0
            for i in range(n_cache):
                if n_in >= n: break
                for j in range(n):
                    if colors[j] == cache[i]:
                        flags[j] = 1; n_in += 1
                        break
            out = [c for c, f in zip(colors, flags) if not f]
        bits, num = 0, len(out)   # delta_encode_cost(out, num, bd, 1)
        if num > 0:
            bits = bd
            if num > 1:
                bits += 2
                deltas = [out[i] - out[i - 1] for i in range(1, num)]
                per = max(_ceil_log2(max(max(deltas), 0) + 1 - 1), bd - 3)
                rng = (1 << bd) - out[0] - 1
                for d in deltas:
                    bits += per
                    rng -= d
                    per = min(per, _ceil_log2(rng))
        return (n_cache + bits) * 512


class RefBackend:
    """the same four through the reference's exported functions"""

    def __init__(self, ref):
        self.L = ref
        ref.svt_av1_count_colors.restype = ref.svt_av1_count_colors_highbd.restype = ref.svt_av1_palette_color_cost_y.restype = C.c_int
        ref.svt_av1_k_means_dim1_c.restype = ref.svt_av1_calc_indices_dim1_c.restype = None

    def count_colors(self, block, bd):
        block = np.ascontiguousarray(block)
        counts = np.zeros(1 << 12, np.int32)
        p, q = block.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)
        if block.dtype == np.uint8: n = self.L.svt_av1_count_colors(p, C.c_int(block.shape[1]), C.c_int(block.shape[0]), C.c_int(block.shape[1]), q)
        else: n = self.L.svt_av1_count_colors_highbd(p, C.c_int(block.shape[1]), C.c_int(block.shape[0]), C.c_int(block.shape[1]), C.c_int(bd), q)
        return n, counts[:1 << bd]

    def calc_indices(self, data, centroids):
        cent = np.asarray(centroids, np.int32)
        idx = np.zeros(len(data), np.uint8)
        self.L.svt_av1_calc_indices_dim1_c(data.ctypes.data_as(C.c_void_p), cent.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), C.c_int(len(data)), C.c_int(len(cent)))
        return idx, None

    def k_means(self, data, centroids, k):
        cent = np.asarray(centroids[:k], np.int32).copy()
        idx = np.zeros(len(data), np.uint8)
        self.L.svt_av1_k_means_dim1_c(data.ctypes.data_as(C.c_void_p), cent.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), C.c_int(len(data)), C.c_int(k), C.c_int(50))
        return [int(v) for v in cent]

    def color_cost(self, colors, cache, bd):
        pmi = PaletteModeInfo()
        for i, c in enumerate(colors): pmi.palette_colors[i] = c
        pmi.palette_size[0] = len(colors)
        cc = (C.c_uint16 * 16)(*cache)
        return self.L.svt_av1_palette_color_cost_y(C.byref(pmi), cc, C.c_int(len(cache)), C.c_int(bd))


# ------------------------------------------------------------------------------------------------------------------ search_palette_luma
def job_ok(job):
    return ((job["bw"], job["bh"]) in SHAPES and 1 <= job["cols"] <= job["bw"] and 1 <= job["rows"] <= job["bh"] and job["x"] >= 0 and job["y"] >= 0 and
            0 <= len(job["cache"]) <= 16 and job["step"] in (1, 2))


def _palette_rd_y(be, data, centroids, n, job, bd):
    """palette_rd_y: -> None (palette_size 0) or the candidate without kind / raw"""
    cache, cent = job["cache"], list(centroids[:n])
    if len(cache) > 0:   # optimize_palette_colors
        for i in range(n):
            min_diff, idx = abs(cent[i] - cache[0]), 0
            for j in range(1, len(cache)):
                if abs(cent[i] - cache[j]) < min_diff: min_diff, idx = abs(cent[i] - cache[j]), j
            if min_diff <= 1: cent[i] = cache[idx]
    cent = sorted(cent)   # av1_remove_duplicates
    uniq = [cent[0]] + [cent[i] for i in range(1, n) if cent[i] != cent[i - 1]]
    k = len(uniq)
    if k < 2: return None
    colors = [min(max(c, 0), (1 << bd) - 1) for c in uniq]
    idx, _ = be.calc_indices(data, uniq)
    rows, cols, bw, bh = job["rows"], job["cols"], job["bw"], job["bh"]
    m = np.empty((bh, bw), np.uint8)   # extend_palette_color_map
    m[:rows, :cols] = idx.reshape(rows, cols)
    m[:rows, cols:] = m[:rows, cols - 1:cols]
    m[rows:, :] = m[rows - 1:rows, :]
    return dict(size=k, colors=colors + [0] * (8 - k), map=m, color_cost=be.color_cost(colors, cache, bd))


def search(be, plane, job, bd):
    """search_palette_luma of one job of `plane` (2-D uint8 / uint16) through backend `be`"""
    if not job_ok(job): return dict(colors=-1, cands=[])
    rows, cols = job["rows"], job["cols"]
    block = np.ascontiguousarray(plane[job["y"]:job["y"] + rows, job["x"]:job["x"] + cols])
    colors, counts = be.count_colors(block, bd)
    out = dict(colors=colors, cands=[])
    if not (1 < colors <= 64): return out
    data = block.ravel().astype(np.int32)   # GENERATE_KMEANS_DATA
    lb, ub = int(data.min()), int(data.max())
    counts = np.array(counts, np.int64)
    top = []
    for _ in range(min(colors, 8)):   # the first largest: the strict > of the reference's scan
        top.append(int(counts.argmax())); counts[top[-1]] = 0

    def consider(centroids, n, kind):
        cand = _palette_rd_y(be, data, centroids, n, job, bd)
        if cand is not None and cand["size"] > 2:
            cand.update(kind=kind, n=n, raw=[int(c) for c in centroids[:n]] + [0] * (8 - n))
            out["cands"].append(cand)

    for n in range(min(colors, 8), 1, -job["step"]):
        consider(top[:n], n, 0)
    for n in range(min(colors, 8), 1, -1):
        if colors == 2: cent = [lb, ub]
        else: cent = be.k_means(data, [lb + (2 * i + 1) * (ub - lb) // n // 2 for i in range(n)], n)
        consider(cent, n, 1)
    assert len(out["cands"]) <= MAX_CANDS
    return out


def ref_search(ref, plane, job, bd):
    return search(RefBackend(ref), plane, job, bd)


def numpy_search(plane, job, bd, backend=None):
    return search(backend or NumpyBackend(), plane, job, bd)


def same_result(a, b):
    """None when two search results agree in every field, else what differs first"""
    if a["colors"] != b["colors"] or len(a["cands"]) != len(b["cands"]): return f"colors / n_cands {a['colors']}, {len(a['cands'])} != {b['colors']}, {len(b['cands'])}"
    for i, (p, q) in enumerate(zip(a["cands"], b["cands"])):
        for f in ("size", "colors", "raw", "n", "kind", "color_cost"):
            if p[f] != q[f]: return f"candidate {i}: {f} {p[f]} != {q[f]}"
        if not np.array_equal(p["map"], q["map"]): return f"candidate {i}: map differs at {np.argwhere(p['map'] != q['map'])[:4].tolist()}"
    return None


# ------------------------------------------------------------------------------------------------------------------ to and from the C ABI
def c_jobs(pkg, jobs, spacing=None):
    """-> (PaletteJob array, bytes of maps): every job gets 14 * bw * bh map bytes (64 * 64 for a job whose own size is bad), `spacing` more between jobs"""
    tab, off = (pkg.PaletteJob * max(len(jobs), 1))(), 0
    for i, j in enumerate(jobs):
        cache = list(j["cache"])
        tab[i] = pkg.PaletteJob(j["x"], j["y"], j["bw"], j["bh"], j["cols"], j["rows"], j.get("n_cache", len(cache)), j["step"], (C.c_uint16 * 16)(*cache[:16]), off)
        j["map_off"] = off
        off += MAX_CANDS * (j["bw"] * j["bh"] if (j["bw"], j["bh"]) in SHAPES else 4096) + (spacing or 0)
    return tab, max(off, 4)


def c_result(job, res, cands, maps, i):
    """job i of the ABI's three outputs as a search result"""
    out = dict(colors=res[i].colors, cands=[])
    area = job["bw"] * job["bh"]
    for c in range(res[i].n_cands):
        r = cands[MAX_CANDS * i + c]
        m = maps[job["map_off"] + c * area: job["map_off"] + (c + 1) * area].reshape(job["bh"], job["bw"])
        out["cands"].append(dict(size=r.size, colors=list(r.colors), raw=list(r.raw), n=r.n, kind=r.kind, color_cost=r.color_cost, map=m, reserved=r.reserved))
    return out


def untouched(jobs, results, res, cands, maps, fill):
    """None when everything outside the jobs' own regions still holds the pre-fill byte `fill`, else what does not: records and map bytes behind n_cands are the
    job's own (unspecified), the space between the jobs' maps and behind the last is nobody's"""
    own = np.zeros(len(maps), bool)
    for i, j in enumerate(jobs):
        if results[i]["colors"] < 0:
            size = MAX_CANDS * C.sizeof(cands[0])
            if C.string_at(C.addressof(cands) + i * size, size) != bytes([fill]) * size: return f"bad job {i}: its records were written"
            continue
        own[j["map_off"]: j["map_off"] + MAX_CANDS * j["bw"] * j["bh"]] = True
    if (maps[~own] != fill).any(): return f"map bytes outside every job's region were written: {np.flatnonzero((maps != fill) & ~own)[:8].tolist()}"
    return None


# ------------------------------------------------------------------------------------------------------------------ content
def _levels(rng, n, bd):
    return np.sort(rng.choice(1 << bd, n, replace=False))


def content(kind, rng, bw, bh, bd, arg=None):
    """a bh x bw block of `kind` content at bit depth bd (values scale with the depth: 10-bit blocks reach 1023)"""
    top, sc = (1 << bd) - 1, 1 << (bd - 8)
    if kind == "colors":        # exactly `arg` distinct values when the block has room for them, each at least once
        n = min(arg, bw * bh)
        lv = _levels(rng, n, bd)
        b = lv[rng.integers(0, n, bw * bh)]
        b[rng.permutation(bw * bh)[:n]] = lv
        return b.reshape(bh, bw)
    if kind == "two_cluster":   # 0 .. 5 and 250 .. 255 at random: empty clusters between the two groups
        return np.where(rng.integers(0, 2, (bh, bw)) == 1, top - rng.integers(0, 6, (bh, bw)), rng.integers(0, 6, (bh, bw)))
    if kind == "text":          # a plain ground with a few strokes of a few far colours
        b = np.full((bh, bw), int(rng.integers(0, 40)) * sc)
        for _ in range(int(rng.integers(2, 6))):
            y, x = int(rng.integers(0, bh)), int(rng.integers(0, bw))
            b[y:y + int(rng.integers(1, 3)), x:x + int(rng.integers(2, 8))] = min(top, int(rng.integers(180, 256)) * sc + int(rng.integers(0, sc)))
        b[rng.integers(0, bh), rng.integers(0, bw)] = top
        return b
    if kind == "ramp":
        return (np.add.outer(np.arange(bh), np.arange(bw)) * sc) % (top + 1)
    if kind == "noise64":       # many iterations: 64 levels spread unevenly
        lv = _levels(rng, 64, bd)
        return lv[np.minimum(63, (rng.random((bh, bw)) ** 2 * 64).astype(int))]
    if kind == "ties":          # four colours of equal count, a fifth rarer, a sixth rarest
        lv = _levels(rng, 6, bd)
        b = np.repeat(lv[:4], bw * bh // 4)
        b[0], b[1], b[2] = lv[4], lv[4], lv[5]
        return rng.permutation(b).reshape(bh, bw)
    if kind == "midpoint":      # 10, 20, 30 and a few samples half way between two of them
        b = np.array([10, 20, 30])[rng.integers(0, 3, bw * bh)] * sc
        b[:3] = 15 * sc
        b[3:6] = np.array([10, 20, 30]) * sc
        return rng.permutation(b).reshape(bh, bw)
    raise ValueError(kind)


def build_cases(dtype, bd, seed=0):
    """The case list of one sample format -> (plane, jobs): blocks packed on shelves of a plane whose rows are wider than the picture, starting at an odd column
    and one column apart, so that sources sit at odd and even x"""
    rng = np.random.default_rng(1000 * bd + np.dtype(dtype).itemsize + seed)
    blocks = []   # (block content bh x bw, job fields)

    def add(block, bw, bh, cols=None, rows=None, cache=(), step=1):
        blocks.append((np.asarray(block), dict(bw=bw, bh=bh, cols=cols or bw, rows=rows or bh, cache=list(cache), step=step)))

    def cache_of(n):
        return sorted(int(v) for v in rng.choice(1 << bd, n, replace=False))

    kinds = ["two_cluster", "text", ("colors", 5), "noise64", "ties", ("colors", 12), "midpoint", "ramp"]
    q = 0
    for bw, bh in SHAPES:                     # every shape whole and cut four ways
        for cut in ("whole", "cols", "rows", "both", "one"):
            kind = kinds[q % len(kinds)]
            blk = content(kind[0], rng, bw, bh, bd, kind[1]) if isinstance(kind, tuple) else content(kind, rng, bw, bh, bd)
            cols = {"whole": bw, "cols": bw - int(rng.integers(1, bw)), "rows": bw, "both": bw - int(rng.integers(1, bw)), "one": 1}[cut]
            rows = {"whole": bh, "cols": bh, "rows": bh - int(rng.integers(1, bh)), "both": bh - int(rng.integers(1, bh)), "one": 1}[cut]
            add(blk, bw, bh, cols, rows, cache_of((0, 1, 16)[q % 3]), 1 + (q // 3) % 2)
            q += 1
    for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 33, 64, 65, 100):   # the colour count, with both dominant steps
        for step in (1, 2):
            add(content("colors", rng, 16, 16, bd, n), 16, 16, step=step, cache=cache_of((0, 1, 16)[n % 3]))
    for kind in ("two_cluster", "text"):       # reseeds of empty clusters
        for bw, bh in ((8, 8), (16, 16), (32, 32), (64, 64)):
            for _ in range(3):
                add(content(kind, rng, bw, bh, bd), bw, bh)
    for kind in ("noise64", "ties", "midpoint"):
        for bw, bh in ((16, 16), (64, 64)):
            add(content(kind, rng, bw, bh, bd), bw, bh, cache=cache_of(16) if kind == "noise64" else ())
    # caches at a distance of exactly 0, 1 and 2 from a block's dominant colours, and one between two of them: both snap to it (duplicates after the snap)
    for n in (4, 8):
        blk = content("colors", rng, 16, 16, bd, n)
        lv = [int(v) for v in np.unique(blk)]
        for d in (0, 1, 2):
            add(blk, 16, 16, cache=sorted({min((1 << bd) - 1, v + d) for v in lv}))
    near = np.array([50, 52, 90, 140, 200])[rng.integers(0, 5, 256)].reshape(16, 16)
    near.flat[:5] = [50, 52, 90, 140, 200]
    add(near, 16, 16, cache=[51])
    add(near, 16, 16, cache=[51], step=2)
    # place them
    width, x, y, shelf = 300, 1, 0, 0
    placed = []
    for blk, job in blocks:
        if x + job["bw"] > width: x, y, shelf = 1 + (len(placed) & 1), y + shelf, 0
        placed.append((x, y)); x += job["bw"] + 1; shelf = max(shelf, job["bh"])
    base = rng.integers(0, 1 << bd, (y + shelf, width + 20)).astype(dtype)   # stride 320, picture 300 wide
    plane = base[:, :width]
    jobs = []
    for (blk, job), (px, py) in zip(blocks, placed):
        plane[py:py + job["bh"], px:px + job["bw"]] = blk
        jobs.append(dict(job, x=px, y=py))
    return plane, jobs


def build_tiles(dtype, bd, tiles_x=64, tiles_y=48, pool=40):
    """a few thousand 8x8 jobs on one plane, drawn from `pool` distinct (content, cache, step) kinds -> (plane, jobs, kind index of every job)"""
    rng = np.random.default_rng(77 + bd)
    kinds = []
    for i in range(pool):
        kind = ("two_cluster", "text", "ties", "midpoint")[i % 4] if i % 5 else None
        blk = content(kind, rng, 8, 8, bd) if kind else content("colors", rng, 8, 8, bd, 1 + i % 13)
        kinds.append((blk, sorted(int(v) for v in rng.choice(1 << bd, (0, 3, 16)[i % 3], replace=False)), 1 + i % 2))
    plane = np.zeros((8 * tiles_y, 8 * tiles_x), dtype)
    jobs, which = [], []
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            k = int(rng.integers(0, pool))
            plane[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8] = kinds[k][0]
            jobs.append(dict(x=8 * tx, y=8 * ty, bw=8, bh=8, cols=8, rows=8, cache=kinds[k][1], step=kinds[k][2])); which.append(k)
    return plane, jobs, which


# ------------------------------------------------------------------------------------------------------------------ is_screen_content
def ref_screen_content(ref, plane, bd):
    """is_screen_content on a 2-D uint8 (bd 8) / uint16 (bd 10) plane through the reference's exports -> [counts_1, counts_2, color_detection, sc_content_detected]"""
    ref.is_valid_palette_nb_colors.restype = ref.is_valid_palette_nb_colors_highbd.restype = C.c_uint8
    ref.svt_aom_variance16x16_c.restype = ref.svt_aom_highbd_10_variance16x16_c.restype = C.c_uint32
    h, w = plane.shape
    offs = np.full(128, 128 if bd == 8 else 512, plane.dtype)
    sse = C.c_uint32()
    counts_1 = counts_2 = 0
    for r in range(0, h - 15, 16):
        for c in range(0, w - 15, 16):
            blk = np.ascontiguousarray(plane[r:r + 16, c:c + 16])   # the 16-bit path works on a packed 16 x 16 copy as well
            if bd == 8:
                if not ref.is_valid_palette_nb_colors(blk.ctypes.data_as(C.c_void_p), C.c_int(16), C.c_int(16), C.c_int(16), C.c_int(4)): continue
                var = ref.svt_aom_variance16x16_c(blk.ctypes.data_as(C.c_void_p), C.c_int(16), offs.ctypes.data_as(C.c_void_p), C.c_int(0), C.byref(sse))
            else:
                if not ref.is_valid_palette_nb_colors_highbd(blk.ctypes.data_as(C.c_void_p), C.c_int(16), C.c_int(16), C.c_int(16), C.c_int(4), C.c_int(bd)): continue
                var = ref.svt_aom_highbd_10_variance16x16_c(C.c_void_p(blk.ctypes.data >> 1), C.c_int(16), C.c_void_p(offs.ctypes.data >> 1), C.c_int(0), C.byref(sse))   # CONVERT_TO_BYTEPTR
            counts_1 += 1
            counts_2 += ((var + 128) >> 8) > 0
    color_detection = int(counts_1 * 16 * 16 * 10 > w * h)
    return [counts_1, counts_2, color_detection, int(bool(color_detection and counts_2 * 16 * 16 * 12 > w * h))]


def sc_block(kind, bd, rng):
    """a 16 x 16 block for the detection: `kind` is "flat", "var0" (two colours, one sample off by one: rounded variance 0), "var1" (two colours, rounded variance
    1), "busy" (256 values of noise) or an integer: exactly that many colours, far apart"""
    sc, mid = 1 << (bd - 8), 128 << (bd - 8)
    if kind == "flat": return np.full((16, 16), mid)
    if kind == "var0":
        b = np.full(256, mid); b[int(rng.integers(0, 256))] += 1
        return b.reshape(16, 16)
    if kind == "var1":
        b = np.repeat([mid - sc, mid + sc], 128)
        return rng.permutation(b).reshape(16, 16)
    if kind == "busy": return rng.integers(0, 1 << bd, (16, 16))
    lv = np.arange(kind) * (200 // kind) * sc + 3
    b = lv[rng.integers(0, kind, 256)]; b[rng.permutation(256)[:kind]] = lv
    return b.reshape(16, 16)


def sc_picture(dtype, bd, w, h, kinds, rng, pad=0):
    """a w x h picture (a view with `pad` more columns in a row) whose whole 16 x 16 blocks are `kinds` in raster order, then "busy"; what lies outside the whole
    blocks is two-colour content that would count if it were looked at"""
    base = rng.integers(0, 1 << bd, (h, w + pad)).astype(dtype)
    pic = base[:, :w]
    pic[...] = np.where(rng.integers(0, 2, (h, w)) == 1, 7, 200)
    i = 0
    for r in range(0, h - 15, 16):
        for c in range(0, w - 15, 16):
            pic[r:r + 16, c:c + 16] = sc_block(kinds[i] if i < len(kinds) else "busy", bd, rng); i += 1
    return pic


def sc_pictures(dtype, bd):
    """[(name, picture, what the four outputs must be when it is known by construction, else None)]"""
    rng = np.random.default_rng(5 + bd)
    out = []
    # 160 x 96 = 6 * 2560: counts_1 one below, on and one above the first threshold; 192 x 96 = 6 * 3072 with counts_1 = 9: counts_2 the same around the second
    for c1 in (5, 6, 7):
        out.append((f"counts_1={c1} of 160x96", sc_picture(dtype, bd, 160, 96, [2] * c1, rng, pad=(c1 - 5) * 16), [c1, c1, int(c1 > 6), int(c1 > 6)]))
    for c2 in (5, 6, 7):
        out.append((f"counts_2={c2} of 192x96", sc_picture(dtype, bd, 192, 96, ["var1"] * c2 + ["var0"] * (9 - c2), rng, pad=c2), [9, c2, 1, int(c2 > 6)]))
    out.append(("4 and 5 colours", sc_picture(dtype, bd, 64, 16, [4, 5, 1, 3], rng), [2, 2, 1, 1]))
    out.append(("var 0 and var 1", sc_picture(dtype, bd, 48, 32, ["var0", "var1", "flat", "var0", "var1", 2], rng, pad=3), [5, 3, 1, 1]))
    out.append(("16x16", sc_picture(dtype, bd, 16, 16, [2], rng), [1, 1, 1, 1]))
    out.append(("175x101, no multiple of 16", sc_picture(dtype, bd, 175, 101, [2, "var0", 3, "busy", 4, 5, "var1"] * 8, rng, pad=9), None))
    out.append(("15x40: no whole block", sc_picture(dtype, bd, 15, 40, [], rng), [0, 0, 0, 0]))
    out.append(("512x288", sc_picture(dtype, bd, 512, 288, ([2, "busy", "var0", 4, "busy", "var1", 5] * 90)[:576], rng, pad=64), None))
    return out
