"""The intra-block-copy hash table and hash search restated in numpy, and the case lists of the tests around them (tests/test_ibc_hash_ref_cpu.py pins the
restatement to the reference; tests/test_ibc_hash_gpu.py and the host-form tests compare the library with it).  File:line under Source/Lib of the reference:
  Encoder/Codec/hash.c:13-62                 the CRC
  Encoder/Codec/hash_motion.c:138-283        the two generators and the inserter
  Encoder/Codec/hash_motion.c:285-369        svt_av1_get_block_hash_value
  Encoder/Codec/EbAdaptiveMotionVectorPrediction.c:2003-2083   av1_is_dv_valid
  Encoder/Codec/av1me.c:273-282, :320-342, :1346-1403          mv_err_cost, is_mv_in, svt_av1_get_mvpred_var, the hash search
Planes hold valid regions only: the plane of block size s of a w x h picture has shape (h - s + 1, w - s + 1)."""
import numpy as np

POLYS = (0x5D6DCB, 0x864CFB)
SIZES = (4, 8, 16, 32, 64, 128)
N_BUCKETS = 1 << 19
MV_MAX, MV_VALS = 16383, 32767
INT32_MAX = (1 << 31) - 1
ENTRY_DTYPE = [("x", "<i2"), ("y", "<i2"), ("hash_value2", "<u4")]
JOB_FIELDS = ("x_pos", "y_pos", "block_size", "intra", "col_min", "col_max", "row_min", "row_max", "ref_mv_row", "ref_mv_col", "error_per_bit", "mi_row_start", "mi_row_end",
              "mi_col_start", "mi_col_end", "mib_size_log2")
RESULT_FIELDS = ("count", "n_matched", "n_valid", "found", "best_cost", "best_row", "best_col")


def crc_table(poly, bits=24):
    """crc_calculator_init_table, as the reference keeps it: 32-bit entries whose bits above `bits` are not masked"""
    tab = np.zeros(256, np.uint32)
    high = 1 << (bits - 1)
    for value in range(256):
        r = 0
        for k in range(7, -1, -1):
            if value & (1 << k): r ^= high
            r = ((r << 1) ^ poly if r & high else r << 1) & 0xFFFFFFFF
        tab[value] = r
    return tab


TABLES = tuple(crc_table(p) for p in POLYS)


def crc(which, data):
    """svt_av1_get_crc_value of every row of `data` (uint8 [..., length]) -> uint32 [...]"""
    tab, data = TABLES[which], np.asarray(data, np.uint8)
    r = np.zeros(data.shape[:-1], np.uint32)
    for i in range(data.shape[-1]):
        r = (r << np.uint32(8)) ^ tab[((r >> np.uint32(16)) ^ data[..., i]) & np.uint32(0xFF)]
    return r & np.uint32(0xFFFFFF)


def _bytes(words):
    """[..., k] little-endian words of any unsigned type -> uint8 [..., k * itemsize]: memory order"""
    w = np.ascontiguousarray(words).astype(words.dtype.newbyteorder("<"))
    return w.view(np.uint8).reshape(w.shape[:-1] + (-1,))


def level2(plane):
    """svt_av1_generate_block_2x2_hash_value -> dict(h1, h2, s0, s1) of shape (h - 1, w - 1)"""
    p = [plane[:-1, :-1], plane[:-1, 1:], plane[1:, :-1], plane[1:, 1:]]
    b = _bytes(np.stack(p, -1))
    return dict(h1=crc(0, b), h2=crc(1, b), s0=((p[0] == p[1]) & (p[2] == p[3])).astype(np.int8), s1=((p[0] == p[2]) & (p[1] == p[3])).astype(np.int8))


def level_up(src, size):
    """svt_av1_generate_block_hash_value: the planes of `size` from those of size / 2"""
    half, quad = size >> 1, size >> 2
    ny, nx = src["h1"].shape[0] - half, src["h1"].shape[1] - half
    at = lambda a, dy, dx: a[dy:dy + ny, dx:dx + nx]
    out = {}
    for k, which in (("h1", 0), ("h2", 1)):
        c = src[k]
        out[k] = crc(which, _bytes(np.stack([at(c, 0, 0), at(c, 0, half), at(c, half, 0), at(c, half, half)], -1)))
    r, c = src["s0"], src["s1"]
    out["s0"] = (at(r, 0, 0) & at(r, 0, quad) & at(r, 0, half) & at(r, half, 0) & at(r, half, quad) & at(r, half, half)).astype(np.int8)
    out["s1"] = (at(c, 0, 0) & at(c, 0, half) & at(c, quad, 0) & at(c, quad, half) & at(c, half, 0) & at(c, half, half)).astype(np.int8)
    ys, xs = np.mgrid[0:ny, 0:nx]
    out["s2"] = (((out["s0"] == 0) & (out["s1"] == 0)) | (((xs & (size - 1)) == 0) & ((ys & (size - 1)) == 0))).astype(np.int8)
    return out


def pyramid(plane, top=128):
    """{block size: planes} for 2, 4, ... up to `top`, as far as the picture has room; empty regions are left out"""
    h, w = plane.shape
    out = {}
    if h < 2 or w < 2: return out
    out[2] = level2(plane)
    s = 4
    while s <= top and s <= h and s <= w:
        out[s] = level_up(out[s >> 1], s)
        s *= 2
    return out


def column_major(planes, size):
    """what the inserter feeds the table for one size, in its order (x ascending, then y): (keys, x, y, hash2)"""
    xs, ys = np.nonzero(planes["s2"].T)
    return (planes["h1"][ys, xs] & 0xFFFF) + (SIZES.index(size) << 16), xs, ys, planes["h2"][ys, xs]


def table(pyr):
    """the six svt_av1_add_to_hash_map_by_row_with_precal_data calls as compressed rows -> (bucket_start int32[2^19 + 1], entries)"""
    keys, xs, ys, h2 = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.uint32)]
    for size in SIZES:
        if size in pyr:
            k, x, y, v = column_major(pyr[size], size)
            keys.append(k.astype(np.int64)); xs.append(x); ys.append(y); h2.append(v)
    keys, xs, ys, h2 = (np.concatenate(a) for a in (keys, xs, ys, h2))
    order = np.argsort(keys, kind="stable")   # a bucket belongs to one size, and the sizes were appended in the reference's order
    start = np.zeros(N_BUCKETS + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(keys, minlength=N_BUCKETS))
    entries = np.zeros(len(keys), ENTRY_DTYPE)
    entries["x"], entries["y"], entries["hash_value2"] = xs[order], ys[order], h2[order]
    return start, entries


def block_hash(plane, x, y, n):
    """svt_av1_get_block_hash_value of the n x n block at (x, y): 2x2 blocks at even offsets, folded four to one -> (hash_value1 with the size bits, hash_value2)"""
    blk = plane[y:y + n, x:x + n]
    b = _bytes(np.stack([blk[0::2, 0::2], blk[0::2, 1::2], blk[1::2, 0::2], blk[1::2, 1::2]], -1))
    h = [crc(0, b), crc(1, b)]
    while h[0].shape[0] > 1:
        h = [crc(i, _bytes(np.stack([a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]], -1))) for i, a in enumerate(h)]
    return (int(h[0][0, 0]) & 0xFFFF) + (SIZES.index(n) << 16), int(h[1][0, 0])


def _cdiv(a, b):
    """C's integer division"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def dv_rule(j, ex, ey):
    """av1_is_dv_valid for job j and the entry at (ex, ey): 0 valid, else the rule that rejects -- 1 .. 4 the tile's top / left / bottom / right edge, 5 / 6 the
    sub-8x8 chroma rules, 7 the coded-superblock delay, 8 the wavefront, 9 the software wavefront"""
    bw = bh = j["block_size"]
    mi_row, mi_col = j["y_pos"] // 4, j["x_pos"] // 4
    dv_row, dv_col = 8 * (ey - j["y_pos"]), 8 * (ex - j["x_pos"])
    assert not (dv_row & 7 or dv_col & 7)
    src_top, tile_top = mi_row * 32 + dv_row, j["mi_row_start"] * 32
    if src_top < tile_top: return 1
    src_left, tile_left = mi_col * 32 + dv_col, j["mi_col_start"] * 32
    if src_left < tile_left: return 2
    src_bottom, tile_bottom = (mi_row * 4 + bh) * 8 + dv_row, j["mi_row_end"] * 32
    if src_bottom > tile_bottom: return 3
    src_right, tile_right = (mi_col * 4 + bw) * 8 + dv_col, j["mi_col_end"] * 32
    if src_right > tile_right: return 4
    if (mi_row & 1) and (mi_col & 1):   # is_chroma_reference at 4:2:0 of a block one mi wide; wider blocks always are, and have bw >= 8
        if bw < 8 and src_left < tile_left + 32: return 5
        if bh < 8 and src_top < tile_top + 32: return 6
    log2 = j["mib_size_log2"]
    sb_size = (1 << log2) * 4
    active_sb_row, active_sb64_col = mi_row >> log2, (mi_col * 4) >> 6
    src_sb_row, src_sb64_col = _cdiv((src_bottom >> 3) - 1, sb_size), ((src_right >> 3) - 1) >> 6
    total = ((j["mi_col_end"] - j["mi_col_start"] - 1) >> 4) + 1
    if src_sb_row * total + src_sb64_col >= active_sb_row * total + active_sb64_col - 4: return 7
    gradient = 1 + 4 + (sb_size > 64)
    if src_sb_row > active_sb_row or src_sb64_col >= active_sb64_col - 4 + gradient * (active_sb_row - src_sb_row): return 8
    if sb_size == 64:
        if src_sb64_col > active_sb64_col + (active_sb_row - src_sb_row): return 9
    elif (((src_right >> 3) - 1) >> 7) > ((mi_col * 4) >> 7) + (active_sb_row - src_sb_row): return 9
    return 0


def mv_limit_rule(j, row, col):
    """is_mv_in: 0 inside, else 1 .. 4 for col_min, col_max, row_min, row_max"""
    if col < j["col_min"]: return 1
    if col > j["col_max"]: return 2
    if row < j["row_min"]: return 3
    if row > j["row_max"]: return 4
    return 0


def mv_err_cost(d_row, d_col, joint_cost, comp_cost, error_per_bit):
    joint = (0 if d_col == 0 else 1) if d_row == 0 else (2 if d_col == 0 else 3)
    cost = int(joint_cost[joint]) + int(comp_cost[0][MV_MAX + d_row]) + int(comp_cost[1][MV_MAX + d_col])
    return (cost * error_per_bit + (1 << 13)) >> 14


def variance(a, b, bd):
    """svt_aom_variance{n}x{n}_c; at bit depth 10 the form of svt_aom_highbd_10_variance{n}x{n}_c"""
    d = a.astype(np.int64) - b.astype(np.int64)
    s, sse, n2 = int(d.sum()), int((d * d).sum()), d.size
    if bd == 8: return ((sse & 0xFFFFFFFF) - (_cdiv(s * s, n2) & 0xFFFFFFFF)) & 0xFFFFFFFF
    sse10, sum10 = ((sse + 8) >> 4) & 0xFFFFFFFF, (s + 2) >> 2
    return max(sse10 - _cdiv(sum10 * sum10, n2), 0)


def _as_int32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def job_ok(j, w, h):
    return (j["block_size"] in SIZES and j["x_pos"] >= 0 and j["y_pos"] >= 0 and j["x_pos"] <= w - j["block_size"] and j["y_pos"] <= h - j["block_size"] and
            0 <= j["mib_size_log2"] <= 16 and all(0 <= j[k] <= 1 << 20 for k in ("mi_row_start", "mi_row_end", "mi_col_start", "mi_col_end")))


def search(plane, bd, start, entries, joint_cost, comp_cost, j, stats=None):
    """the hash search of svt_av1_full_pixel_search for one job -> a result dict.  `stats`, a dict, counts why entries were passed over"""
    h, w = plane.shape
    empty = lambda count: dict(count=count, n_matched=0, n_valid=0, found=0, best_cost=INT32_MAX, best_row=0, best_col=0)
    if not job_ok(j, w, h): return empty(-1)
    n, x0, y0 = j["block_size"], j["x_pos"], j["y_pos"]
    key, hash2 = block_hash(plane, x0, y0, n)
    first, count = int(start[key]), int(start[key + 1] - start[key])
    R = empty(count)
    note = (lambda k: stats.__setitem__(k, stats.get(k, 0) + 1)) if stats is not None else (lambda k: None)
    if count <= (1 if j["intra"] else 0):
        note("stopped")
        return R
    what = plane[y0:y0 + n, x0:x0 + n]
    for e in entries[first:first + count]:
        ex, ey = int(e["x"]), int(e["y"])
        if int(e["hash_value2"]) != hash2:
            note("hash2")
            continue
        R["n_matched"] += 1
        if j["intra"]:
            rule = dv_rule(j, ex, ey)
            if rule:
                note("dv%d" % rule)
                continue
        row, col = ey - y0, ex - x0
        rule = mv_limit_rule(j, row, col)
        if rule:
            note("limit%d" % rule)
            continue
        d_row, d_col = row * 8 - j["ref_mv_row"], col * 8 - j["ref_mv_col"]
        if max(abs(d_row), abs(d_col)) > MV_MAX:
            note("table")
            continue
        R["n_valid"] += 1
        cost = _as_int32(variance(what, plane[ey:ey + n, ex:ex + n], bd) + mv_err_cost(d_row, d_col, joint_cost, comp_cost, j["error_per_bit"]))
        if cost < R["best_cost"]:
            R.update(found=1, best_cost=cost, best_row=row, best_col=col)
    return R


# ---------------------------------------------------------------------------------------------------------------- pictures
def as_format(pic8, dtype, bd):
    """an 8-bit picture in the sample format under test: 16-bit samples at depth 10 get two more bits, so both bytes of a sample differ between samples"""
    p = pic8.astype(dtype)
    return ((p << 2) | (p & 3)).astype(dtype) if bd == 10 else p


def noise(w, h, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def flat(w, h, v=77):
    return np.full((h, w), v, np.uint8)


def row_stripes(w, h):
    """every row of one value, no two neighbouring rows alike: every block has its rows alike and its columns not"""
    return np.repeat(((np.arange(h) * 37 + 11) % 251).astype(np.uint8)[:, None], w, 1)


def col_stripes(w, h):
    return np.ascontiguousarray(row_stripes(h, w).T)


def tiled(w, h, seed=2):
    t = np.random.default_rng(seed).integers(0, 256, (8, 8)).astype(np.uint8)
    return np.tile(t, ((h + 7) // 8, (w + 7) // 8))[:h, :w].copy()


def text_like(w, h, seed=3):
    """a flat page with paragraphs of lines of 5 x 7 glyphs from a small alphabet in a few colours: repeated glyphs, long flat runs, sharp edges"""
    rng = np.random.default_rng(seed)
    pic = np.full((h, w), 235, np.uint8)
    glyphs = rng.integers(0, 2, (12, 7, 5)).astype(bool)
    for gy in range(4, h - 9, 10):
        if (gy // 10) % 7 == 6: continue   # a blank band between paragraphs: flat blocks on the grid in two neighbouring superblock rows
        ink = int(rng.choice([16, 40, 90]))
        for gx in range(4, w - 7, 6):
            g = int(rng.integers(0, 16))
            if g < 12: pic[gy:gy + 7, gx:gx + 5][glyphs[g]] = ink
    return pic


SMALL = [(1, 1), (3, 2), (4, 4), (5, 7), (12, 9), (20, 18), (136, 130)]   # (w, h) of the block-hash pictures


def small_picture(w, h):
    """a quarter noise, a quarter flat, the rest an 8 x 8 tile: every same_info value and both kinds of flag occur once the picture has room"""
    pic = tiled(w, h, seed=w * 1000 + h)
    pic[: h // 2, : w // 2] = noise(w // 2, h // 2, seed=w + h) if w > 1 and h > 1 else pic[: h // 2, : w // 2]
    pic[h // 2:, : w // 2] = 9
    return pic


def table_pictures():
    """{name: 8-bit picture} of the table tests"""
    return dict(noise=noise(160, 120), flat=flat(72, 40), rows=row_stripes(48, 40), cols=col_stripes(48, 40), tiled=tiled(200, 136), text=text_like(352, 240))


# ---------------------------------------------------------------------------------------------------------------- the search's jobs
def cost_tables(seed=5, zero=False):
    """(joint[4], comp[2][32767]): costs that grow with the magnitude, as the encoder's do, with a little noise so that no two differences cost the same"""
    if zero: return np.zeros(4, np.int32), np.zeros((2, MV_VALS), np.int32)
    rng = np.random.default_rng(seed)
    mag = np.abs(np.arange(-MV_MAX, MV_MAX + 1))
    comp = np.stack([(np.log2(mag + 1) * 512).astype(np.int32) + rng.integers(0, 64, MV_VALS).astype(np.int32) for _ in range(2)])
    return np.array([300, 900, 950, 1400], np.int32), comp


def job(x, y, n, intra=1, limits=None, ref_mv=(0, 0), epb=40, tile=None, log2=4, w=0, h=0):
    """limits (col_min, col_max, row_min, row_max), default wide open; tile (mi_row_start, mi_row_end, mi_col_start, mi_col_end), default the picture"""
    limits = limits or (-4096, 4096, -4096, 4096)
    tile = tile or (0, (h + 3) // 4, 0, (w + 3) // 4)
    return dict(zip(JOB_FIELDS, (x, y, n, intra) + tuple(limits) + tuple(ref_mv) + (epb,) + tuple(tile) + (log2,)))


def search_jobs(w, h):
    """the job list of a w x h picture whose content repeats with period 8 (tiled): every block size the picture has room for, positions on and off the 4-sample
    grid, the last block row and column, both superblock sizes (and the two values the reference's caller passes, its sb_size_log2), intra and inter, tight limits
    on each side, tiles that cut the picture, a reference vector that puts differences outside the tables"""
    jobs = []
    for n in SIZES:
        if n > w or n > h: continue
        spots = {(w - n, h - n), ((w - n) // 8 * 8, (h - n) // 8 * 8), (((w - n) // 2) & ~7, ((h - n) // 2) & ~7), (8, (h - n) // 8 * 8), ((w - n) // 8 * 8, 72 if h - n >= 72 else 0)}
        for x, y in sorted(spots):
            for log2 in (4, 5):
                jobs.append(job(x, y, n, 1, log2=log2, w=w, h=h))
            jobs.append(job(x, y, n, 0, w=w, h=h))
    x, y = (w - 8) // 8 * 8, (h - 8) // 8 * 8
    for n in (4, 8, 16):
        jobs += [job(x, y, n, 1, log2=6, w=w, h=h), job(x, y, n, 1, log2=7, w=w, h=h)]
        jobs += [job(x - 16, y - 16, n, 0, limits=lim, w=w, h=h) for lim in ((-24, 4096, -4096, 4096), (-4096, 8, -4096, 4096), (-4096, 4096, -16, 4096), (-4096, 4096, -4096, 0),
                                                                              (-24, 8, -16, 0))]
        jobs += [job(x, y, n, 1, tile=t, w=w, h=h) for t in ((8, (h + 3) // 4, 0, (w + 3) // 4), (0, (h + 3) // 4, 10, (w + 3) // 4), (0, (h + 3) // 4 - 4, 0, (w + 3) // 4),
                                                              (0, (h + 3) // 4, 0, (w + 3) // 4 - 4), (2, (h + 3) // 4, 6, (w + 3) // 4))]
        jobs.append(job(x, y, n, 0, ref_mv=(16000, 9000), w=w, h=h))
        jobs.append(job(x, y, n, 1, ref_mv=(-(y - 8) * 8 + 3, -(x - 16) * 8 - 5), epb=150, w=w, h=h))
    # 4 x 4 blocks at odd mi_row and mi_col in a tile that starts close by: the two chroma rules
    for tx, ty in ((x // 4 - 9, 1), (1, y // 4 - 9), (x // 4 - 9, y // 4 - 9)):
        jobs.append(job(x + 4, y + 4, 4, 1, tile=(ty, (h + 3) // 4, tx, (w + 3) // 4), w=w, h=h))
        jobs.append(job(x - 4, y - 4, 4, 1, tile=(ty, (h + 3) // 4, tx, (w + 3) // 4), log2=5, w=w, h=h))
    return jobs


def first_is_not_row_major(plane, bd, start, entries, j):
    """the job's valid candidates of the smallest cost under all-zero cost tables, in bucket order -> True when the first is not the one of the smallest (y, x)"""
    n, (key, hash2) = j["block_size"], block_hash(plane, j["x_pos"], j["y_pos"], j["block_size"])
    what = plane[j["y_pos"]:j["y_pos"] + n, j["x_pos"]:j["x_pos"] + n]
    e = entries[start[key]:start[key + 1]]
    ok = [(int(c["x"]), int(c["y"])) for c in e if int(c["hash_value2"]) == hash2 and not (j["intra"] and dv_rule(j, int(c["x"]), int(c["y"]))) and
          not mv_limit_rule(j, int(c["y"]) - j["y_pos"], int(c["x"]) - j["x_pos"])]
    cost = [variance(what, plane[y:y + n, x:x + n], bd) for x, y in ok]
    best = [p for p, c in zip(ok, cost) if c == min(cost)] if ok else []
    return len(best) >= 2 and best[0] != min(best, key=lambda p: (p[1], p[0]))


def search_cases():
    """[dict(name, pic (8-bit), jobs, zero)]: the tiled picture carries the grid of sizes, limits, tiles and superblock sizes; the noise picture the job that
    stops at count <= intra and the buckets that mix hash_value2; the text picture the wavefront rule (it needs six 64-sample columns) and, with all-zero cost
    tables, the jobs whose equal-cost candidates come in an order that differs between column-major and row-major"""
    cases = []
    pic = tiled(200, 136)
    cases.append(dict(name="tiled", pic=pic, jobs=search_jobs(200, 136), zero=False))
    # noise: every block is alone in the picture; some buckets hold two or more blocks all the same
    pic = noise(160, 120)
    h, w = pic.shape
    start, entries = table(pyramid(pic))
    jobs = [job(40, 40, 8, 1, w=w, h=h), job(41, 43, 16, 1, w=w, h=h), job(w - 4, h - 4, 4, 1, w=w, h=h)]
    sizes = np.diff(start)
    for k in np.nonzero(sizes >= 2)[0][:400:40]:
        e = entries[start[k]:start[k + 1]]
        if len(set(e["hash_value2"].tolist())) > 1:
            jobs += [job(int(c["x"]), int(c["y"]), SIZES[k >> 16], intra, w=w, h=h) for c in e[:2] for intra in (0, 1)]
    cases.append(dict(name="noise", pic=pic, jobs=jobs, zero=False))
    pic = text_like(352, 240)
    h, w = pic.shape
    jobs = [job(x, 132, 4, 1, log2=log2, w=w, h=h) for x in (0, 8, 60, 64, 200) for log2 in (4, 5)] + [job(x, 136, 4, 0, w=w, h=h) for x in (0, 348)]
    jobs += [job(4 + 6 * i, 4 + 10 * k, n, 0, w=w, h=h) for k in (0, 1, 9, 20) for i in (0, 7, 30, 56) for n in (4, 8)]
    jobs += [job(4 + 6 * i, 4 + 10 * k, 4, 1, limits=(-100, 100, -60, 60), w=w, h=h) for k in (9, 20) for i in (7, 30)]
    cases.append(dict(name="text", pic=pic, jobs=jobs, zero=True))
    cases.append(dict(name="text_costs", pic=pic, jobs=jobs[::3], zero=False))
    return cases


def forged_case(dtype, bd):
    """Two CRCs that agree mean equal blocks in practice, so a table built from the picture never leads to a variance other than 0.  This table is made by hand:
    the bucket of each job lists blocks that differ from the job's under the job's hash_value2 (and, for every other size, the job's own block somewhere in the
    middle), so the sums, the scaled form at depth 10 and the cost comparison all work on real differences.  -> (plane, bucket_start, entries, jobs)"""
    plane = as_format(noise(200, 136, seed=9), dtype, bd)
    h, w = plane.shape
    rng = np.random.default_rng(4)
    jobs, buckets = [], {}
    for i, n in enumerate(SIZES):
        x0, y0 = (w - n) // 2 + 1, (h - n) // 2
        jobs.append(job(x0, y0, n, 0, ref_mv=(8, -16), epb=60, w=w, h=h))
        key, hash2 = block_hash(plane, x0, y0, n)
        spots = [(int(rng.integers(0, w - n + 1)), int(rng.integers(0, h - n + 1))) for _ in range(100 if n == 8 else 5)]
        if i & 1: spots.insert(2, (x0, y0))
        buckets[key] = [(x, y, hash2 if k % 4 else hash2 ^ 1) for k, (x, y) in enumerate(spots, 1)]
    start, entries = np.zeros(N_BUCKETS + 1, np.int32), np.zeros(sum(len(b) for b in buckets.values()), ENTRY_DTYPE)
    for key, b in buckets.items(): start[key + 1] = len(b)
    start = np.cumsum(start).astype(np.int32)
    for key, b in buckets.items(): entries[start[key]:start[key + 1]] = np.array(b, ENTRY_DTYPE)
    return plane, start, entries, jobs


BAD_JOBS = [dict(block_size=2), dict(block_size=12), dict(block_size=256), dict(block_size=0), dict(x_pos=-1), dict(y_pos=-8), dict(x_pos=10 ** 6), dict(y_pos=10 ** 6),
            dict(mib_size_log2=-1), dict(mib_size_log2=17), dict(mi_row_start=-1), dict(mi_col_end=(1 << 20) + 1)]


def c_jobs(pkg, jobs):
    tab = (pkg.IbcSearchJob * len(jobs))()
    for i, j in enumerate(jobs):
        for k in JOB_FIELDS: setattr(tab[i], k, j[k])
    return tab


def c_results(res, n):
    return [{k: getattr(res[i], k) for k in RESULT_FIELDS} for i in range(n)]
