"""CPU: the numpy restatement of the intra-block-copy hash table and hash search (tests/ibc_hash_common.py) against the reference, the conditions its case lists
exist for, and the library's host forms against the restatement.

What the reference exports with plain arguments is called through ctypes: the CRC, the table's inserter and its count, the variances, mv_err_cost.  The two
generators, svt_av1_get_block_hash_value and av1_is_dv_valid take PictureControlSet / IntraBcContext / MacroBlockD pointers whose offsets a test cannot know;
they are pinned by tests/golden/ibc_hash.npz, the way resize_planes.npz was made: a throw-away C program outside the repository, built against the reference's
headers, called them on the pictures of ibc_hash_common.SMALL (8-bit, and 12 x 9 / 20 x 18 also as 16-bit samples at depth 10), on block positions of every
size, and on 1392 (dv, position, tile, superblock size) cases chosen so that every rule of av1_is_dv_valid decides at least 58 of them; the file keeps inputs and
results only, valid regions only (of 136 x 130 below size 128: every 5th row and 7th column)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ibc_hash_common as I
from conftest import ROOT, ptr

GOLDEN = os.path.join(ROOT, "tests", "golden", "ibc_hash.npz")
FORMATS = [(np.uint8, 8), (np.uint16, 8), (np.uint16, 10)]


# ------------------------------------------------------------------------------------------------------------------ the reference's exports
def test_crc_equals_the_reference(ref):
    rng = np.random.default_rng(0)
    for which, poly in enumerate(I.POLYS):
        calc = (C.c_uint32 * 260)()   # CRC_CALCULATOR
        ref.svt_av1_crc_calculator_init(calc, 24, poly)
        ref.svt_av1_get_crc_value.restype = C.c_uint32
        for length in (4, 8, 16):
            data = rng.integers(0, 256, (200, length)).astype(np.uint8)
            data[0] = 0; data[1] = 255
            want = [ref.svt_av1_get_crc_value(calc, ptr(np.ascontiguousarray(row)), length) for row in data]
            assert I.crc(which, data).tolist() == want


class Vector(C.Structure):
    _fields_ = [("size", C.c_size_t), ("capacity", C.c_size_t), ("element_size", C.c_size_t), ("data", C.c_void_p)]


def ref_table(ref, pyr, w, h):
    """svt_av1_hash_table_create and the six svt_av1_add_to_hash_map_by_row_with_precal_data calls on the restatement's planes -> (counts, {bucket: entries})"""
    lookup = C.POINTER(C.POINTER(Vector))()   # HashTable: one member, p_lookup_table
    assert ref.svt_av1_hash_table_create(C.byref(lookup)) == 0
    for size in I.SIZES:
        if size not in pyr: continue
        full = {k: np.zeros((h, w), np.uint32 if k[0] == "h" else np.int8) for k in ("h1", "h2", "s2")}
        ny, nx = pyr[size]["h1"].shape
        for k in full: full[k][:ny, :nx] = pyr[size][k]
        hashes = (C.c_void_p * 2)(full["h1"].ctypes.data, full["h2"].ctypes.data)
        ref.svt_av1_add_to_hash_map_by_row_with_precal_data(C.byref(lookup), hashes, ptr(full["s2"]), w, h, size)
    counts, buckets = np.zeros(I.N_BUCKETS, np.int64), {}
    ref.svt_av1_hash_table_count.restype = C.c_int32
    used = np.nonzero(np.frombuffer(C.string_at(lookup, 8 * I.N_BUCKETS), np.uint64))[0].tolist()
    for k in used:
        v = lookup[k].contents
        assert v.element_size == 8 and (k % 97 or ref.svt_av1_hash_table_count(C.byref(lookup), k) == v.size)
        counts[k] = v.size
        buckets[k] = np.frombuffer(C.string_at(v.data, 8 * v.size), I.ENTRY_DTYPE).copy()
    ref.svt_av1_hash_table_destroy(C.byref(lookup))
    return counts, buckets


@pytest.fixture(scope="module")
def tables():
    """{(picture, dtype name, bd): (plane, pyramid, bucket_start, entries)} of the restatement"""
    out = {}
    for name, pic in I.table_pictures().items():
        for dtype, bd in FORMATS:
            plane = I.as_format(pic, dtype, bd)
            pyr = I.pyramid(plane)
            out[name, np.dtype(dtype).name, bd] = (plane, pyr) + I.table(pyr)
    return out


def test_table_and_bucket_order_equal_the_reference(ref, tables):
    for key, (plane, pyr, start, entries) in tables.items():
        if key[2] == 8 and key[1] == "uint16": continue   # the same hashes as uint16 at depth 10 would give no new order
        h, w = plane.shape
        counts, buckets = ref_table(ref, pyr, w, h)
        assert (np.diff(start) == counts).all(), key
        for k, e in buckets.items():
            assert (entries[start[k]:start[k + 1]] == e).all(), (key, k)


def test_variance_and_cost_equal_the_reference(ref):
    rng = np.random.default_rng(1)
    for n in I.SIZES:
        f = getattr(ref, "svt_aom_variance%dx%d_c" % (n, n)); f.restype = C.c_uint32
        for lo, hi in ((0, 256), (0, 2), (250, 256)):
            a, b = (np.ascontiguousarray(rng.integers(lo, hi, (n, n + 3)).astype(np.uint8)) for _ in range(2))
            for x, y in ((a, b), (a, 255 - a), (a, a)):
                sse = C.c_uint32()
                assert f(ptr(x), n + 3, ptr(y), n + 3, C.byref(sse)) == I.variance(x[:, :n], y[:, :n], 8), (n, lo, hi)
    jc, cc = I.cost_tables()
    comp = np.ascontiguousarray(cc)
    mid = (C.c_void_p * 2)(comp[0].ctypes.data + 4 * I.MV_MAX, comp[1].ctypes.data + 4 * I.MV_MAX)   # mvcost[i] points at difference 0
    for _ in range(300):
        mv, r = rng.integers(-1000, 1000, 2) * 8, rng.integers(-8000, 8000, 2)
        if rng.random() < .2: r[int(rng.integers(0, 2))] = mv[int(rng.integers(0, 2))]
        d = mv - r
        if np.abs(d).max() > I.MV_MAX: continue
        epb = int(rng.integers(1, 400))
        got = ref.mv_err_cost(ptr(mv.astype(np.int16)), ptr(r.astype(np.int16)), ptr(jc), mid, epb)
        assert got == I.mv_err_cost(int(d[0]), int(d[1]), jc, cc, epb)


# ------------------------------------------------------------------------------------------------------------------ the recorded results
def test_generators_block_hash_and_dv_rules_equal_the_recorded_reference():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 100 * 1024
    shapes = []
    for i in range(7):
        pic = g["pic%d" % i]
        h, w = pic.shape
        shapes.append((w, h, pic.dtype.itemsize))
        pyr = I.pyramid(pic)
        assert sorted(pyr) == sorted(int(k.split("_")[1]) for k in g.files if k.startswith("hash%d_" % i))
        for s, pl in pyr.items():
            sy, sx = (5, 7) if (w, h) == (136, 130) and s < 128 else (1, 1)
            assert (g["hash%d_%d" % (i, s)] == np.stack([pl["h1"], pl["h2"]])[:, ::sy, ::sx]).all(), (i, s)
            for k in range(2 if s == 2 else 3):
                assert (g["same%d_%d" % (i, s)][k] == pl["s%d" % k][::sy, ::sx]).all(), (i, s, k)
        for x, y, n, h1, h2 in g["blocks%d" % i].tolist():
            assert I.block_hash(pic, x, y, n) == (h1, h2), (i, x, y, n)
            assert pyr[n]["h1"][y, x] & 0xFFFF == h1 & 0xFFFF and pyr[n]["h2"][y, x] == h2   # ... which is the plane's value at that position
    assert shapes == [(w, h, 1) for w, h in I.SMALL[2:]] + [(12, 9, 2), (20, 18, 2)]
    rules = {}
    for (dv_row, dv_col, mi_row, mi_col, idx, rs, re, cs, ce, log2), valid in zip(g["dv"].tolist(), g["dv_valid"].tolist()):
        j = I.job(mi_col * 4, mi_row * 4, I.SIZES[idx], 1, tile=(rs, re, cs, ce), log2=log2)
        rule = I.dv_rule(j, j["x_pos"] + dv_col // 8, j["y_pos"] + dv_row // 8)
        assert (rule == 0) == bool(valid), (j, dv_row, dv_col)
        rules[rule, log2] = rules.get((rule, log2), 0) + 1
    assert all(sum(rules.get((r, l), 0) for l in (4, 5, 6, 7)) >= 58 for r in range(10)) and all(rules.get((0, l), 0) > 0 for l in (4, 5, 6, 7))


# ------------------------------------------------------------------------------------------------------------------ what the case lists exist for
def test_the_pictures_meet_their_conditions(tables):
    plane, pyr, start, entries = tables["noise", "uint8", 8]
    assert any(len(set(entries["hash_value2"][start[k]:start[k + 1]].tolist())) > 1 for k in np.nonzero(np.diff(start) > 1)[0])
    plane, pyr, start, entries = tables["tiled", "uint8", 8]
    big = np.nonzero(np.diff(start) > 64)[0]
    assert any(len(set(entries["hash_value2"][start[k]:start[k + 1]].tolist())) == 1 for k in big)
    plane, pyr, start, entries = tables["flat", "uint8", 8]
    assert len(entries) > 0
    for size in (4, 8, 16, 32):
        xs, ys = np.nonzero(pyr[size]["s2"].T)
        assert len(xs) and not (xs & (size - 1)).any() and not (ys & (size - 1)).any()
    for name, want in (("rows", (1, 0)), ("cols", (0, 1))):
        plane, pyr, start, entries = tables[name, "uint8", 8]
        for size in (2, 4, 8, 16, 32):
            assert (pyr[size]["s0"] == want[0]).all() and (pyr[size]["s1"] == want[1]).all(), (name, size)
    plane, pyr, start, entries = tables["text", "uint8", 8]
    assert np.diff(start).max() > 1000 and len(entries) > 300000


@pytest.fixture(scope="module")
def searches():
    out = []
    for c in I.search_cases():
        start, entries = I.table(I.pyramid(c["pic"]))
        jc, cc = I.cost_tables(zero=c["zero"])
        stats = {}
        want = [I.search(c["pic"], 8, start, entries, jc, cc, j, stats) for j in c["jobs"]]
        out.append(dict(c, start=start, entries=entries, jc=jc, cc=cc, want=want, stats=stats))
    return out


def test_the_search_list_meets_its_conditions(searches):
    stats = {}
    for c in searches:
        for k, v in c["stats"].items(): stats[k] = stats.get(k, 0) + v
    # every stage takes effect: a job stopped by count <= intra, entries passed over for hash_value2, by each rule of av1_is_dv_valid (the sub-pel rule cannot
    # reject whole-sample vectors), by each of the four limits, and by a difference outside the cost tables
    assert set(stats) >= {"stopped", "hash2", "table"} | {"dv%d" % r for r in range(1, 10)} | {"limit%d" % r for r in range(1, 5)}, stats
    jobs = [j for c in searches for j in c["jobs"]]
    assert {j["block_size"] for j in jobs} == set(I.SIZES) and {j["mib_size_log2"] for j in jobs} >= {4, 5} and {j["intra"] for j in jobs} == {0, 1}
    tiled = searches[0]
    h, w = tiled["pic"].shape
    assert any(j["y_pos"] + j["block_size"] == h for j in tiled["jobs"]) and any(j["x_pos"] + j["block_size"] == w for j in tiled["jobs"])
    assert any(r["found"] and r["n_valid"] > 64 for r in tiled["want"]) and any(r["count"] > 1 and not r["found"] for r in tiled["want"])
    zero = [c for c in searches if c["zero"]][0]
    assert sum(I.first_is_not_row_major(zero["pic"], 8, zero["start"], zero["entries"], j) for j in zero["jobs"]) >= 5


# ------------------------------------------------------------------------------------------------------------------ the host forms
def test_host_table_equals_the_restatement(pkg, tables):
    for key, (plane, pyr, start, entries) in tables.items():
        got_start, got_entries, info = pkg.ibc_hash_table_host(plane, bd=key[2])
        assert info.tolist() == [len(entries), 1] and (got_start == start).all() and (got_entries[:len(entries)] == entries).all(), key
        got_start, got_entries, info = pkg.ibc_hash_table_host(plane, capacity=len(entries) - 1, bd=key[2])
        assert info.tolist() == [len(entries), 0] and (got_start == start).all() and not got_entries.view(np.uint8).any(), key
    for w, h in I.SMALL:
        plane = I.small_picture(w, h)
        start, entries = I.table(I.pyramid(plane))
        got_start, got_entries, info = pkg.ibc_hash_table_host(plane)
        assert info.tolist() == [len(entries), 1] and (got_start == start).all() and (got_entries[:len(entries)] == entries).all(), (w, h)


@pytest.mark.parametrize("dtype,bd", FORMATS, ids=["u8", "u16_bd8", "u16_bd10"])
def test_host_search_equals_the_restatement(pkg, searches, dtype, bd):
    for c in searches:
        plane = I.as_format(c["pic"], dtype, bd)
        start, entries = (c["start"], c["entries"]) if bd == 8 and dtype == np.uint8 else I.table(I.pyramid(plane))
        jobs = c["jobs"] + [dict(c["jobs"][0], **b) for b in I.BAD_JOBS]
        want = [I.search(plane, bd, start, entries, c["jc"], c["cc"], j) for j in jobs]
        assert [r["count"] for r in want[len(c["jobs"]):]] == [-1] * len(I.BAD_JOBS)
        if bd == 8:   # 8-bit samples in 16-bit words: other hashes (and other chance meetings in a bucket), the same candidates and the same choice
            keys = ("n_valid", "found", "best_cost", "best_row", "best_col")
            assert [[r[k] for k in keys] for r in want[:len(c["jobs"])]] == [[r[k] for k in keys] for r in c["want"]]
        got = I.c_results(pkg.ibc_hash_search_host(plane, start, entries, c["jc"], c["cc"], I.c_jobs(pkg, jobs), bd=bd), len(jobs))
        for i, (g, r) in enumerate(zip(got, want)):
            assert g == r, (c["name"], i, jobs[i])


@pytest.mark.parametrize("dtype,bd", FORMATS, ids=["u8", "u16_bd8", "u16_bd10"])
def test_host_search_costs_real_differences(pkg, dtype, bd):
    """the hand-made table of ibc_hash_common.forged_case: variances other than 0"""
    plane, start, entries, jobs = I.forged_case(dtype, bd)
    jc, cc = I.cost_tables()
    want = [I.search(plane, bd, start, entries, jc, cc, j) for j in jobs]
    assert all(r["found"] and r["n_matched"] < r["count"] for r in want) and sum(r["best_cost"] > 1000 for r in want) == 3 and any(r["n_valid"] > 64 for r in want)
    assert I.c_results(pkg.ibc_hash_search_host(plane, start, entries, jc, cc, I.c_jobs(pkg, jobs), bd=bd), len(jobs)) == want


def test_variance_at_depth_10_is_the_scaled_form():
    """two 16-bit blocks far apart: sse needs more than 32 bits before it is scaled"""
    a, b = np.zeros((128, 128), np.uint16), np.full((128, 128), 1023, np.uint16)
    b[0, 0] = 1000
    d = a.astype(np.int64) - b
    sse, s = (int((d * d).sum()) + 8) >> 4, (int(d.sum()) + 2) >> 2
    assert int((d * d).sum()) > 1 << 32 and I.variance(a, b, 10) == sse - (s * s) // 16384 > 0


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_standalone_program(pkg, searches, flags, tmp_path):
    """csrc/ibc_hash.h in a program of its own (no Python, nothing preloaded) over the small pictures and the search cases: its table and results, byte for
    byte, against what the library's host forms gave here"""
    if flags:
        probe = tmp_path / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this compiler has no sanitizer runtime")
    exe = str(tmp_path / "ibc_hash_host_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "ibc_hash_host_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    runs = [(I.as_format(I.small_picture(w, h), dtype, bd), bd, [], *I.cost_tables()) for w, h in I.SMALL for dtype, bd in ((np.uint8, 8), (np.uint16, 10))]
    runs += [(c["pic"], 8, c["jobs"] + [dict(c["jobs"][0], **b) for b in I.BAD_JOBS], c["jc"], c["cc"]) for c in searches[:3]]
    runs.append((I.as_format(searches[0]["pic"], np.uint16, 10), 10, searches[0]["jobs"][::4], searches[0]["jc"], searches[0]["cc"]))
    for n, (plane, bd, jobs, jc, cc) in enumerate(runs):
        h, w = plane.shape
        start, entries, info = pkg.ibc_hash_table_host(plane, bd=bd)
        tab = I.c_jobs(pkg, jobs)
        res = pkg.ibc_hash_search_host(plane, start, entries, jc, cc, tab, bd=bd)
        path = str(tmp_path / ("run%d.bin" % n))
        with open(path, "wb") as f:
            f.write(np.array([plane.itemsize, bd, w, w, h, info[0], info[0] + (n % 3), len(jobs)], np.int32).tobytes())
            f.write(np.ascontiguousarray(plane).tobytes() + jc.tobytes() + cc.tobytes() + bytes(tab)[:C.sizeof(pkg.IbcSearchJob) * len(jobs)])
            f.write(start.tobytes() + entries[:info[0]].tobytes() + bytes(res)[:C.sizeof(pkg.IbcSearchResult) * len(jobs)])
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok "), (n, (r.stdout + r.stderr)[-3000:])
