"""CPU: the palette luma search and the screen-content detection against the reference, without a device.  search_palette_luma restated around the reference's
exported functions (tests/palette_common.py: ref_search) equals the same restatement around a plain numpy k-means (numpy_search) and the library's host form
(svt_hip_palette_search_host: csrc/palette.h, the arithmetic the kernel shares) on the whole case list, record for record and map byte for map byte; the host form
also runs in a program of its own under AddressSanitizer + UndefinedBehaviorSanitizer.  The conditions the case list has to meet are asserted here, from what
the numpy k-means records about itself, so that tests/test_palette_gpu.py -- which runs the same list -- provably exercises them.

Two conditions of the list cannot be met as first written, both because of n = 2.  "A block with all fourteen candidates kept": a candidate that starts from
n = 2 centroids has at most two distinct colours and the reference keeps a candidate only when palette_size > 2, so the two n = 2 slots are never kept and twelve
is the most a block can keep; the list has blocks that keep all twelve, which is asserted.  "For every n 2 .. 8 a clustering that reseeds an empty cluster":
k-means runs only when colors > 2, so ub - lb >= 2 and the two initial centroids lb + (ub - lb) / 4 and lb + 3 (ub - lb) / 4 differ; with c0 < c1 the sample lb is
never nearer to c1 and the sample ub is strictly nearer to c1, so neither cluster is empty; and the rounded mean of the lower cluster is at most its largest
value, below the smallest value, and so the rounded mean, of the upper one: c0 < c1 again.  A clustering of two never reseeds; the list reseeds at every n 3 .. 8,
and that it does not at 2 is asserted as well."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import palette_common as P
from conftest import ROOT


@pytest.fixture(scope="module")
def lists():
    """{(dtype, bd): (plane, jobs)}"""
    return {(np.dtype(t).name, bd): P.build_cases(t, bd) for t, bd in P.FORMATS}


@pytest.fixture(scope="module")
def by_numpy(lists):
    """{format: (results, backend)}: the backend carries the k-means records of the whole list, `per_job` the records of each job"""
    out = {}
    for key, (plane, jobs) in lists.items():
        be, res, per_job = P.NumpyBackend(), [], []
        for j in jobs:
            first = len(be.stats)
            res.append(P.numpy_search(plane, j, key[1], be))
            per_job.append(be.stats[first:])
        be.per_job = per_job
        out[key] = (res, be)
    return out


@pytest.fixture(scope="module")
def by_ref(ref, lists):
    return {key: [P.ref_search(ref, plane, j, key[1]) for j in jobs] for key, (plane, jobs) in lists.items()}


def test_numpy_search_equals_ref_search(by_numpy, by_ref):
    for key in by_ref:
        for i, (a, b) in enumerate(zip(by_numpy[key][0], by_ref[key])):
            assert P.same_result(a, b) is None, (key, i, P.same_result(a, b))


def _host(pkg, plane, jobs, bd, fill=0):
    tab, nbytes = P.c_jobs(pkg, jobs, spacing=5)
    res, cands = (pkg.PaletteResult * max(len(jobs), 1))(), (pkg.PaletteCand * (P.MAX_CANDS * max(len(jobs), 1)))()
    C.memset(res, fill, C.sizeof(res)); C.memset(cands, fill, C.sizeof(cands))
    maps = np.full(nbytes, fill, np.uint8)
    pkg.palette_search_host(plane, tab, res, cands, maps, bd=bd)
    return tab, res, cands, maps


def test_host_form_equals_both(pkg, lists, by_numpy, by_ref):
    for key, (plane, jobs) in lists.items():
        _, res, cands, maps = _host(pkg, plane, jobs, key[1], fill=0xA5)
        for i, j in enumerate(jobs):
            got = P.c_result(j, res, cands, maps, i)
            assert all(c["reserved"] == 0 for c in got["cands"])
            for want in (by_ref[key][i], by_numpy[key][0][i]):
                assert P.same_result(got, want) is None, (key, i, j, P.same_result(got, want))
        assert P.untouched(jobs, by_ref[key], res, cands, maps, 0xA5) is None


def test_host_form_bad_jobs_and_refusals(pkg, lists):
    plane, jobs = lists[("uint8", 8)]
    good = jobs[0]
    bad = [dict(good, bw=8, bh=64), dict(good, bw=12, bh=12), dict(good, bw=128, bh=128), dict(good, bw=4, bh=4), dict(good, bw=4, bh=8), dict(good, cols=0),
           dict(good, cols=good["bw"] + 1), dict(good, rows=0), dict(good, rows=good["bh"] + 1), dict(good, n_cache=17), dict(good, n_cache=-1), dict(good, step=0),
           dict(good, step=3), dict(good, x=-1), dict(good, y=-1)]
    seq = [dict(good)] + [dict(j) for b in bad for j in (b, good)]   # c_jobs notes each job's map_off in its dict
    _, res, cands, maps = _host(pkg, plane, seq, 8, fill=0x5A)
    want = P.numpy_search(plane, good, 8)
    results = []
    for i, j in enumerate(seq):
        if i % 2 == 0:
            assert P.same_result(P.c_result(j, res, cands, maps, i), want) is None, i
            results.append(want)
        else:
            assert (res[i].colors, res[i].n_cands) == (-1, 0), (i, j)
            results.append(dict(colors=-1, cands=[]))
    assert P.untouched(seq, results, res, cands, maps, 0x5A) is None
    L = pkg.lib()
    buf = (C.c_uint8 * 65536)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(pix_bytes=1, bd=8, plane=p, stride=64, jobs=p, njobs=0, results=p, cands=p, maps=p)
    call = lambda **chg: L.svt_hip_palette_search_host(*[dict(ok, **chg)[k] for k in ("pix_bytes", "bd", "plane", "stride", "jobs", "njobs", "results", "cands", "maps")])
    assert call() == 0
    for chg in (dict(plane=None), dict(jobs=None), dict(results=None), dict(cands=None), dict(maps=None), dict(njobs=-1), dict(stride=0), dict(stride=-64), dict(pix_bytes=0),
                dict(pix_bytes=3), dict(bd=10), dict(pix_bytes=2, bd=12), dict(pix_bytes=2, bd=9)):
        assert call(**chg) == 2, chg


def test_the_case_list_meets_its_conditions(lists, by_numpy):
    for key, (plane, jobs) in lists.items():
        res, be = by_numpy[key]
        colors = [r["colors"] for r in res]
        for lo, hi in ((1, 1), (2, 2), (3, 8), (9, 64), (65, 1 << 12)):
            assert any(lo <= c <= hi for c in colors), (key, "colours in", lo, hi)
        for k in range(3, 9):
            assert any(s["k"] == k and any(s["reseeds"]) for s in be.stats), (key, "no reseed at n =", k)
        assert not any(s["k"] == 2 and any(s["reseeds"]) for s in be.stats), (key, "a reseed at n = 2: see the module text")
        assert any(max(s["reseeds"], default=0) >= 2 for s in be.stats), (key, "two reseeds in one iteration")
        assert any(s["n"] == 4096 for s in be.stats) and any(s["iterations"] >= 5 for s in be.stats), key
        assert be.equidistant > 0, (key, "a sample equidistant from two centroids")
        assert not any(s["restored"] for s in be.stats), (key, "the this_dist > pre_dist branch was taken: the tests do not cover it")
        assert max(s["iterations"] for s in be.stats) < 50
        ties = False
        for j, r in zip(jobs, res):
            if 1 < r["colors"] <= 64:
                cnt = np.sort(np.bincount(plane[j["y"]:j["y"] + j["rows"], j["x"]:j["x"] + j["cols"]].ravel()))[::-1]
                ties = ties or any(cnt[i] == cnt[i + 1] > 0 for i in range(min(7, len(cnt) - 1)))
        assert ties, (key, "two colours of equal count among the top eight")
        assert any(c["size"] < c["n"] for r in res for c in r["cands"]), (key, "duplicates after rounding")
        assert all(len(r["cands"]) <= 12 for r in res) and any(len(r["cands"]) == 12 for r in res), (key, "every candidate with n >= 3 kept")
        slots = lambda j, r: len(range(min(r["colors"], 8), 1, -j["step"])) + min(r["colors"], 8) - 1
        assert any(1 < r["colors"] <= 64 and len(r["cands"]) < slots(j, r) for j, r in zip(jobs, res)), (key, "a candidate dropped because k <= 2")
        assert {len(j["cache"]) for j in jobs} >= {0, 1, 16}
        diffs = {abs(v - c) for j, r in zip(jobs, res) for cand in r["cands"] for v in cand["raw"][:cand["n"]] for c in j["cache"]}
        assert {0, 1, 2} <= diffs, (key, "centroid - cache differences of 0, 1 and 2")
        assert {(j["step"], r["colors"] & 1) for j, r in zip(jobs, res) if 2 < r["colors"] <= 64} >= {(2, 0), (2, 1), (1, 0), (1, 1)}
        for bw, bh in P.SHAPES:
            cuts = {(j["cols"] < bw, j["rows"] < bh) for j in jobs if (j["bw"], j["bh"]) == (bw, bh)}
            assert cuts == {(False, False), (True, False), (False, True), (True, True)}, (key, bw, bh)
            assert any((j["bw"], j["bh"], j["cols"], j["rows"]) == (bw, bh, 1, 1) for j in jobs)
        assert any(j["x"] & 1 for j in jobs) and any(not j["x"] & 1 for j in jobs) and plane.strides[0] > plane.shape[1] * plane.itemsize
        assert int(plane.max()) == (1 << key[1]) - 1
    assert lists[("uint16", 10)][0].max() == 1023


def test_two_slots_are_never_kept(lists, by_numpy):
    """n = 2 cannot give palette_size > 2: the fourteen slots of the ABI hold at most twelve candidates (see the module text)"""
    for key in lists:
        assert all(c["n"] >= 3 for r in by_numpy[key][0] for c in r["cands"])


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_standalone_program(pkg, lists, flags, tmp_path):
    """csrc/palette.h in a program of its own (no Python, nothing preloaded) over recorded jobs of every format: its outputs, byte for byte, against what the
    library's host form gave here"""
    if flags:
        probe = tmp_path / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this compiler has no sanitizer runtime")
    exe = str(tmp_path / "palette_host_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "palette_host_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    for key, (plane, jobs) in lists.items():
        pick = [j for i, j in enumerate(jobs) if i % 9 == 0 or j["bw"] * j["bh"] == 4096 and i % 2] + [dict(jobs[0], bw=5)]
        tab, res, cands, maps = _host(pkg, plane, pick, key[1], fill=0)
        root = np.ascontiguousarray(plane)
        path = str(tmp_path / f"{key[0]}_{key[1]}.bin")
        with open(path, "wb") as f:
            f.write(np.array([plane.itemsize, key[1], root.shape[1], root.shape[0], len(pick), len(maps)], np.int32).tobytes())
            f.write(root.tobytes() + bytes(tab)[:C.sizeof(pkg.PaletteJob) * len(pick)] + bytes(res) + bytes(cands) + maps.tobytes())
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout + r.stderr)[-3000:]


# ------------------------------------------------------------------------------------------------------------------ screen content
def numpy_screen_content(plane, bd):
    h, w = plane.shape
    c1 = c2 = 0
    for r in range(0, h - 15, 16):
        for c in range(0, w - 15, 16):
            b = plane[r:r + 16, c:c + 16].astype(np.int64)
            if not 1 < len(np.unique(b)) <= 4: continue
            d = b - (128 << (bd - 8))
            s, sse = int(d.sum()), int((d * d).sum())
            if bd == 8: var = sse - (s * s) // 256
            else:
                sse, s = (sse + 8) >> 4, (s + 2) >> 2
                var = max(0, sse - (s * s) // 256)
            c1 += 1; c2 += ((var + 128) >> 8) > 0
    cd = int(c1 * 2560 > w * h)
    return [c1, c2, cd, int(bool(cd and c2 * 3072 > w * h))]


@pytest.mark.parametrize("dtype,bd", [(np.uint8, 8), (np.uint16, 10)])
def test_screen_content_pictures(ref, dtype, bd):
    """the detection's pictures are what they are named after, by the reference's functions and by numpy"""
    pics = P.sc_pictures(dtype, bd)
    for name, pic, want in pics:
        got = P.ref_screen_content(ref, pic, bd)
        assert got == numpy_screen_content(pic, bd), name
        assert want is None or got == want, (name, got, want)
    named = {n: P.ref_screen_content(ref, p, bd) for n, p, _ in pics}
    # one below, on and one above either threshold: counts * 2560 (3072) against width * height
    assert [named[f"counts_1={c} of 160x96"][0] * 2560 - 160 * 96 for c in (5, 6, 7)] == [-2560, 0, 2560]
    assert [named[f"counts_2={c} of 192x96"][1] * 3072 - 192 * 96 for c in (5, 6, 7)] == [-3072, 0, 3072]
    assert [named[f"counts_1={c} of 160x96"][2] for c in (5, 6, 7)] == [0, 0, 1] and [named[f"counts_2={c} of 192x96"][3] for c in (5, 6, 7)] == [0, 0, 1]
    rng = np.random.default_rng(1)
    for kind, valid, var in ((4, True, None), (5, False, None), ("var0", True, 0), ("var1", True, 1), ("flat", False, None)):
        pic = P.sc_block(kind, bd, rng).astype(dtype)
        got = P.ref_screen_content(ref, pic, bd)
        assert got[0] == int(valid) and (var is None or got[1] == var), (kind, got)
    assert any(p.shape[0] % 16 and p.shape[1] % 16 for _, p, _ in pics) and max(p.shape[1] for _, p, _ in pics) <= 512 and max(p.shape[0] for _, p, _ in pics) <= 288
