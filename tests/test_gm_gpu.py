"""GPU, bit for bit: the global-motion warp error, frame error, shear parameters and the device-side parameter walk against the reference's own exported
functions (svt_av1_warp_error, svt_av1_frame_error, svt_get_shear_params, svt_av1_refine_integerized_param) and the restatement of tests/gm_common.py.
The references are computed once per process and shared."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import gm_common as g
import test_gm_abi as abi
from conftest import ROOT

pytestmark = pytest.mark.gpu
ONE = g.ONE
ROT = g.ROT


def models_for(w, h):
    """about 40 models: identity, +-64 px translations (the window lies wholly outside the picture), the largest zoom / shear inside validity, random models inside
    what the bitstream carries, models far beyond it (clamped global path), invalid ones, one with wmmat[2] <= 0"""
    rng = np.random.default_rng(w * 1000 + h)
    ms = [(0, 0, ONE, 0, 0, ONE), ROT, (64 * ONE, 0, ONE, 0, 0, ONE), (-64 * ONE, 0, ONE, 0, 0, ONE), (0, 64 * ONE, ONE, 0, 0, ONE), (0, -64 * ONE, ONE, 0, 0, ONE),
          (64 * ONE, -64 * ONE, ONE + 512, -300, 300, ONE + 512), (-200 * ONE, 300 * ONE, ONE, 0, 0, ONE), (12345, -54321, ONE, 0, 0, ONE),
          (0, 0, ONE + 8191, 0, 0, ONE + 8191), (0, 0, ONE - 8192, 0, 0, ONE - 8192), (0, 0, ONE, 8191, -8191, ONE), (0, 0, ONE, -8192, 8192, ONE),
          (3 * ONE, ONE, ONE + 8191, 4000, -4000, ONE - 8192), (0, 0, ONE + 16320, 0, 0, ONE), (0, 0, ONE, 9300, 0, ONE), (0, 0, ONE, 0, 16000, ONE),
          (0, 0, ONE, 0, 0, ONE + 16000), (w * ONE // 2, 0, 2 * ONE - 2048, 0, 0, ONE), (0, 0, 20000, 0, 0, 2 * ONE),
          (0, 0, ONE + 16384, 0, 0, ONE), (0, 0, ONE, 9400, 0, ONE), (0, 0, 69536, 8000, -8000, 69536), (0, 0, ONE, 0, 16400, ONE),   # invalid
          (0, 0, 0, 0, 0, ONE), (0, 0, -ONE, 0, 0, ONE)]                                                                                  # wmmat[2] <= 0
    while len(ms) < 40:
        ms.append((int(rng.integers(-8 * ONE, 8 * ONE)), int(rng.integers(-8 * ONE, 8 * ONE)), ONE + int(rng.integers(-8192, 8192)), int(rng.integers(-8192, 8192)),
                   int(rng.integers(-8192, 8192)), ONE + int(rng.integers(-8192, 8192))))
    return ms


def device_models(pkg, L, ms):
    """GmModel array with the REFERENCE's shear parameters: the warp-error tests check the error kernel alone"""
    arr = (pkg.GmModel * len(ms))()
    for o, m in zip(arr, ms):
        a, b, c, d, ok = g.ref_shear(L, m)
        for k in range(6): o.mat[k] = m[k]
        o.alpha, o.beta, o.gamma, o.delta, o.valid = a, b, c, d, ok
    return arr


def ref_errors(L, ms, rf, src):
    return np.array([g.ref_warp_error(L, g.make_wm(list(m) + [0, 0]), rf, src) for m in ms], np.int64)


@functools.lru_cache(maxsize=None)
def _planes(w, h):
    return g.picture_pair(100 + w, w, h, ROT)


@pytest.mark.parametrize("w,h", [(96, 80), (100, 76), (90, 50)])
def test_warp_error_batch(hip, pkg, ref, w, h):
    src, rf = _planes(w, h)
    ms = models_for(w, h)
    want = ref_errors(ref, ms, rf, src)
    assert (want == 1).sum() >= 6 and (want > 1).sum() >= 25
    got = hip.gm_warp_error_batch(src, rf, device_models(pkg, ref, ms))
    assert np.array_equal(got, want), np.flatnonzero(got != want)


def test_warp_error_reference_of_another_size(hip, pkg, ref):
    src, rf = g.picture_pair(55, 96, 80, ROT, ref_size=(120, 70))
    ms = models_for(96, 80)[:24]
    assert np.array_equal(hip.gm_warp_error_batch(src, rf, device_models(pkg, ref, ms)), ref_errors(ref, ms, rf, src))


def test_warp_error_saturated_planes(hip, pkg, ref):
    w, h = 176, 144
    src, rf = np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    ms = [(0, 0, ONE, 0, 0, ONE), ROT, (64 * ONE, 0, ONE + 4096, 0, 0, ONE)]
    got = hip.gm_warp_error_batch(src, rf, device_models(pkg, ref, ms))
    assert list(got) == [16384 * w * h] * 3 and np.array_equal(got, ref_errors(ref, ms, rf, src))
    assert list(hip.gm_warp_error_batch(rf, src, device_models(pkg, ref, ms))) == [16384 * w * h] * 3


def test_warp_error_embedded_planes_read_nothing_outside(hip, pkg, ref):
    """the planes at an odd offset and stride inside larger buffers whose surroundings are filled twice with different values"""
    w, h = 100, 76
    src, rf = _planes(w, h)
    ms = models_for(w, h)
    want = ref_errors(ref, ms, rf, src)
    for fill in (0x11, 0xEE):
        big_s, big_r = np.full((h + 9, w + 37), fill, np.uint8), np.full((h + 12, w + 51), 255 - fill, np.uint8)
        vs, vr = big_s[5:5 + h, 3:3 + w], big_r[7:7 + h, 13:13 + w]
        vs[:], vr[:] = src, rf
        assert np.array_equal(hip.gm_warp_error_batch(vs, vr, device_models(pkg, ref, ms)), want), fill


@pytest.mark.parametrize("n", [0, 1, 37])
def test_warp_error_counts(hip, pkg, ref, n):
    src, rf = _planes(96, 80)
    ms = models_for(96, 80)[:n]
    got = hip.gm_warp_error_batch(src, rf, device_models(pkg, ref, ms))
    assert got.shape == (n,) and np.array_equal(got, ref_errors(ref, ms, rf, src))


def test_shear_params_batch(hip, pkg, ref):
    mats = g.shear_matrices(2000, seed=5)
    out = hip.gm_shear_params_batch(mats)
    bad = []
    for m, o in zip(mats, out):
        a, b, c, d, ok = g.ref_shear(ref, m)
        want = (a, b, c, d) if m[2] > 0 else (0, 0, 0, 0)
        if o.valid != ok or list(o.mat) != list(m) or (o.alpha, o.beta, o.gamma, o.delta) != want:
            bad.append(list(m))
    assert not bad, bad[:5]
    assert 200 < sum(o.valid for o in out) < len(mats) - 200
    assert len(hip.gm_shear_params_batch(np.zeros((0, 6), np.int32))) == 0


@pytest.mark.parametrize("n", [1, 8])
def test_frame_error_batch(hip, ref, n):
    w, h = 100, 76
    src = _planes(w, h)[0]
    refs = [g.picture_pair(200 + i, w, h, ROT)[1] for i in range(n)]
    if n == 8:
        refs[3] = src.copy(); refs[5] = 255 - src
        big = np.full((h + 3, w + 29), 0x77, np.uint8); big[2:2 + h, 11:11 + w] = refs[6]; refs[6] = big[2:2 + h, 11:11 + w]
    want = [g.ref_frame_error(ref, r, src) for r in refs]
    assert list(hip.gm_frame_error_batch(src, refs)) == want
    if n == 8:
        assert want[3] == 0


def make_jobs(pkg, specs):
    """specs: (ref index, wmtype, start, n_refinements, best_frame_error)"""
    jobs = (pkg.GmJob * len(specs))()
    for j, (ri, wmtype, start, n, bfe) in zip(jobs, specs):
        j.ref, j.wmtype, j.n_refinements, j.best_frame_error = ri, wmtype, n, bfe
        for k, v in enumerate(start): j.wmmat[k] = v
    return jobs


def check_result(out, want, rest):
    assert (list(out.wmmat), out.wmtype, out.best_error) == want
    assert (out.probes, out.invalid_probes) == (rest["probes"], rest["invalid"])
    assert out.rounds >= 1


@pytest.mark.parametrize("name", g.WALK_NAMES)
def test_refine_one_job(hip, pkg, ref, name):
    wk = g.walk_by_name(name)
    src, rf = g.walk_planes(wk)
    want, rest = g.walk_reference(ref, name)
    out, polls = hip.gm_refine_picture(src, [rf], make_jobs(pkg, [(0, wk["wmtype"], wk["start"], wk["n"], wk["bfe"])]))
    check_result(out[0], want, rest)
    assert polls >= 1


@functools.lru_cache(maxsize=None)
def _seven(L):
    """one source, seven reference planes of two sizes, seven jobs of all four types; expected results from the reference and the restatement"""
    w, h = 96, 80
    truths = [ROT, (2 * ONE, -ONE, ONE + 200, -150, 150, ONE + 200), (5 * ONE + 4096, 3 * ONE, ONE, 0, 0, ONE), (0, 0, ONE - 300, 250, -200, ONE + 100),
              (-3 * ONE, 2 * ONE, ONE + 64, 32, -32, ONE + 64), (0, 0, ONE, 0, 0, ONE), (ONE, ONE, ONE + 500, 400, -400, ONE + 500)]
    pairs = [g.picture_pair(1, w, h, t, ref_size=(112, 88) if i % 2 else None) for i, t in enumerate(truths)]
    src = pairs[0][0]
    refs = [p[1] for p in pairs]
    types = [g.ROTZOOM, g.AFFINE, g.TRANSLATION, g.AFFINE, g.ROTZOOM, g.IDENTITY, g.TRANSLATION]
    specs = []
    for i, (t, ty) in enumerate(zip(truths, types)):
        start = (t[0] + 2048 * (i - 3), t[1] - 1024 * i, t[2] + 8 * i, t[3] - 6 * i, t[4] + 4, t[5] - 10)
        specs.append((i, ty, start, 3 + i % 3, g.INT64_MAX if i != 4 else 5 * 10 ** 6))
    want = []
    for ri, ty, start, n, bfe in specs:
        want.append((g.ref_refine(L, start, ty, refs[ri], src, n, bfe), g.restated_walk(L, start, ty, refs[ri], src, n, bfe)))
        assert (want[-1][1]["wmmat"], want[-1][1]["wmtype"], want[-1][1]["error"]) == want[-1][0]
    return src, refs, specs, want


def test_refine_seven_jobs_on_seven_planes(hip, pkg, ref):
    src, refs, specs, want = _seven(ref)
    out, _ = hip.gm_refine_picture(src, refs, make_jobs(pkg, specs))
    for o, (wt, rest) in zip(out, want):
        check_result(o, wt, rest)
    assert len({o.rounds for o in out}) > 1   # jobs of one call end in different rounds


def test_refine_shuffled_jobs_and_planes(hip, pkg, ref):
    src, refs, specs, want = _seven(ref)
    order, planes = [4, 0, 6, 2, 5, 1, 3], [2, 5, 0, 6, 3, 1, 4]          # job order; plane i of the table is refs[planes[i]]
    table = [refs[p] for p in planes]
    shuffled = [(planes.index(specs[j][0]),) + specs[j][1:] for j in order]
    out, _ = hip.gm_refine_picture(src, table, make_jobs(pkg, shuffled))
    for o, j in zip(out, order):
        check_result(o, *want[j])


def test_refine_two_calls_back_to_back(hip, pkg, ref):
    src, refs, specs, want = _seven(ref)
    out, _ = hip.gm_refine_picture(src, refs, make_jobs(pkg, specs), repeat=2)
    for o, (wt, rest) in zip(out, want):
        check_result(o, wt, rest)


def test_refine_refuses_a_job_it_cannot_run(hip, pkg, ref):
    """jobs live in device memory: the device refuses what the host cannot see, and the other jobs of the call are not disturbed"""
    src, refs, specs, want = _seven(ref)
    specs = [specs[0], (7, g.ROTZOOM, ROT, 3, g.INT64_MAX), (-1, g.ROTZOOM, ROT, 3, g.INT64_MAX), (0, 4, ROT, 3, g.INT64_MAX), (0, g.AFFINE, ROT, 13, g.INT64_MAX),
             (0, g.AFFINE, ROT, -1, g.INT64_MAX), specs[1]]
    out, _ = hip.gm_refine_picture(src, refs, make_jobs(pkg, specs))
    check_result(out[0], *want[0]); check_result(out[6], *want[1])
    for o in out[1:6]:
        assert (o.wmtype, o.best_error, o.probes) == (-1, -1, 0)


def test_refine_no_jobs(hip, pkg):
    src, rf = _planes(96, 80)
    out, polls = hip.gm_refine_picture(src, [rf], make_jobs(pkg, []))
    assert len(out) == 0 and polls == 0


def test_golden_walk_needs_no_reference(hip, pkg):
    z = np.load(os.path.join(ROOT, "tests", "golden", "gm_walks.npz"))
    jobs = make_jobs(pkg, [(0, int(z["spec"][0]), [int(v) for v in z["start"]], int(z["spec"][1]), g.INT64_MAX)])
    out, _ = hip.gm_refine_picture(z["src"], [z["ref"]], jobs)
    assert list(out[0].wmmat) == list(z["wmmat"])
    assert [out[0].wmtype, out[0].best_error, out[0].probes, out[0].invalid_probes] == list(z["result"])
    start = [int(v) for v in z["start"]] + [0, 0]
    g.force_wmtype(start, int(z["spec"][0]))
    m = hip.gm_shear_params_batch(np.array([start[:6]], np.int32))
    assert list(hip.gm_warp_error_batch(z["src"], z["ref"], m)) == list(z["start_error"])


def test_bad_arguments_with_a_live_context(hip, pkg):
    L = pkg.lib()
    d = hip.empty(1 << 16)
    try:
        for c in abi.SHEAR_BAD:
            assert abi.call_shear(L, hip.h, d, **c) == abi.BAD_ARG, c
        for c in abi.WARP_BAD:
            assert abi.call_warp(L, hip.h, d, **c) == abi.BAD_ARG, c
        for c in abi.FRAME_BAD:
            assert abi.call_frame(pkg, L, hip.h, d, **c) == abi.BAD_ARG, c
        for c in abi.REFINE_BAD:
            assert abi.call_refine(pkg, L, hip.h, d, **c) == abi.BAD_ARG, c
        assert b"bad argument" in L.svt_hip_last_error(hip.h)
    finally:
        hip.free(d)
