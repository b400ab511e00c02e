"""CPU: what the super-resolution GPU tests rest on.  The library's host helpers against the reference's exports; the conditions of the upscale (tile columns,
phases, the table, both clips) shown on the reference itself; resize_filters.h against the reference's source text; and the Python restatement of the scaler
(tests/resize_common.py) against planes the reference's own av1_resize_plane / av1_highbd_resize_plane produced."""
import os
import re

import numpy as np
import pytest

import resize_common as rc

REF_ROOT = "/root/reference"
WIDTHS = list(range(1, 71)) + [352, 1920, 3840]


@pytest.fixture(scope="module")
def L(pkg):
    return pkg.lib()


@pytest.fixture(scope="module")
def refp(ref):
    return rc.prepare(ref)


# ---------------------------------------------------------------- host helpers
def test_scaled_dim_and_upscale_params_equal_the_reference(L, refp, pkg):
    import ctypes as C
    for denom in range(8, 17):
        for w in WIDTHS:
            small = L.svt_hip_superres_scaled_dim(w, denom)
            assert small == rc.ref_scaled_dim(refp, w, denom) == rc.scaled_dim(w, denom), (w, denom)
            step, x0 = C.c_int32(-1), C.c_int32(-1)
            assert L.svt_hip_superres_upscale_params(small, w, C.byref(step), C.byref(x0)) == 0
            assert step.value == rc.upscale_step(small, w) == ((small << 14) + w // 2) // w, (w, denom)
            assert x0.value == refp.get_upscale_convolve_x0(small, w, step.value) == rc.upscale_x0(small, w, step.value), (w, denom)
            assert 0 < step.value <= 1 << 14 and 0 <= x0.value < 1 << 14
    assert L.svt_hip_superres_scaled_dim(1920, 8) == 1920


# ---------------------------------------------------------------- conditions of the upscale
def _plane(seed, rows, w, dtype, bd):
    return np.random.default_rng(seed).integers(0, 1 << bd, (rows, w)).astype(dtype)


@pytest.mark.parametrize("dtype,bd", [(np.uint8, 8), (np.uint16, 10)])
def test_tile_columns_do_not_change_the_upscale(refp, dtype, bd):
    """svt_av1_upscale_normative_rows advances x0_qn by dst_width * step - (src_width << 14) per tile column and pads only the outer two: composed per column
    (1, 2 and 3 columns, at multiples of 4 source samples) it equals one call on the whole plane, and that equals the clamped whole-row form."""
    for w, denom in [(64, 9), (64, 13), (120, 11), (352, 16), (176, 15)]:
        small = rc.scaled_dim(w, denom)
        small -= small % 8   # the reference's last column ends at mi_cols * 4: stay on widths where that is the plane's width
        p = _plane(w * denom, 3, small, dtype, bd)
        whole = rc.ref_upscale(refp, p, w, bd, sentinel=7)
        assert np.array_equal(whole, rc.numpy_upscale(p, w, bd))
        # a column is at least a superblock wide; 8 samples already keep an unpadded column's 5 outer taps inside the row
        for bounds in ([], [small // 2 // 4 * 4], [small // 3 // 4 * 4, 2 * small // 3 // 4 * 4], [8], [small - 8]):
            assert np.array_equal(rc.ref_upscale_tiled(refp, p, w, denom, bounds, bd), whole), (w, denom, bounds)


def test_case_list_reaches_all_64_phases():
    seen = set()
    for w in rc.UPSCALE_WIDTHS:
        for d in rc.SUPERRES_DENOMS:
            seen |= rc.upscale_phases(w, w * d // 8)
    assert seen == set(range(64))


def test_normative_table_read_out_of_the_reference(refp):
    """An impulse of 128 on a floor of 1024 (16-bit samples at bd 12; a row of the table sums to 128, so the floor comes back as 1024 and no tap is clipped):
    output x minus 1024 is tap k of phase f wherever the window of x holds the impulse at position k.  Every (phase, tap) pair is met across the widths,
    consistently, and the 512 readings equal resize_filters.h."""
    got = np.full((64, 8), 1 << 20, np.int64)
    for in_w, out_w in [(64, 127), (90, 101), (129, 161), (61, 64)]:
        step = rc.upscale_step(in_w, out_w)
        x0 = refp.get_upscale_convolve_x0(in_w, out_w, step)
        for c in range(8, in_w - 8):
            p = np.full((1, in_w), 1024, np.uint16)   # a floor, so that negative taps stay above the clip at 0
            p[0, c] += 128
            out = rc.ref_upscale(refp, p, out_w, 12)[0].astype(np.int64) - 1024
            for x in range(out_w):
                q = x0 + x * step
                k = c - ((q >> 14) - 4)
                if 0 <= k < 8:
                    f = (q & 0x3fff) >> 8
                    assert got[f, k] in (1 << 20, out[x])
                    got[f, k] = out[x]
    assert np.array_equal(got, rc.TABLES["NORMATIVE"])


@pytest.mark.parametrize("dtype,bd", [(np.uint8, 8), (np.uint16, 8), (np.uint16, 10), (np.uint16, 12)])
def test_alternating_content_binds_both_clips(refp, dtype, bd):
    maxv = (1 << bd) - 1
    p = ((np.arange(90)[None, :] & 1) * maxv).astype(dtype).repeat(2, axis=0)
    step = rc.upscale_step(90, 101)
    q = rc.upscale_x0(90, 101, step) + np.arange(101) * step
    idx = np.clip((q >> 14)[:, None] - 4 + np.arange(8)[None, :], 0, 89)
    raw = ((p[0].astype(np.int64)[idx] * rc.TABLES["NORMATIVE"][(q & 0x3fff) >> 8]).sum(axis=1) + 64) >> 7
    assert raw.min() < 0 and raw.max() > maxv
    want = rc.ref_upscale(refp, p, 101, bd)
    assert np.array_equal(want, rc.numpy_upscale(p, 101, bd)) and want.min() == 0 and want.max() == maxv


# ---------------------------------------------------------------- the tables
def _c_numbers(path, name):
    txt = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    txt = re.sub(r"^\s*#.*$", "", re.sub(r"//.*$", "", txt, flags=re.M), flags=re.M)
    m = re.search(r"\b" + name + r"\s*(?:\[[^\]]*\]\s*)+=\s*\{(.*?)\}\s*;", txt, flags=re.S)
    return [int(v) for v in re.findall(r"-?\d+", m.group(1))]


def test_tables_equal_the_reference_source():
    if not os.path.isdir(REF_ROOT):
        pytest.skip("the reference's source is not here")
    resize_c = os.path.join(REF_ROOT, "Source", "Lib", "Encoder", "Codec", "EbResize.c")
    superres_h = os.path.join(REF_ROOT, "Source", "Lib", "Common", "Codec", "EbSuperRes.h")
    assert _c_numbers(superres_h, "av1_resize_filter_normative") == rc.TABLES["NORMATIVE"].reshape(-1).tolist()
    for band in ("875", "750", "625", "500"):
        assert _c_numbers(resize_c, "filteredinterp_filters" + band) == rc.TABLES[band].reshape(-1).tolist()
    assert _c_numbers(resize_c, "av1_down2_symeven_half_filter") == rc.TABLES["EVEN"]
    assert _c_numbers(resize_c, "av1_down2_symodd_half_filter") == rc.TABLES["ODD"]


def test_tables_are_filters():
    for name in rc.FILTER_NAMES:
        assert rc.TABLES[name].shape == (64, 8) and (rc.TABLES[name].sum(axis=1) == 128).all()
    assert 2 * sum(rc.TABLES["EVEN"]) == 128 and rc.TABLES["ODD"][0] + 2 * sum(rc.TABLES["ODD"][1:]) == 128


# ---------------------------------------------------------------- the restatement against the reference's own results
def test_restatement_equals_the_recorded_reference():
    """tests/golden/resize_planes.npz holds, for every case of resize_common.golden_shapes() in 8-bit samples and in 16-bit samples at bit depth 10, the input
    plane (resize_common.make_plane) and what the reference's av1_resize_plane / av1_highbd_resize_plane (static, Encoder/Codec/EbResize.c:456, :729) made of it.
    It was recorded once by a throw-away C program outside the repository that includes EbResize.c, links oracle/_ref/libsvtav1_ref.so, reads the input planes
    from a file and writes the output planes; only those planes are kept.  The restatement must reproduce them, and in doing so go through every range of
    down2_symeven, down2_symodd and interpolate_core and choose each of the five filter sets."""
    golden = rc.load_golden()
    rc.TAKEN.clear()
    for name, ih, iw, oh, ow, content in rc.golden_shapes():
        for t, dtype, bd in (("u8", np.uint8, 8), ("u16", np.uint16, 10)):
            src, want = golden[name, t]
            assert np.array_equal(src, rc.make_plane(name, ih, iw, content, dtype, bd)), name
            assert np.array_equal(rc.resize_plane(src, oh, ow, bd), want), (name, t)
    for fn in ("down2_symeven", "down2_symodd", "interpolate_core"):
        for rng in ("short", "initial", "middle", "end"):
            assert rc.TAKEN[fn, rng] > 0, (fn, rng)
    for name in rc.FILTER_NAMES:
        assert rc.TAKEN["filter", name] > 0, name


def test_clamped_form_equals_the_recorded_reference():
    """every range of every filter only leaves out clamps that cannot bind there: one form with both clamps (the device's) gives the same planes"""
    golden = rc.load_golden()
    for name, ih, iw, oh, ow, _ in rc.golden_shapes():
        for t, bd in (("u8", 8), ("u16", 10)):
            src, want = golden[name, t]
            assert np.array_equal(rc.numpy_resize_plane(src, oh, ow, bd), want), (name, t)
    for in_len, out_len in [(130, 77), (70, 45), (352, 235), (33, 70), (9, 2), (16384, 3)]:   # beyond the golden: against the function-for-function form
        line = np.random.default_rng(in_len).integers(0, 1024, (1, in_len))
        assert rc.numpy_multistep(line, out_len, 10)[0].tolist() == rc.resize_multistep(line[0].tolist(), in_len, out_len, 10), (in_len, out_len)


def test_golden_cases_are_the_issue_list():
    names = {c[0] for c in rc.golden_shapes()}
    for a, b in [(1, 1), (2, 1), (3, 2), (5, 3), (6, 3), (7, 4), (16, 16), (100, 25), (64, 15), (65, 16), (16, 24)]:
        assert f"row_{a}_{b}" in names and f"col_{a}_{b}" in names
    for w in (16, 17, 64, 353):
        for d in rc.SUPERRES_DENOMS:
            assert f"row_{w}_{rc.scaled_dim(w, d)}" in names
    assert rc.get_down2_steps(100, 25) == 2 and rc.get_down2_steps(64, 15) == 2 and rc.get_down2_steps(65, 16) == 2 and rc.get_down2_steps(16, 24) == 0
    assert rc.get_down2_steps(64, 32) == 1 and rc.get_down2_steps(17, 16) == 0 and rc.scaled_dim(17, 16) == 16 and rc.scaled_dim(353, 16) == 177
    assert os.path.getsize(rc.GOLDEN) < 100 * 1024


def test_checkerboard_clips_the_intermediate_plane():
    """the golden checkerboard: the row pass overshoots both ways, so a column pass fed with unclipped values gives another plane"""
    src, want = rc.load_golden()["checker_24x20_15x11", "u8"]
    rows_raw = []
    for r in src:
        line = [int(v) for v in r]
        # the row pass without its final clip: interpolate_core's sum, clipped far outside the sample range
        rows_raw.append(rc.interpolate_core(line, 24, 15, 20, rc.TABLES[rc.choose_interp_filter(24, 15)]))
    raw = np.array(rows_raw) - 0
    assert raw.max() > 255
    unclipped = np.stack([rc.resize_multistep([int(v) for v in raw[:, i]], 20, 11, 8) for i in range(15)], axis=1)
    assert not np.array_equal(unclipped, want)
