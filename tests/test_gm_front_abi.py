"""CPU: the entry points of the global-motion front half (corners, cross-correlation, correspondences) have their Context methods and the header compiles as C99
(declarations, exports and prototypes: tests/test_abi_binding.py), and calls the host can see to be wrong are refused with SVT_HIP_ERR_BAD_ARG before anything touches HIP (no device exists here: a call that reached the runtime would fail differently
or crash).  The same bad arguments with a live context are checked in tests/test_gm_front_gpu.py."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

BAD_ARG = 2   # SVT_HIP_ERR_BAD_ARG


def _header():
    return open(os.path.join(ROOT, "include", "svt_hip.h")).read()


def test_declared_exported_bound(pkg):
    hdr = _header()
    assert re.search(r"SVT_HIP_ERR_BAD_ARG\s*=\s*%d\b" % BAD_ARG, hdr)
    for m in ("gm_corners_batch", "gm_cross_correlation_batch", "gm_correspondences_batch"):
        assert hasattr(pkg.Context, m)
    assert int(re.search(r"#define SVT_HIP_GM_MAX_CORNERS (\d+)", hdr).group(1)) == pkg.GM_MAX_CORNERS == 4096
    assert "stay on the host" in hdr and not re.search(r"Corner detection, correspondences[^.]*stay on the host", hdr)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "svt_hip.h"\nint main(void){return (int)sizeof(&svt_hip_gm_corners_batch_dev) + (int)sizeof(&svt_hip_gm_cross_correlation_batch_dev) +'
                   " (int)sizeof(&svt_hip_gm_correspondences_batch_dev) + (int)sizeof(&svt_hip_gm_corners_scratch_bytes) + SVT_HIP_GM_MAX_CORNERS == 0;}\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_scratch_size(pkg):
    L = pkg.lib()

    def size(dims, n=None, plane=1, stride=None):
        tab = (pkg.GmRef * 10)()
        for i, (w, h) in enumerate(dims):
            tab[i] = pkg.GmRef(plane, w, h, stride or w, 0)
        return L.svt_hip_gm_corners_scratch_bytes(tab, len(dims) if n is None else n)

    one, three = size([(96, 80)]), size([(96, 80), (352, 288), (96, 80)])
    assert 96 * 80 + 4 * 80 <= one < 2 * 96 * 80 and three >= 2 * one + 352 * 288 and size([(16384, 16384)] * 9) >= 9 << 28
    # what svt_hip_gm_corners_batch_dev would refuse has no size
    assert size([(96, 80)], n=0) == 0 and size([(96, 80)] * 10) == 0 and size([(7, 80)]) == 0 and size([(96, 16385)]) == 0 and size([(96, 80)], plane=None) == 0
    assert size([(96, 80)], stride=95) == 0 and L.svt_hip_gm_corners_scratch_bytes(None, 1) == 0


# one thing wrong at a time; shared with the GPU test, which repeats them with a live context.  1 = "a valid pointer"
CORNERS_OK = dict(planes=1, n_planes=3, max_points=4096, d_points=1, d_counts=1, d_kept=1, d_scratch=1, plane=1, w=96, h=80, stride=96)
CORNERS_BAD = [dict(planes=None), dict(d_points=None), dict(d_counts=None), dict(d_scratch=None), dict(plane=None), dict(n_planes=0), dict(n_planes=10), dict(n_planes=-1),
               dict(max_points=0), dict(max_points=4097), dict(max_points=-1), dict(w=7), dict(h=7), dict(w=16385, stride=16385), dict(h=16385), dict(stride=95),
               dict(stride=-96)]
CORR_OK = dict(d_im1=1, stride1=96, d_im2=1, stride2=100, w=96, h=80, d_pairs=1, n=5, d_out=1)
CORR_BAD = [dict(d_im1=None), dict(d_im2=None), dict(d_pairs=None), dict(d_out=None), dict(n=-1), dict(n=(1 << 20) + 1), dict(w=7), dict(h=7),
            dict(w=16385, stride1=16385, stride2=16385), dict(h=16385), dict(stride1=95), dict(stride2=95)]
MATCH_OK = dict(d_src=1, src_stride=96, w=96, h=80, d_src_points=1, d_src_count=1, refs=1, n_refs=2, d_ref_points=1, d_ref_counts=1, max_points=4096, d_corr=1, d_ncorr=1,
                ref_plane=1, ref_stride=100)
MATCH_BAD = [dict(d_src=None), dict(d_src_points=None), dict(d_src_count=None), dict(refs=None), dict(d_ref_points=None), dict(d_ref_counts=None), dict(d_corr=None),
             dict(d_ncorr=None), dict(ref_plane=None), dict(n_refs=0), dict(n_refs=9), dict(n_refs=-1), dict(max_points=0), dict(max_points=4097), dict(w=7), dict(h=7),
             dict(w=16385, src_stride=16385, ref_stride=16385), dict(h=16385), dict(src_stride=95), dict(ref_stride=95)]


def _q(a, p):
    return lambda k: p if a[k] == 1 else a[k]


def call_corners(pkg, L, ctx, p, **chg):
    """`p` stands in for every pointer that is 1 in the OK set"""
    a = dict(CORNERS_OK); a.update(chg); q = _q(a, p)
    tab = (pkg.GmRef * 10)()
    for i in range(10):
        tab[i] = pkg.GmRef(q("plane"), a["w"], a["h"], a["stride"], 0)
    return L.svt_hip_gm_corners_batch_dev(ctx, tab if a["planes"] == 1 else None, a["n_planes"], a["max_points"], q("d_points"), q("d_counts"), q("d_kept"),
                                          q("d_scratch"))


def call_correlation(L, ctx, p, **chg):
    a = dict(CORR_OK); a.update(chg); q = _q(a, p)
    return L.svt_hip_gm_cross_correlation_batch_dev(ctx, q("d_im1"), a["stride1"], q("d_im2"), a["stride2"], a["w"], a["h"], q("d_pairs"), a["n"], q("d_out"))


def call_match(pkg, L, ctx, p, **chg):
    a = dict(MATCH_OK); a.update(chg); q = _q(a, p)
    tab = (pkg.GmRef * 9)()
    for i in range(9):
        tab[i] = pkg.GmRef(q("ref_plane"), a["w"], a["h"], a["ref_stride"], 0)
    return L.svt_hip_gm_correspondences_batch_dev(ctx, q("d_src"), a["src_stride"], a["w"], a["h"], q("d_src_points"), q("d_src_count"), tab if a["refs"] == 1 else None,
                                                  a["n_refs"], q("d_ref_points"), q("d_ref_counts"), a["max_points"], q("d_corr"), q("d_ncorr"))


def test_null_context_and_bad_arguments_are_refused(pkg):
    L = pkg.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p).value
    for c in [{}] + CORNERS_BAD:
        assert call_corners(pkg, L, None, p, **c) == BAD_ARG, c
    for c in [{}] + CORR_BAD:
        assert call_correlation(L, None, p, **c) == BAD_ARG, c
    for c in [{}] + MATCH_BAD:
        assert call_match(pkg, L, None, p, **c) == BAD_ARG, c
