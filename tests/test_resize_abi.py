"""CPU: the super-resolution entry points have their Context methods and the header compiles as C99 with them (declarations, exports and prototypes:
tests/test_abi_binding.py), the scratch size is monotone and 0 for what the call refuses, and calls the host can see to be wrong are refused with
SVT_HIP_ERR_BAD_ARG before anything touches HIP (no device exists here).  The same bad arguments with a live context: tests/test_superres_gpu.py."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

BAD_ARG = 2   # SVT_HIP_ERR_BAD_ARG


def test_declared_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "svt_hip.h")).read()
    assert re.search(r"SVT_HIP_ERR_BAD_ARG\s*=\s*%d\b" % BAD_ARG, hdr)
    for m in ("superres_upscale_planes", "resize_planes"):
        assert hasattr(pkg.Context, m)
    for f in ("svt_hip_superres_scaled_dim", "svt_hip_superres_upscale_params", "svt_hip_superres_upscale_planes_dev", "svt_hip_resize_scratch_bytes",
              "svt_hip_resize_planes_dev"):
        assert f in pkg.PROTOTYPES and hasattr(pkg.lib(), f)
    assert [n for n, _ in pkg.UpscalePlane._fields_] == ["d_src", "src_stride", "in_w", "d_dst", "dst_stride", "out_w", "rows"]
    assert [n for n, _ in pkg.ResizePlane._fields_] == ["d_src", "src_stride", "in_w", "in_h", "d_dst", "dst_stride", "out_w", "out_h"]


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "svt_hip.h"\nint main(void){SvtHipUpscalePlane u = {0}; SvtHipResizePlane r = {0}; u.rows = 2; r.out_h = 1;\n'
                   "return (int)sizeof(&svt_hip_superres_scaled_dim) + (int)sizeof(&svt_hip_superres_upscale_params) + (int)sizeof(&svt_hip_superres_upscale_planes_dev) +"
                   " (int)sizeof(&svt_hip_resize_scratch_bytes) + (int)sizeof(&svt_hip_resize_planes_dev) + u.rows + r.out_h == 0;}\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_host_helpers_refuse(pkg):
    L = pkg.lib()
    step, x0 = C.c_int32(), C.c_int32()
    assert L.svt_hip_superres_scaled_dim(1920, 7) == 0 and L.svt_hip_superres_scaled_dim(1920, 17) == 0 and L.svt_hip_superres_scaled_dim(0, 9) == 0
    assert L.svt_hip_superres_scaled_dim(65536, 9) == 0 and L.svt_hip_superres_scaled_dim(10, 16) == 10 and L.svt_hip_superres_scaled_dim(20, 16) == 16
    assert L.svt_hip_superres_upscale_params(16, 32, C.byref(step), C.byref(x0)) == 0 and step.value == 8192
    for in_w, out_w, a, b in [(0, 16, step, x0), (17, 16, step, x0), (16, 16385, step, x0), (16, 32, None, x0), (16, 32, step, None)]:
        assert L.svt_hip_superres_upscale_params(in_w, out_w, C.byref(a) if a is not None else None, C.byref(b) if b is not None else None) == BAD_ARG


def _resize_tab(pkg, shapes, src=1 << 20, dst=2 << 20, src_stride=None, dst_stride=None):
    tab = (pkg.ResizePlane * 4)()
    for i, (iw, ih, ow, oh) in enumerate(shapes):
        tab[i] = pkg.ResizePlane(src, src_stride or iw, iw, ih, dst, dst_stride or ow, ow, oh)
    return tab


def test_scratch_size(pkg):
    L = pkg.lib()

    def size(shapes, pix_bytes=1, n=None, **kw):
        return L.svt_hip_resize_scratch_bytes(pix_bytes, _resize_tab(pkg, shapes, **kw), len(shapes) if n is None else n)

    # nothing when the height stays (super-resolution scales the width alone); the row pass's result when both axes change; temporaries per column halving
    assert size([(352, 288, 235, 288)]) == 0 and size([(352, 288, 352, 288)]) == 0
    both = size([(48, 40, 30, 25)])
    assert 30 * 40 <= both < 30 * 40 + 256 and size([(48, 40, 48, 25)]) == 0
    assert 30 * 100 + 30 * 50 <= size([(48, 100, 30, 25)]) < 30 * 100 + 30 * 50 + 512       # two halvings: one temporary
    assert 30 * 100 + 30 * 50 + 30 * 25 <= size([(48, 100, 30, 12)]) < 30 * 100 + 30 * 50 + 30 * 25 + 768   # three stages: both
    # monotone in the input height, the output width, the sample size and the planes
    sizes = [size([(64, 64 + 8 * k, 40, 30)]) for k in range(8)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    sizes = [size([(64, 80, 20 + 8 * k, 30)]) for k in range(8)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert size([(48, 40, 30, 25)], pix_bytes=2) >= 2 * 30 * 40 > both
    assert size([(48, 40, 30, 25)] * 3) >= 3 * both and size([(16384, 16384, 16383, 16383)], pix_bytes=2) >= 2 * 16383 * 16384
    # what svt_hip_resize_planes_dev would refuse has no size
    ok = (48, 40, 30, 25)
    assert size([ok], n=0) == 0 and size([ok] * 4) == 0 and size([ok], pix_bytes=3) == 0 and size([ok], src=None) == 0 and size([ok], dst=None) == 0
    assert size([ok], src=4096, dst=4096) == 0 and size([ok], src_stride=47) == 0 and size([ok], dst_stride=29) == 0 and L.svt_hip_resize_scratch_bytes(1, None, 1) == 0
    for bad in [(0, 40, 30, 25), (48, 0, 30, 25), (48, 40, 0, 25), (48, 40, 30, 0), (16385, 40, 30, 25), (48, 16385, 30, 25), (48, 40, 16385, 25), (48, 40, 30, 16385)]:
        assert size([bad]) == 0, bad


# one thing wrong at a time; shared with the GPU test, which repeats them with a live context.  1 = "a valid pointer", 2 = "another valid pointer"
UPSCALE_OK = dict(pix_bytes=1, bd=8, planes=1, n_planes=3, d_src=1, src_stride=40, in_w=40, d_dst=2, dst_stride=64, out_w=64, rows=2)
UPSCALE_BAD = [dict(planes=None), dict(d_src=None), dict(d_dst=None), dict(d_dst=1), dict(n_planes=0), dict(n_planes=4), dict(n_planes=-1), dict(in_w=0), dict(in_w=-1),
               dict(out_w=39), dict(out_w=16385, dst_stride=16385), dict(rows=0), dict(rows=16385), dict(src_stride=39), dict(dst_stride=63), dict(pix_bytes=0),
               dict(pix_bytes=3), dict(bd=10), dict(pix_bytes=2, bd=7), dict(pix_bytes=2, bd=13)]
RESIZE_OK = dict(pix_bytes=1, bd=8, planes=1, n_planes=3, d_src=1, src_stride=48, in_w=48, in_h=40, d_dst=2, dst_stride=30, out_w=30, out_h=25, d_scratch=1, scratch_bytes=1 << 20)
RESIZE_BAD = [dict(planes=None), dict(d_src=None), dict(d_dst=None), dict(d_dst=1), dict(n_planes=0), dict(n_planes=4), dict(n_planes=-1), dict(in_w=0), dict(in_h=0),
              dict(out_w=0), dict(out_h=0), dict(in_w=16385, src_stride=16385), dict(in_h=16385), dict(out_w=16385, dst_stride=16385), dict(out_h=16385),
              dict(src_stride=47), dict(dst_stride=29), dict(d_scratch=None), dict(scratch_bytes=100), dict(pix_bytes=0), dict(pix_bytes=3), dict(bd=10),
              dict(pix_bytes=2, bd=7), dict(pix_bytes=2, bd=13)]


def _q(a, p, p2):
    return lambda k: {1: p, 2: p2}.get(a[k], a[k]) if a[k] is not None else None


def call_upscale(pkg, L, ctx, p, p2, **chg):
    """`p` / `p2` stand in for the pointers that are 1 / 2 in the OK set"""
    a = dict(UPSCALE_OK); a.update(chg); q = _q(a, p, p2)
    tab = (pkg.UpscalePlane * 4)()
    for i in range(4):
        tab[i] = pkg.UpscalePlane(q("d_src"), a["src_stride"], a["in_w"], q("d_dst"), a["dst_stride"], a["out_w"], a["rows"])
    return L.svt_hip_superres_upscale_planes_dev(ctx, a["pix_bytes"], a["bd"], tab if a["planes"] == 1 else None, a["n_planes"])


def call_resize(pkg, L, ctx, p, p2, p3, **chg):
    a = dict(RESIZE_OK); a.update(chg); q = _q(a, p, p2)
    tab = (pkg.ResizePlane * 4)()
    for i in range(4):
        tab[i] = pkg.ResizePlane(q("d_src"), a["src_stride"], a["in_w"], a["in_h"], q("d_dst"), a["dst_stride"], a["out_w"], a["out_h"])
    return L.svt_hip_resize_planes_dev(ctx, a["pix_bytes"], a["bd"], tab if a["planes"] == 1 else None, a["n_planes"], p3 if a["d_scratch"] == 1 else None, a["scratch_bytes"])


def test_null_context_and_bad_arguments_are_refused(pkg):
    L = pkg.lib()
    bufs = [(C.c_uint8 * 4096)() for _ in range(3)]
    p, p2, p3 = (C.cast(b, C.c_void_p).value for b in bufs)
    for c in [{}] + UPSCALE_BAD:
        assert call_upscale(pkg, L, None, p, p2, **c) == BAD_ARG, c
    for c in [{}] + RESIZE_BAD:
        assert call_resize(pkg, L, None, p, p2, p3, **c) == BAD_ARG, c
