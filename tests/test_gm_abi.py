"""CPU: the global-motion entry points have their Context methods (declarations, exports, prototypes and layouts: tests/test_abi_binding.py), the error table the
library generates is the formula's, and calls the host can see to be wrong are refused with SVT_HIP_ERR_BAD_ARG before anything touches HIP (no device exists
here: a call that reached the runtime would fail differently or crash).  The same bad arguments with a live context are checked in tests/test_gm_gpu.py."""
import ctypes as C
import os
import re

import numpy as np

import gm_common as g
from conftest import ROOT

BAD_ARG = 2   # SVT_HIP_ERR_BAD_ARG


def _header():
    return open(os.path.join(ROOT, "include", "svt_hip.h")).read()


def test_declared_exported_bound(pkg):
    hdr = _header()
    assert re.search(r"SVT_HIP_ERR_BAD_ARG\s*=\s*%d\b" % BAD_ARG, hdr)
    for m in ("gm_shear_params_batch", "gm_warp_error_batch", "gm_frame_error_batch", "gm_refine_picture"):
        assert hasattr(pkg.Context, m)
    assert int(re.search(r"#define SVT_HIP_GM_MAX_REFS (\d+)", hdr).group(1)) == pkg.GM_MAX_REFS == 8


def test_error_table_is_the_formula(pkg):
    """the table is generated, not copied: min(16384, floor(16384 (|i - 255| / 255)^0.7 + 0.5)); tests/test_gm_ref_cpu.py pins the formula to the reference's table"""
    L = pkg.lib()
    out = np.zeros(512, np.uint16)
    assert L.svt_hip_gm_error_table(out.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(out.astype(np.int64), g.error_table())
    assert (out[0], out[254], out[255], out[256], out[510], out[511]) == (16384, 339, 0, 339, 16384, 16384)
    assert L.svt_hip_gm_error_table(None) == BAD_ARG


def test_scratch_size_grows_with_the_jobs(pkg):
    L = pkg.lib()
    s = [L.svt_hip_gm_refine_scratch_bytes(n) for n in (-1, 0, 1, 7, 1024)]
    assert s[0] == s[1] > 0 and s[1] < s[2] <= s[3] < s[4] < (1 << 20)


# one thing wrong at a time; shared with the GPU test, which repeats them with a live context
SHEAR_OK = dict(d_wmmat=1, n=1, d_out=1)
SHEAR_BAD = [dict(n=-1), dict(n=(1 << 20) + 1), dict(d_wmmat=None), dict(d_out=None)]
WARP_OK = dict(d_src=1, src_stride=96, w=96, h=80, d_ref=1, ref_width=96, ref_height=80, ref_stride=96, d_models=1, n=1, d_err=1)
WARP_BAD = [dict(d_src=None), dict(d_ref=None), dict(d_models=None), dict(d_err=None), dict(n=-1), dict(n=(1 << 20) + 1), dict(w=7), dict(h=7), dict(w=0), dict(h=-8),
            dict(w=16385, src_stride=16385), dict(src_stride=95), dict(src_stride=-96), dict(ref_stride=95), dict(ref_width=7), dict(ref_height=0),
            dict(ref_height=16385)]
FRAME_OK = dict(d_src=1, src_stride=96, w=96, h=80, refs=1, n_refs=1, d_err=1, ref_stride=96, ref_plane=1)
FRAME_BAD = [dict(d_src=None), dict(refs=None), dict(d_err=None), dict(n_refs=-1), dict(n_refs=9), dict(w=7), dict(h=7), dict(src_stride=95), dict(ref_stride=95),
             dict(ref_plane=None)]
REFINE_OK = dict(d_src=1, src_stride=96, w=96, h=80, refs=1, n_refs=1, d_jobs=1, njobs=1, d_results=1, d_scratch=1, ref_stride=96, ref_plane=1, ref_width=96,
                 ref_height=80)
REFINE_BAD = [dict(d_src=None), dict(refs=None), dict(d_jobs=None), dict(d_results=None), dict(d_scratch=None), dict(n_refs=0), dict(n_refs=9), dict(njobs=-1),
              dict(njobs=1025), dict(w=7), dict(h=7), dict(w=16385, src_stride=16385), dict(src_stride=95), dict(ref_stride=95), dict(ref_plane=None),
              dict(ref_width=7), dict(ref_height=7)]


def _q(a, p):
    return lambda k: p if a[k] == 1 else a[k]


def call_shear(L, ctx, p, **chg):
    """`p` stands in for every pointer that is 1 in the OK set"""
    a = dict(SHEAR_OK); a.update(chg); q = _q(a, p)
    return L.svt_hip_gm_shear_params_batch_dev(ctx, q("d_wmmat"), a["n"], q("d_out"))


def call_warp(L, ctx, p, **chg):
    a = dict(WARP_OK); a.update(chg); q = _q(a, p)
    return L.svt_hip_gm_warp_error_batch_dev(ctx, q("d_src"), a["src_stride"], a["w"], a["h"], q("d_ref"), a["ref_width"], a["ref_height"], a["ref_stride"], q("d_models"),
                                             a["n"], q("d_err"))


def _tab(pkg, a, p, n):
    tab = (pkg.GmRef * pkg.GM_MAX_REFS)()
    for i in range(pkg.GM_MAX_REFS):
        tab[i] = pkg.GmRef(p if a["ref_plane"] == 1 else None, a.get("ref_width", a["w"]), a.get("ref_height", a["h"]), a["ref_stride"], 0)
    return tab if a["refs"] == 1 else None


def call_frame(pkg, L, ctx, p, **chg):
    a = dict(FRAME_OK); a.update(chg); q = _q(a, p)
    return L.svt_hip_gm_frame_error_batch_dev(ctx, q("d_src"), a["src_stride"], a["w"], a["h"], _tab(pkg, a, p, a["n_refs"]), a["n_refs"], q("d_err"))


def call_refine(pkg, L, ctx, p, **chg):
    a = dict(REFINE_OK); a.update(chg); q = _q(a, p)
    return L.svt_hip_gm_refine_picture_dev(ctx, q("d_src"), a["src_stride"], a["w"], a["h"], _tab(pkg, a, p, a["n_refs"]), a["n_refs"], q("d_jobs"), a["njobs"],
                                           q("d_results"), q("d_scratch"), None)


def test_null_context_and_bad_arguments_are_refused(pkg):
    L = pkg.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    for c in [{}] + SHEAR_BAD:
        assert call_shear(L, None, p, **c) == BAD_ARG, c
    for c in [{}] + WARP_BAD:
        assert call_warp(L, None, p, **c) == BAD_ARG, c
    for c in [{}] + FRAME_BAD:
        assert call_frame(pkg, L, None, p, **c) == BAD_ARG, c
    for c in [{}] + REFINE_BAD:
        assert call_refine(pkg, L, None, p, **c) == BAD_ARG, c
