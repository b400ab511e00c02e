"""CPU: the CfL and filter-intra entry points have their Context methods (declarations, exports, prototypes and layouts: tests/test_abi_binding.py), and calls the
host can see to be wrong are refused with SVT_HIP_ERR_BAD_ARG before anything touches HIP (no device exists here: a call that reached the runtime would fail differently or crash).
The same bad arguments with a live context are checked in tests/test_cfl_gpu.py and tests/test_filter_intra_gpu.py."""
import ctypes as C
import os
import re

from conftest import ROOT

BAD_ARG = 2   # SVT_HIP_ERR_BAD_ARG


def _header():
    return open(os.path.join(ROOT, "include", "svt_hip.h")).read()


def test_declared_exported_bound(pkg):
    hdr = _header()
    assert re.search(r"SVT_HIP_ERR_BAD_ARG\s*=\s*%d\b" % BAD_ARG, hdr)
    assert hasattr(pkg.Context, "cfl_predict_batch") and hasattr(pkg.Context, "filter_intra_predict_batch")
    # the batch entry point's comment no longer lists what now has an entry point
    assert "CfL, filter-intra, palette and intra block copy are not covered" not in hdr and "palette and intra block copy are\n * not covered" in hdr


# one thing wrong at a time; shared with the GPU tests, which repeat them with a live context
CFL_OK = dict(pix_bytes=1, bd=8, d_luma=1, luma_stride=128, d_edges=1, d_jobs=1, njobs=1, d_cb=1, d_cr=1, chroma_stride=64, d_ac=1)
CFL_BAD = [dict(pix_bytes=3), dict(pix_bytes=0), dict(bd=12), dict(bd=10), dict(pix_bytes=2, bd=9), dict(njobs=-1), dict(luma_stride=0), dict(luma_stride=-128),
           dict(chroma_stride=0), dict(chroma_stride=-64), dict(d_luma=None), dict(d_edges=None), dict(d_jobs=None), dict(d_cb=None, d_cr=None)]
FI_OK = dict(pix_bytes=1, bd=8, d_edges=1, d_jobs=1, njobs=1, d_dst=1, dst_stride=64)
FI_BAD = [dict(pix_bytes=3), dict(pix_bytes=0), dict(bd=12), dict(bd=10), dict(pix_bytes=2, bd=9), dict(njobs=-1), dict(dst_stride=0), dict(dst_stride=-64),
          dict(d_edges=None), dict(d_jobs=None), dict(d_dst=None)]


def call_cfl(L, ctx, p, **chg):
    """`p` stands in for every pointer that is 1 in CFL_OK"""
    a = dict(CFL_OK); a.update(chg)
    q = lambda k: p if a[k] == 1 else a[k]
    return L.svt_hip_cfl_predict_batch_dev(ctx, a["pix_bytes"], a["bd"], q("d_luma"), a["luma_stride"], q("d_edges"), q("d_jobs"), a["njobs"], q("d_cb"), q("d_cr"),
                                           a["chroma_stride"], q("d_ac"))


def call_fi(L, ctx, p, **chg):
    a = dict(FI_OK); a.update(chg)
    q = lambda k: p if a[k] == 1 else a[k]
    return L.svt_hip_filter_intra_predict_batch_dev(ctx, a["pix_bytes"], a["bd"], q("d_edges"), q("d_jobs"), a["njobs"], q("d_dst"), a["dst_stride"])


def test_null_context_and_bad_arguments_are_refused(pkg):
    L = pkg.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    for c in [{}] + CFL_BAD:
        assert call_cfl(L, None, p, **c) == BAD_ARG, c
    for c in [{}] + FI_BAD:
        assert call_fi(L, None, p, **c) == BAD_ARG, c
