"""CPU: the two intra entry points have their Context methods (declarations, exports, prototypes and layouts: tests/test_abi_binding.py), and calls the host
can see to be wrong are refused with SVT_HIP_ERR_BAD_ARG before anything touches HIP (no device exists here: a call that reached the runtime would fail differently or crash).
The same bad arguments with a live context are checked in tests/test_intra_ois_gpu.py and tests/test_intra_predict_gpu.py."""
import ctypes as C
import os
import re

from conftest import ROOT

BAD_ARG = 2   # SVT_HIP_ERR_BAD_ARG


def _header():
    return open(os.path.join(ROOT, "include", "svt_hip.h")).read()


def test_declared_exported_bound(pkg):
    assert re.search(r"SVT_HIP_ERR_BAD_ARG\s*=\s*%d\b" % BAD_ARG, _header())
    assert hasattr(pkg.Context, "intra_ois_picture") and hasattr(pkg.Context, "intra_predict_batch")


def test_null_context_and_bad_arguments_are_refused(pkg):
    L = pkg.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    ois, batch = L.svt_hip_intra_ois_picture_dev, L.svt_hip_intra_predict_batch_dev
    # (d_src, stride, w, h, mode_end, d_mode, d_cost): a valid set first, then one thing wrong at a time
    ok = dict(d_src=p, stride=352, w=352, h=288, mode_end=12, d_mode=p, d_cost=p)
    cases = [{}, dict(w=356), dict(h=292), dict(w=8, stride=16), dict(h=8), dict(mode_end=13), dict(mode_end=-1), dict(stride=351), dict(w=200, stride=200),
             dict(d_src=None), dict(d_mode=None), dict(d_cost=None), dict(w=0), dict(h=-16)]
    for c in cases:
        a = dict(ok); a.update(c)
        assert ois(None, a["d_src"], a["stride"], a["w"], a["h"], a["mode_end"], a["d_mode"], a["d_cost"]) == BAD_ARG, c
    # (pix_bytes, bd, d_edges, d_jobs, njobs, d_dst, dst_stride)
    ok = dict(pix_bytes=1, bd=8, d_edges=p, d_jobs=p, njobs=1, d_dst=p, dst_stride=64)
    cases = [{}, dict(pix_bytes=3), dict(pix_bytes=0), dict(bd=12), dict(bd=10), dict(pix_bytes=2, bd=9), dict(njobs=-1), dict(dst_stride=0), dict(dst_stride=-64),
             dict(d_edges=None), dict(d_jobs=None), dict(d_dst=None)]
    for c in cases:
        a = dict(ok); a.update(c)
        assert batch(None, a["pix_bytes"], a["bd"], a["d_edges"], a["d_jobs"], a["njobs"], a["d_dst"], a["dst_stride"]) == BAD_ARG, c
