"""CPU: the two intra entry points are declared, exported and bound, the job structure matches the header, and calls the host can see to be wrong are
refused with SVT_HIP_ERR_BAD_ARG before anything touches HIP (no device exists here: a call that reached the runtime would fail differently or crash).
The same bad arguments with a live context are checked in tests/test_intra_ois_gpu.py and tests/test_intra_predict_gpu.py."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NAMES = ("svt_hip_intra_predict_batch_dev", "svt_hip_intra_ois_picture_dev")
BAD_ARG = 2   # SVT_HIP_ERR_BAD_ARG


def _header():
    return open(os.path.join(ROOT, "include", "svt_hip.h")).read()


def test_declared_exported_bound(pkg):
    L = pkg.lib()
    hdr = _header()
    assert re.search(r"SVT_HIP_ERR_BAD_ARG\s*=\s*%d\b" % BAD_ARG, hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(SvtHipCtx \*ctx" % n, hdr, flags=re.M), f"{n} not declared in include/svt_hip.h"
        assert re.search(r"\sT\s+%s$" % n, out, flags=re.M), f"{n} not exported"
        assert getattr(L, n).argtypes, f"{n}: no argtypes"
    assert "} SvtHipIntraJob;" in hdr
    assert hasattr(pkg, "IntraJob") and hasattr(pkg.Context, "intra_ois_picture") and hasattr(pkg.Context, "intra_predict_batch")


def test_job_structure_matches_the_header(pkg, tmp_path):
    """sizeof / offsets of the ctypes mirror against a C99 compiler's view of include/svt_hip.h."""
    fields = [f[0] for f in pkg.IntraJob._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svt_hip.h"\nint main(void){printf("%d", (int)sizeof(SvtHipIntraJob));' +
                   "".join(f'printf(" %d", (int)offsetof(SvtHipIntraJob, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(pkg.IntraJob)
    assert got[1:] == [getattr(pkg.IntraJob, f).offset for f in fields]


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
