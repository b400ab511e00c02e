"""CPU: the intra-block-copy full-search entry points are declared, exported and bound (prototypes and layouts against the header: tests/test_abi_binding.py), the
header compiles as C99 with them, the size function answers without a device, and calls the host can see to be wrong are refused with SVT_HIP_ERR_BAD_ARG before
anything touches HIP.  The same bad arguments with a live context: tests/test_ibc_search_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import ibc_hash_common as H
import ibc_search_common as S
from conftest import ROOT
from test_ibc_hash_abi import BAD_ARG, PICTURE_BAD

ENTRY_POINTS = ("svt_hip_ibc_full_search_scratch_bytes", "svt_hip_ibc_full_search_batch_dev", "svt_hip_ibc_full_search_host")


def test_declared_exported_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "svt_hip.h")).read()
    assert hasattr(pkg.Context, "ibc_full_search_batch") and callable(pkg.ibc_full_search_host)
    for f in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % f, hdr) and f in pkg.PROTOTYPES and hasattr(pkg.lib(), f)
    assert [n for n, _ in pkg.IbcFullSearchJob._fields_] == list(S.JOB_FIELDS) and C.sizeof(pkg.IbcFullSearchJob) == 4 * len(S.JOB_FIELDS)
    assert [n for n, _ in pkg.IbcFullSearchResult._fields_] == list(S.RESULT_FIELDS)
    assert C.sizeof(pkg.IbcFullSearchResult) == 4 * (len(S.RESULT_FIELDS) - 1) + C.sizeof(pkg.IbcSearchResult)
    # the header cites the reference lines the entry point replaces
    for cite in (":346-435", ":437-573", "av1me.c:578-643", ":650-710", ":712-775", ":1306-1411", "EbModeDecision.c:4523"):
        assert cite in hdr, cite
    src = open(os.path.join(ROOT, "svt-av1_amd", "csrc", "ibc_search.h")).read()
    for cite in ("av1me.c:346-435", "av1me.c:437-573", "av1me.c:578-643", "av1me.c:650-710", "av1me.c:712-775", "av1me.c:1306-1411", "second_best_mv", "mv_check_bounds"):
        assert cite in src, cite


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "svt_hip.h"\nint main(void){SvtHipIbcFullSearchJob j = {0}; SvtHipIbcFullSearchResult r = {0}; j.use_hash = 1; r.hash.best_cost = 2;\n'
                   "return (int)sizeof(&svt_hip_ibc_full_search_batch_dev) + (int)sizeof(&svt_hip_ibc_full_search_host) + (int)sizeof(&svt_hip_ibc_full_search_scratch_bytes) +"
                   " j.use_hash + r.hash.best_cost + r.dv_valid == 0;}\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_scratch_size_without_a_device(pkg):
    L = pkg.lib()
    assert L.svt_hip_ibc_full_search_scratch_bytes(-1) == 0 and L.svt_hip_ibc_full_search_scratch_bytes(-(1 << 31)) == 0
    sizes = [L.svt_hip_ibc_full_search_scratch_bytes(n) for n in (0, 1, 2, 1000)]
    assert sizes[0] == 0 and 0 < sizes[1] <= sizes[2] < sizes[3] and all(s % 256 == 0 for s in sizes)
    assert 1000 * 64 * 8 < sizes[3] < 1000 * 1024   # 64 partial minima of 8 bytes a job, and a little more


# one thing wrong at a time; shared with the GPU test.  1 = "a valid pointer", SCRATCH = "as many bytes as njobs needs"
SCRATCH = -1
GOOD, FIRST_INVALID = [64, 4, 16, 1, 0, 0, 0, 0], [300, 1, 0, 0, 7, -3, 0, 0]
FULL_OK = dict(pix_bytes=1, bd=8, d_luma=1, stride=64, width=64, height=32, d_bucket_start=1, d_entries=1, d_mv_joint_cost=1, d_mv_comp_cost=1, patterns=GOOD, d_jobs=1,
               njobs=1, d_results=1, d_scratch=1, scratch_bytes=SCRATCH)
# a pattern the walk can reach with interval < 1 or range outside 1 .. 256; a half-NULL table
PATTERNS_BAD = [dict(patterns=None), dict(patterns=[64, 4, 16, 0, 0, 0, 0, 0]), dict(patterns=[64, 4, 0, 1, 0, 0, 0, 0]), dict(patterns=[64, 4, 257, 1, 0, 0, 0, 0]),
                dict(patterns=[64, 4, 16, -1, 0, 0, 0, 0]), dict(patterns=[64, 8, 28, 4, 15, 0, 7, 1]), dict(patterns=[64, 8, 28, 4, 15, 2, 0, 1]),
                dict(patterns=[64, 8, 28, 4, 15, 2, 7, 0]), dict(patterns=[64, 1, 16, 0, 0, 0, 0, 0]), dict(patterns=[7, 7, -1, 1, 0, 0, 0, 0])]
# ... and lists that are accepted: an invalid first pattern, patterns behind one of interval 1, a first pattern whose walk can never become progressive
PATTERNS_GOOD = [GOOD, FIRST_INVALID, [256, 1, 0, 0, 0, 0, 0, 0], [200, 1, -5, -5, 0, 0, 0, 0], [64, 8, 28, 4, 15, 1, 0, 0], [6, 1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0]]
FULL_BAD = PICTURE_BAD + PATTERNS_BAD + [dict(d_bucket_start=None), dict(d_entries=None), dict(d_mv_joint_cost=None), dict(d_mv_comp_cost=None), dict(d_jobs=None),
                                         dict(njobs=-1), dict(njobs=(1 << 24) + 1), dict(d_results=None)]
SCRATCH_BAD = [dict(d_scratch=None), dict(scratch_bytes=0), dict(scratch_bytes=SCRATCH - 1)]


def call_full(L, ctx, p, host=False, **chg):
    """`p` stands in for every pointer that is 1 in FULL_OK: one address for all of them (calls that are refused), or {parameter: address}"""
    a = dict(FULL_OK); a.update(chg)
    if a["scratch_bytes"] < 0:
        a["scratch_bytes"] = max(L.svt_hip_ibc_full_search_scratch_bytes(a["njobs"]) + (a["scratch_bytes"] - SCRATCH), 0)
    q = lambda k: (p[k] if isinstance(p, dict) else p) if a[k] == 1 else a[k]
    pat = None if a["patterns"] is None else np.array(a["patterns"], np.int32)
    head = (a["pix_bytes"], a["bd"], q("d_luma"), a["stride"], a["width"], a["height"], q("d_bucket_start"), q("d_entries"), q("d_mv_joint_cost"), q("d_mv_comp_cost"),
            None if pat is None else pat.ctypes.data_as(C.c_void_p), q("d_jobs"), a["njobs"], q("d_results"))
    if host: return L.svt_hip_ibc_full_search_host(*head)
    return L.svt_hip_ibc_full_search_batch_dev(ctx, *head, q("d_scratch"), a["scratch_bytes"])


def test_null_context_and_bad_arguments_are_refused(pkg):
    L = pkg.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    for c in [{}] + FULL_BAD + SCRATCH_BAD + [dict(patterns=g) for g in PATTERNS_GOOD]:
        assert call_full(L, None, p, **c) == BAD_ARG, c
    # the host form needs no context: the same refusals.  njobs = 0 makes the accepted calls harmless: `p` is no picture
    for c in FULL_BAD:
        assert call_full(L, None, p, host=True, njobs=0, **c) == BAD_ARG if "njobs" not in c else call_full(L, None, p, host=True, **c) == BAD_ARG, c
    for g in PATTERNS_GOOD:
        assert call_full(L, None, p, host=True, njobs=0, patterns=g) == 0, g
    assert call_full(L, None, p, host=True, njobs=0, d_bucket_start=None, d_entries=None) == 0


def test_refusal_texts_are_literals_that_name_the_entry_point():
    src = open(os.path.join(ROOT, "svt-av1_amd", "csrc", "svt_hip_api.cpp")).read()
    body = src[src.index("int svt_hip_ibc_full_search_batch_dev("):]
    body = body[:body.index("\n}\n")]
    texts = re.findall(r'bad_arg\(c(?:, ("[^"]*"))?\)', body)
    assert len(texts) >= 4 and all(t.startswith('"svt_hip_ibc_full_search_batch_dev: ') for t in texts), texts
