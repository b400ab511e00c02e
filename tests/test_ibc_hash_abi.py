"""CPU: the intra-block-copy entry points are declared, exported and bound (prototypes and layouts against the header: tests/test_abi_binding.py), the header
compiles as C99 with them, the two size functions answer without a device, and calls the host can see to be wrong are refused with SVT_HIP_ERR_BAD_ARG before
anything touches HIP (no device exists here: a call that reached the runtime would fail differently or crash).  The same bad arguments with a live context:
tests/test_ibc_hash_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import ibc_hash_common as I
from conftest import ROOT

BAD_ARG = 2   # SVT_HIP_ERR_BAD_ARG
ENTRY_POINTS = ("svt_hip_ibc_hash_scratch_bytes", "svt_hip_ibc_hash_max_entries", "svt_hip_ibc_block_hashes_dev", "svt_hip_ibc_hash_table_dev",
                "svt_hip_ibc_hash_search_batch_dev", "svt_hip_ibc_hash_table_host", "svt_hip_ibc_hash_search_host")


def test_declared_exported_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "svt_hip.h")).read()
    assert re.search(r"SVT_HIP_ERR_BAD_ARG\s*=\s*%d\b" % BAD_ARG, hdr)
    assert re.search(r"#define\s+SVT_HIP_IBC_HASH_BUCKETS\s+\(1 << 19\)", hdr) and pkg.IBC_HASH_BUCKETS == 1 << 19 == I.N_BUCKETS
    assert re.search(r"#define\s+SVT_HIP_IBC_MV_VALS\s+%d\b" % pkg.IBC_MV_VALS, hdr) and pkg.IBC_MV_VALS == I.MV_VALS
    for m in ("ibc_block_hashes", "ibc_hash_table", "ibc_hash_search_batch"):
        assert hasattr(pkg.Context, m)
    assert callable(pkg.ibc_hash_table_host) and callable(pkg.ibc_hash_search_host)
    for f in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % f, hdr) and f in pkg.PROTOTYPES and hasattr(pkg.lib(), f)
    assert [n for n, _ in pkg.IbcHashEntry._fields_] == [n for n, _ in I.ENTRY_DTYPE] and C.sizeof(pkg.IbcHashEntry) == 8
    assert [n for n, _ in pkg.IbcSearchJob._fields_] == list(I.JOB_FIELDS)
    assert [n for n, _ in pkg.IbcSearchResult._fields_] == list(I.RESULT_FIELDS)
    # every entry point cites the reference lines it replaces
    for cite in ("hash_motion.c:138-186", "hash_motion.c:253-283", "av1me.c:1346-1403", "EbAdaptiveMotionVectorPrediction.c:2003-2083", "hash.c:13-62"):
        assert cite in hdr


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "svt_hip.h"\nint main(void){SvtHipIbcHashEntry e = {0}; SvtHipIbcSearchJob j = {0}; SvtHipIbcSearchResult r = {0}; e.hash_value2 = 1; j.mib_size_log2 = 4;\n'
                   "return (int)sizeof(&svt_hip_ibc_block_hashes_dev) + (int)sizeof(&svt_hip_ibc_hash_table_dev) + (int)sizeof(&svt_hip_ibc_hash_search_batch_dev) +"
                   " (int)sizeof(&svt_hip_ibc_hash_table_host) + (int)sizeof(&svt_hip_ibc_hash_search_host) + (int)sizeof(&svt_hip_ibc_hash_scratch_bytes) +"
                   " (int)sizeof(&svt_hip_ibc_hash_max_entries) + (int)e.hash_value2 + j.mib_size_log2 + r.best_cost + SVT_HIP_IBC_HASH_BUCKETS + SVT_HIP_IBC_MV_VALS == 0;}\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_sizes_without_a_device(pkg):
    L = pkg.lib()
    assert L.svt_hip_ibc_hash_max_entries(3, 3) == 0 and L.svt_hip_ibc_hash_max_entries(4, 4) == 1 and L.svt_hip_ibc_hash_max_entries(5, 7) == 2 * 4
    assert L.svt_hip_ibc_hash_max_entries(136, 130) == sum((136 - s + 1) * (130 - s + 1) for s in I.SIZES)
    for w, h in ((0, 4), (4, 0), (-1, 8), (32768, 16), (16, 32768)):   # 32767 x 32767 is below 2^31: the int16 bound implies the 31-bit one
        assert L.svt_hip_ibc_hash_scratch_bytes(w, h) == 0 and L.svt_hip_ibc_hash_max_entries(w, h) == 0, (w, h)
    assert L.svt_hip_ibc_hash_scratch_bytes(1, 1) > 0 and L.svt_hip_ibc_hash_scratch_bytes(32767, 16) > 22 * 32767 * 16
    # two plane sets of 11 bytes a position and the sort's records of 9: the estimate of docs/kernels/ibc_hash.md
    assert 31 * 3840 * 2160 < L.svt_hip_ibc_hash_scratch_bytes(3840, 2160) < 32 * 3840 * 2160


# one thing wrong at a time; shared with the GPU tests, which repeat them with a live context.  1 = "a valid pointer", SCRATCH = "as many bytes as the picture needs"
SCRATCH = -1
HASHES_OK = dict(pix_bytes=1, bd=8, d_luma=1, stride=64, width=64, height=32, block_size=8, d_hash1=1, d_hash2=1, d_same=1, d_scratch=1, scratch_bytes=SCRATCH)
TABLE_OK = dict(pix_bytes=1, bd=8, d_luma=1, stride=64, width=64, height=32, d_bucket_start=1, d_entries=1, capacity=16, d_info=1, d_scratch=1, scratch_bytes=SCRATCH)
SEARCH_OK = dict(pix_bytes=1, bd=8, d_luma=1, stride=64, width=64, height=32, d_bucket_start=1, d_entries=1, d_mv_joint_cost=1, d_mv_comp_cost=1, d_jobs=1, njobs=1, d_results=1)
PICTURE_BAD = [dict(d_luma=None), dict(width=0), dict(height=0), dict(width=-64), dict(width=32768, stride=32768), dict(height=32768),
               dict(stride=63), dict(stride=0), dict(pix_bytes=0), dict(pix_bytes=3), dict(bd=10), dict(bd=12), dict(pix_bytes=2, bd=9), dict(pix_bytes=2, bd=12)]
SCRATCH_BAD = [dict(d_scratch=None), dict(scratch_bytes=0), dict(scratch_bytes=SCRATCH - 1)]
HASHES_BAD = PICTURE_BAD + SCRATCH_BAD + [dict(d_hash1=None), dict(d_hash2=None), dict(d_same=None), dict(block_size=0), dict(block_size=1), dict(block_size=3), dict(block_size=256)]
TABLE_BAD = PICTURE_BAD + SCRATCH_BAD + [dict(d_bucket_start=None), dict(d_entries=None), dict(capacity=-1), dict(d_info=None)]
SEARCH_BAD = PICTURE_BAD + [dict(d_bucket_start=None), dict(d_entries=None), dict(d_mv_joint_cost=None), dict(d_mv_comp_cost=None), dict(d_jobs=None), dict(njobs=-1),
                            dict(d_results=None)]


def _args(L, ok, p, chg):
    a = dict(ok); a.update(chg)
    if a.get("scratch_bytes", 0) < 0:
        a["scratch_bytes"] = max(L.svt_hip_ibc_hash_scratch_bytes(a["width"], a["height"]) + (a["scratch_bytes"] - SCRATCH), 0)
    return a, (lambda k: (p[k] if isinstance(p, dict) else p) if a[k] == 1 else a[k])


def call_hashes(L, ctx, p, **chg):
    """`p` stands in for every pointer that is 1 in HASHES_OK: one address for all of them (calls that are refused), or {parameter: address} (a call that runs
    needs buffers that do not overlap)"""
    a, q = _args(L, HASHES_OK, p, chg)
    return L.svt_hip_ibc_block_hashes_dev(ctx, a["pix_bytes"], a["bd"], q("d_luma"), a["stride"], a["width"], a["height"], a["block_size"], q("d_hash1"), q("d_hash2"), q("d_same"),
                                          q("d_scratch"), a["scratch_bytes"])


def call_table(L, ctx, p, host=False, **chg):
    a, q = _args(L, TABLE_OK, p, chg)
    tail = (q("d_bucket_start"), q("d_entries"), a["capacity"], q("d_info"), q("d_scratch"), a["scratch_bytes"])
    if host: return L.svt_hip_ibc_hash_table_host(a["pix_bytes"], a["bd"], q("d_luma"), a["stride"], a["width"], a["height"], *tail)
    return L.svt_hip_ibc_hash_table_dev(ctx, a["pix_bytes"], a["bd"], q("d_luma"), a["stride"], a["width"], a["height"], *tail)


def call_search(L, ctx, p, host=False, **chg):
    a, q = _args(L, SEARCH_OK, p, chg)
    tail = (q("d_bucket_start"), q("d_entries"), q("d_mv_joint_cost"), q("d_mv_comp_cost"), q("d_jobs"), a["njobs"], q("d_results"))
    if host: return L.svt_hip_ibc_hash_search_host(a["pix_bytes"], a["bd"], q("d_luma"), a["stride"], a["width"], a["height"], *tail)
    return L.svt_hip_ibc_hash_search_batch_dev(ctx, a["pix_bytes"], a["bd"], q("d_luma"), a["stride"], a["width"], a["height"], *tail)


def test_null_context_and_bad_arguments_are_refused(pkg):
    L = pkg.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    for c in [{}] + HASHES_BAD:
        assert call_hashes(L, None, p, **c) == BAD_ARG, c
    for c in [{}] + TABLE_BAD:
        assert call_table(L, None, p, **c) == BAD_ARG, c
    for c in [{}] + SEARCH_BAD:
        assert call_search(L, None, p, **c) == BAD_ARG, c
    # the host forms need no context: the same refusals (the good call is not made here: `p` is no picture)
    for c in TABLE_BAD:
        assert call_table(L, None, p, host=True, **c) == BAD_ARG, c
    for c in SEARCH_BAD:
        assert call_search(L, None, p, host=True, **c) == BAD_ARG, c
