"""CPU: the OBMC target / motion-refinement entry points are declared, exported and bound (prototypes and layouts against the header: tests/test_abi_binding.py),
the header compiles as C99 with them, calls the host can see to be wrong are refused with SVT_HIP_ERR_BAD_ARG before anything touches HIP, one thing wrong at a
time, and the library's host forms (svt_hip_obmc_neighbours_host, svt_hip_obmc_target_host, svt_hip_obmc_search_host) equal the numpy restatement on the lists the
GPU test launches.  The same bad arguments with a live context: tests/test_obmc_search_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import obmc_common as S
from conftest import ROOT

BAD_ARG = 2
ENTRY_POINTS = ("svt_hip_obmc_neighbours_host", "svt_hip_obmc_target_batch_dev", "svt_hip_obmc_search_batch_dev", "svt_hip_obmc_target_host", "svt_hip_obmc_search_host")


def test_declared_exported_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "svt_hip.h")).read()
    assert hasattr(pkg.Context, "obmc_batch") and callable(pkg.obmc_target_host) and callable(pkg.obmc_search_host) and callable(pkg.obmc_neighbours_host)
    for f in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % f, hdr) and f in pkg.PROTOTYPES and hasattr(pkg.lib(), f)
    assert [n for n, _ in pkg.ObmcTargetJob._fields_] == list(S.TARGET_FIELDS) and C.sizeof(pkg.ObmcTargetJob) == 4 * (10 + 4 * 4)
    assert [n for n, _ in pkg.ObmcSearchJob._fields_] == list(S.JOB_FIELDS) and C.sizeof(pkg.ObmcSearchJob) == 4 * len(S.JOB_FIELDS)
    assert [n for n, _ in pkg.ObmcSearchResult._fields_] == list(S.RESULT_FIELDS) and C.sizeof(pkg.ObmcSearchResult) == 4 * len(S.RESULT_FIELDS)
    # the header and the shared arithmetic cite the reference lines they replace, and say what is not covered
    cites = (":2376-2437", ":2196-2224", ":2226-2256", ":2233-2260", ":918-958", ":960-996", "EbModeDecision.c:2951-3036", "av1me.c:836-855", ":791-834", ":776-790",
             ":1069-1254", ":973-1035", "variance.c:212-269", ":270-299", ":2495-2522", "EbModeDecision.c:2958")
    for cite in cites:
        assert cite in hdr, cite
    for word in ("force_integer_mv", "use_scaled_rec_refs_if_needed", "choose_best_av1_mv_pred", "chroma", "hook"):
        assert word in hdr[hdr.index("SvtHipObmcBlk;"):hdr.index("SvtHipObmcTargetJob;")], word
    src = open(os.path.join(ROOT, "svt-av1_amd", "csrc", "obmc_search.h")).read()
    for cite in (":2376-2437", ":918-996", ":2951-3036", ":836-855", ":1069-1254", ":212-269", ":85-99", "ibcs::mvsad_err_cost", "ibc::mv_err_cost"):
        assert cite in src, cite
    assert "inline uint32_t mvsad_err_cost" not in src and " mv_err_cost(" not in src.replace("ibc::mv_err_cost(", "")   # reused, not restated


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "svt_hip.h"\nint main(void){SvtHipObmcTargetJob t = {0}; SvtHipObmcSearchJob j = {0}; SvtHipObmcSearchResult r = {0}; t.above_rel[3] = 1;\n'
                   "j.allow_hp = 1; r.besterr = 4000000000u;\n"
                   "return (int)sizeof(&svt_hip_obmc_target_batch_dev) + (int)sizeof(&svt_hip_obmc_search_batch_dev) + (int)sizeof(&svt_hip_obmc_target_host) +"
                   " (int)sizeof(&svt_hip_obmc_search_host) + (int)sizeof(&svt_hip_obmc_neighbours_host) + t.above_rel[3] + j.allow_hp + (int)r.besterr == 0;}\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_library_exports_the_declared_symbols(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    assert set(ENTRY_POINTS) <= exported
    assert not [s for s in exported if "obmc" in s and s not in ENTRY_POINTS + ("svt_hip_obmc_cost_batch_dev",)]   # no launcher, no helper


# ------------------------------------------------------------------------------------------------------------------ refusals
# one thing wrong at a time; shared with the GPU test.  1 = "a valid pointer"; `job` = changes to the one good job
SEG = lambda *v: list(v) + [0] * (4 - len(v))
TARGET_JOB = dict(bsize=6, x=16, y=16, n_above=1, above_rel=SEG(0), above_len=SEG(4), n_left=1, left_rel=SEG(0), left_len=SEG(4), above_off=0, above_stride=16, left_off=256,
                  left_stride=8, wm_off=0)
TARGET_OK = dict(d_src=1, src_stride=96, width=96, height=64, d_nbr=1, nbr_samples=4096, jobs=1, njobs=1, d_wsrc=1, d_mask=1, wm_samples=1024, job={})
TARGET_BAD = [dict(d_src=None), dict(jobs=None), dict(d_wsrc=None), dict(d_mask=None), dict(d_nbr=None), dict(njobs=-1), dict(njobs=(1 << 24) + 1), dict(width=0), dict(height=0),
              dict(src_stride=95), dict(nbr_samples=-1), dict(wm_samples=-1),
              dict(job=dict(bsize=-1)), dict(job=dict(bsize=22)), dict(job=dict(bsize=0)), dict(job=dict(bsize=2)), dict(job=dict(bsize=16)), dict(job=dict(bsize=17)),   # not the 17
              dict(job=dict(x=-1)), dict(job=dict(y=-1)), dict(job=dict(x=81)), dict(job=dict(y=49)),
              dict(job=dict(n_above=-1)), dict(job=dict(n_above=5)), dict(job=dict(n_left=-1)), dict(job=dict(n_left=5)),
              dict(job=dict(above_len=SEG(0))), dict(job=dict(above_len=SEG(5))), dict(job=dict(above_rel=SEG(1))), dict(job=dict(above_rel=SEG(-1))),
              dict(job=dict(n_above=2, above_rel=SEG(0, 1), above_len=SEG(2, 2))),   # overlapping
              dict(job=dict(n_above=2, above_rel=SEG(2, 0), above_len=SEG(2, 2))),   # descending
              dict(job=dict(n_left=2, left_rel=SEG(0, 2), left_len=SEG(2, 3))),      # past the block
              dict(job=dict(above_off=-1)), dict(job=dict(above_off=4096 - 7 * 16 - 16 + 1)), dict(job=dict(above_stride=-1)), dict(job=dict(above_stride=600)),
              dict(job=dict(left_off=-1)), dict(job=dict(left_off=4096 - 15 * 8 - 8 + 1)), dict(job=dict(left_stride=-1)), dict(job=dict(left_stride=300)),
              dict(job=dict(wm_off=-1)), dict(job=dict(wm_off=1024 - 255))]
TARGET_GOOD = [{}, dict(njobs=0), dict(d_nbr=None, nbr_samples=0, job=dict(n_above=0, n_left=0)), dict(job=dict(x=80, y=48)), dict(job=dict(wm_off=1024 - 256)),
               dict(job=dict(above_off=4096 - 7 * 16 - 16)), dict(job=dict(left_off=4096 - 15 * 8 - 8)), dict(job=dict(above_stride=0, left_stride=0)),
               dict(job=dict(n_above=2, above_rel=SEG(0, 2), above_len=SEG(2, 2), n_left=2, left_rel=SEG(1, 3), left_len=SEG(1, 1)))]
SEARCH_JOB = dict(bsize=6, mi_row=4, mi_col=4, wm_off=0, mv_row=0, mv_col=0, ref_mv_row=0, ref_mv_col=0, sad_per_bit=10, error_per_bit=10, allow_hp=1)
SEARCH_OK = dict(d_ref=1, ref_stride=256, width=96, height=64, pad_w=80, pad_h=80, mi_rows=16, mi_cols=24, d_wsrc=1, d_mask=1, wm_samples=4096, d_mv_joint_cost=1,
                 d_mv_comp_cost=1, jobs=1, njobs=1, d_results=1, job={})
SEARCH_BAD = [dict(d_ref=None), dict(d_wsrc=None), dict(d_mask=None), dict(d_mv_joint_cost=None), dict(d_mv_comp_cost=None), dict(jobs=None), dict(d_results=None),
              dict(njobs=-1), dict(njobs=(1 << 24) + 1), dict(width=0), dict(height=0), dict(ref_stride=255), dict(pad_w=-1), dict(pad_h=-1), dict(mi_rows=0), dict(mi_cols=0),
              dict(wm_samples=-1),
              dict(job=dict(bsize=-1)), dict(job=dict(bsize=22)), dict(job=dict(bsize=0)), dict(job=dict(bsize=17)),
              dict(job=dict(mi_row=-1)), dict(job=dict(mi_col=-1)), dict(job=dict(mi_row=16)), dict(job=dict(mi_col=24)),
              dict(job=dict(wm_off=-1)), dict(job=dict(wm_off=4096 - 255)),
              # a vector outside the reference's int16: beyond it a difference could leave the MV cost tables
              dict(job=dict(mv_row=32768)), dict(job=dict(mv_col=-32769)), dict(job=dict(ref_mv_row=40000)), dict(job=dict(ref_mv_col=-40000)),
              dict(job=dict(sad_per_bit=-1)), dict(job=dict(error_per_bit=-1)), dict(job=dict(allow_hp=2)), dict(job=dict(allow_hp=-1)),
              # the border: a 16-wide block needs 16 + 8 samples on the left / top and 16 + 9 on the right / bottom, whatever the walk does
              dict(pad_w=24), dict(pad_h=24), dict(pad_w=0, pad_h=0), dict(pad_w=72, pad_h=80, job=dict(bsize=12, mi_row=0, mi_col=0)),
              dict(pad_w=80, pad_h=72, job=dict(bsize=12, mi_row=0, mi_col=0)),
              dict(width=95, pad_w=25, pad_h=25), dict(height=63, pad_w=25, pad_h=25)]   # the picture ends before 4 * mi_cols / 4 * mi_rows: the right / bottom border starts sooner
SEARCH_GOOD = [{}, dict(njobs=0), dict(pad_w=25, pad_h=25), dict(pad_w=73, pad_h=73, job=dict(bsize=12, mi_row=0, mi_col=0)), dict(job=dict(wm_off=4096 - 256)),
               dict(pad_w=0, pad_h=0, ref_stride=96, job=dict(ref_mv_row=32767, ref_mv_col=32767)),   # empty limits: status 1, nothing is read
               dict(job=dict(mv_row=-32768, mv_col=32767, ref_mv_row=-300, ref_mv_col=300)), dict(job=dict(sad_per_bit=0, error_per_bit=0, allow_hp=0))]


def call(pkg, kind, ctx, p, host=False, **chg):
    """`p` stands in for every pointer that is 1 in TARGET_OK / SEARCH_OK"""
    a = dict(TARGET_OK if kind == "target" else SEARCH_OK); a.update(chg)
    q = lambda k: p if a[k] == 1 else a[k]
    L = pkg.lib()
    if kind == "target":
        jobs = S.c_target_jobs(pkg, [dict(TARGET_JOB, **a["job"])])
        args = (q("d_src"), a["src_stride"], a["width"], a["height"], q("d_nbr"), a["nbr_samples"], None if a["jobs"] is None else C.cast(jobs, C.c_void_p), a["njobs"],
                q("d_wsrc"), q("d_mask"), a["wm_samples"])
        return L.svt_hip_obmc_target_host(*args) if host else L.svt_hip_obmc_target_batch_dev(ctx, *args)
    jobs = S.c_search_jobs(pkg, [dict(SEARCH_JOB, **a["job"])])
    args = (q("d_ref"), a["ref_stride"], a["width"], a["height"], a["pad_w"], a["pad_h"], a["mi_rows"], a["mi_cols"], q("d_wsrc"), q("d_mask"), a["wm_samples"],
            q("d_mv_joint_cost"), q("d_mv_comp_cost"), None if a["jobs"] is None else C.cast(jobs, C.c_void_p), a["njobs"], q("d_results"))
    return L.svt_hip_obmc_search_host(*args) if host else L.svt_hip_obmc_search_batch_dev(ctx, *args)


@pytest.mark.parametrize("kind", ["target", "search"])
def test_null_context_and_bad_arguments_are_refused(pkg, kind):
    buf = np.zeros(1 << 20, np.uint8)   # zeros: a flat picture, flat neighbours and free vectors for the calls that are accepted; `p` has room on every side
    p = C.c_void_p(buf.ctypes.data + (1 << 19))
    bad, good = (TARGET_BAD, TARGET_GOOD) if kind == "target" else (SEARCH_BAD, SEARCH_GOOD)
    for c in bad + good:
        assert call(pkg, kind, None, p, **c) == BAD_ARG, c   # no context
    for c in bad:
        assert call(pkg, kind, None, p, host=True, **c) == BAD_ARG, c
    for c in good:
        assert call(pkg, kind, None, p, host=True, **c) == 0, c


def test_neighbour_helper_refusals(pkg):
    L = pkg.lib()
    job = pkg.ObmcTargetJob()
    sb, flag = np.full(32, 6, np.uint8), np.ones(32, np.uint8)
    q = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = [q(sb), q(flag), q(sb), q(flag), 16, 24, 4, 4, 6, C.byref(job)]
    assert L.svt_hip_obmc_neighbours_host(*ok) == 0 and (job.n_above, job.n_left) == (1, 1)
    for i, v in ((9, None), (8, 0), (8, 22), (8, 17), (4, 0), (5, 0), (6, -1), (7, -1), (6, 16), (7, 24), (6, 5), (7, 3), (0, None), (3, None)):
        args = list(ok); args[i] = v
        assert L.svt_hip_obmc_neighbours_host(*args) == BAD_ARG, (i, v)
    bad_sb = sb.copy(); bad_sb[1] = 22
    assert L.svt_hip_obmc_neighbours_host(q(bad_sb), q(flag), None, None, 16, 24, 4, 4, 6, C.byref(job)) == BAD_ARG
    assert L.svt_hip_obmc_neighbours_host(None, None, None, None, 16, 24, 4, 4, 6, C.byref(job)) == 0 and (job.n_above, job.n_left) == (0, 0)


def test_refusal_texts_are_literals_that_name_the_entry_point():
    src = open(os.path.join(ROOT, "svt-av1_amd", "csrc", "svt_hip_api.cpp")).read()
    for name in ("svt_hip_obmc_target_batch_dev", "svt_hip_obmc_search_batch_dev"):
        body = src[src.index("int %s(" % name):]
        body = body[:body.index("\n}\n")]
        texts = re.findall(r'bad_arg\(c(?:, ("[^"]*"))?\)', body)
        assert len(texts) >= 1 and all(t.startswith('"%s: ' % name) for t in texts), (name, texts)


# ------------------------------------------------------------------------------------------------------------------ the host forms
SB_OF_SIDE = {1: 0, 2: 3, 4: 6, 8: 9, 16: 12, 32: 15}   # a square BlockSize of that many 4-sample units


@pytest.mark.parametrize("which", ["small", "big"])
def test_neighbour_helper_equals_the_restatement(pkg, which):
    case, _, _ = S.cached("target", which)
    for spec, job, (sa, sl, a, l) in zip(case["specs"], case["jobs"], case["segs"]):
        side = lambda lay: None if lay is None else ([SB_OF_SIDE[s] for s in lay[0]], lay[1])
        got = pkg.obmc_neighbours_host(side(a), side(l), spec["mi_rows"], spec["mi_cols"], job["y"] // 4, job["x"] // 4, job["bsize"])
        for name in ("n_above", "n_left"):
            assert getattr(got, name) == job[name], (spec, name)
        for name in ("above_rel", "above_len", "left_rel", "left_len"):
            assert list(getattr(got, name)) == job[name], (spec, name)


@pytest.mark.parametrize("which", ["small", "big"])
def test_target_host_form_equals_the_restatement(pkg, which):
    case, (wsrc, mask), _ = S.cached("target", which)
    got_w, got_m = pkg.obmc_target_host(case["plane"], case["nbr"], S.c_target_jobs(pkg, case["jobs"]), case["wm_samples"])
    assert (got_w == wsrc).all() and (got_m == mask).all()


@pytest.mark.parametrize("which", ["small", "big"])
def test_search_host_form_equals_the_restatement(pkg, which):
    case, want, _ = S.cached("search", which)
    n = len(case["jobs"])
    res = pkg.obmc_search_host(S.picture_view(case), case["pad_w"], case["pad_h"], case["mi_rows"], case["mi_cols"], case["wsrc"], case["mask"], case["jc"], case["cc"],
                               S.c_search_jobs(pkg, case["jobs"]))
    for k, (r, w) in enumerate(zip(S.results_as_dicts(res, n), want)):
        assert r == w, (k, case["specs"][k])
    # ... and stage 1's host form makes the arrays stage 2 read
    t = case["target"]
    got_w, got_m = pkg.obmc_target_host(t["plane"], t["nbr"], S.c_target_jobs(pkg, t["jobs"]), t["wm_samples"])
    assert (got_w == case["wsrc"]).all() and (got_m == case["mask"]).all()
