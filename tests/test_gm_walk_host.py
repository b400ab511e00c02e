"""CPU: the refinement's state machine (svt-av1_amd/csrc/gm_walk.h, the text the device compiles) built for the host and driven with the reference's own
svt_av1_warp_error as the probe: every shared walk must end where svt_av1_refine_integerized_param ends, count the probes the restatement counts, and hand every
candidate the shear parameters svt_get_shear_params gives the struct the reference would hold at that point (stale rows 4-5 of a ROTZOOM model included).
Also svt_get_shear_params itself against the host build on random and boundary matrices."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gm_common as g
from conftest import ROOT


@pytest.fixture(scope="module")
def host(pkg, tmp_path_factory):
    so = tmp_path_factory.mktemp("gm_walk") / "libgm_walk_host.so"
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "gm_walk_host.cpp"), "-o", str(so)])
    H = C.CDLL(str(so))
    H.gm_walk_host.argtypes = [C.POINTER(pkg.GmJob), PROBE, C.c_void_p, C.POINTER(pkg.GmResult), C.POINTER(C.c_int)]
    H.gm_shear_params_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    H.gm_shear_params_host.restype = None
    return H


PROBE = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int)


def test_k_is_what_the_tests_assume(host):
    assert host.gm_walk_host_k() == g.K


@pytest.mark.parametrize("name", g.WALK_NAMES)
def test_state_machine_against_the_reference(pkg, ref, host, name):
    wk = g.walk_by_name(name)
    src, rf = g.walk_planes(wk)
    (want_mat, want_type, want_err), rest = g.walk_reference(ref, name)
    wrong = []

    def probe(_user, model_p, pre, wmtype):
        m = C.cast(model_p, C.POINTER(pkg.GmModel)).contents
        mat = list(m.mat)
        if wmtype == g.ROTZOOM:
            mat[4], mat[5] = pre[0], pre[1]
        wm = g.make_wm(mat + [0, 0], wmtype)
        a, b, c, d, ok = g.ref_shear(ref, mat)
        if ok != m.valid or (mat[2] > 0 and (a, b, c, d) != (m.alpha, m.beta, m.gamma, m.delta)):
            wrong.append((mat, (a, b, c, d, ok), (m.alpha, m.beta, m.gamma, m.delta, m.valid)))
        e = g.ref_warp_error(ref, wm, rf, src)
        if ok and list(wm.wmmat)[:6] != list(m.mat):
            wrong.append(("warped with", list(wm.wmmat)[:6], list(m.mat)))
        return e

    job = pkg.GmJob(ref=0, wmtype=wk["wmtype"], n_refinements=wk["n"], best_frame_error=wk["bfe"])
    for k, v in enumerate(wk["start"]):
        job.wmmat[k] = v
    out, n_eval = pkg.GmResult(), C.c_int()
    assert host.gm_walk_host(C.byref(job), PROBE(probe), None, C.byref(out), C.byref(n_eval)) == 0
    assert not wrong, wrong[:3]
    assert (list(out.wmmat), out.wmtype, out.best_error) == (want_mat, want_type, want_err)
    assert (out.probes, out.invalid_probes) == (rest["probes"], rest["invalid"])
    assert n_eval.value >= out.probes and out.rounds >= 1


def test_shear_params_host_build(pkg, ref, host):
    mats = g.shear_matrices(2000, seed=3)
    out = (pkg.GmModel * len(mats))()
    host.gm_shear_params_host(mats.ctypes.data_as(C.c_void_p), len(mats), out)
    for m, o in zip(mats, out):
        a, b, c, d, ok = g.ref_shear(ref, m)
        assert o.valid == ok and list(o.mat) == list(m), m
        if m[2] > 0:
            assert (o.alpha, o.beta, o.gamma, o.delta) == (a, b, c, d), m
        else:
            assert (o.alpha, o.beta, o.gamma, o.delta) == (0, 0, 0, 0)
