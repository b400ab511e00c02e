"""Shared by the tests of svt_hip_gm_estimate_picture_dev: the picture pairs and the reference's result for each (compute_global_motion composed of the reference's
functions in its order, gm_fit_common.ref_estimate), computed once per process."""
import functools

import numpy as np

import gm_common as g
import gm_fit_common as fc
import gm_front_common as f

ONE = g.ONE
SHEAR = (0, 0, ONE + 3000, 6000, -500, ONE - 2500)
SQUEEZE = (0, 0, ONE + 4000, 0, 0, ONE - 4000)


@functools.lru_cache(maxsize=None)
def pair(name):
    """name -> (source, reference)"""
    if name == "rot_96x80": return f.rot_pair(32, 96, 80)
    if name == "rot_352x288": return f.rot_pair(33, 352, 288)
    if name == "identical_96x80": return f.tex(21, 96, 80), f.tex(21, 96, 80)
    if name == "noise_96x80": return f.noise(27, 96, 80), f.noise(28, 96, 80)
    if name == "noise_352x288": return f.noise(24, 352, 288), f.noise(26, 352, 288)
    if name == "flat_96x80": return f.flat(96, 80), f.flat(96, 80)
    if name == "shifted_96x80": return f.tex(21, 96, 80), f.tex(21, 96, 80, dx=-3, dy=2)
    if name == "shear_96x80": return tuple(f._frozen(a) for a in g.picture_pair(40, 96, 80, SHEAR))
    if name == "shear_352x288": return tuple(f._frozen(a) for a in g.picture_pair(40, 352, 288, SHEAR))
    if name == "squeeze_352x288": return tuple(f._frozen(a) for a in g.picture_pair(42, 352, 288, SQUEEZE))
    raise KeyError(name)


SMALL = ["rot_96x80", "identical_96x80", "noise_96x80", "flat_96x80", "shifted_96x80", "shear_96x80"]
LARGE = ["rot_352x288", "noise_352x288", "shear_352x288", "squeeze_352x288"]
_want = {}


def reference(L, name, rotzoom_model_only=0, allow_hp=0):
    key = (name, rotzoom_model_only, allow_hp)
    if key not in _want:
        s, r = pair(name)
        _want[key] = fc.ref_estimate(L, s, r, rotzoom_model_only, allow_hp)
    return _want[key]


def strided(plane, pad, fill):
    """a copy of the plane inside a wider buffer: another row stride, the same samples"""
    buf = np.full((plane.shape[0] + 2, plane.shape[1] + pad), fill, np.uint8)
    buf[1:-1, 3:3 + plane.shape[1]] = plane
    return buf[1:-1, 3:3 + plane.shape[1]]


def same_estimate(e, want):
    """an SvtHipGmEstimate against ref_estimate's result: the final model and every per-model record the decision consumed"""
    bad = []
    if (list(e.wmmat), e.wmtype) != (want["wmmat"], want["wmtype"]): bad.append(("final", list(e.wmmat), e.wmtype, want["wmmat"], want["wmtype"]))
    if e.ref_frame_error != want["ref_frame_error"]: bad.append(("frame error", e.ref_frame_error, want["ref_frame_error"]))
    if e.n_models != len(want["records"]): bad.append(("n_models", e.n_models))
    for m, rec in enumerate(want["records"]):
        got = e.models[m]
        refined = rec["wmtype"] >= 0
        if (got.num_inliers_kept, got.fit_wmtype, got.wmtype) != (rec["num_inliers_kept"], rec["fit_wmtype"], rec["wmtype"]): bad.append(("record", m, got.num_inliers_kept, got.fit_wmtype, got.wmtype, rec))
        if refined and (list(got.wmmat), got.best_error) != (rec["wmmat"], rec["best_error"]): bad.append(("refined", m, list(got.wmmat), got.best_error, rec))
    return bad
