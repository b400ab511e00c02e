"""CPU: the TPL synthesizer / r0-beta entry points have their Context methods and size_t sizes (declarations, exports, prototypes and layouts: tests/test_abi_binding.py),
calls the host can see to be wrong are refused with SVT_HIP_ERR_BAD_ARG before anything touches HIP (no device exists here), and the size helpers give what
the layout needs.  The same refusals with a live context, and their texts, are checked in tests/test_tpl_synth_gpu.py."""
import ctypes as C
import os
import re

from conftest import ROOT

BAD_ARG = 2   # SVT_HIP_ERR_BAD_ARG
ENTRY_POINTS = ("svt_hip_tpl_dep_bytes", "svt_hip_tpl_r0beta_out_bytes", "svt_hip_tpl_r0beta_scratch_bytes", "svt_hip_tpl_synth_picture_dev",
                "svt_hip_tpl_r0beta_dev", "svt_hip_tpl_window_dev", "svt_hip_tpl_window_host")


def test_declared_exported_bound(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "svt_hip.h")).read()
    for n in ENTRY_POINTS[:3]:
        assert getattr(L, n).restype is C.c_size_t
    for m in ("tpl_window", "tpl_synth_picture", "tpl_r0beta"):
        assert hasattr(pkg.Context, m)
    assert hasattr(pkg, "tpl_window_host") and hasattr(pkg, "tpl_ref_window")
    assert pkg.TPL_MAX_WINDOW == int(re.search(r"#define SVT_HIP_TPL_MAX_WINDOW (\d+)", hdr).group(1)) == 60


def test_ref_window_binding(pkg):
    """First matching index per slot, entry 0 from POC 0, -1 where the POC is not in the window."""
    assert pkg.tpl_ref_window([0, 16, 8, 4], [8, 0, None, 5]) == [0, 2, 0, -1, -1, -1, -1, -1]
    assert pkg.tpl_ref_window([32, 48, 40], [32]) == [-1, 0, -1, -1, -1, -1, -1, -1]
    assert pkg.tpl_ref_window([16, 0, 8, 0], [0, 8, 16, 0, 8, 16, 3]) == [1, 1, 2, 0, 1, 2, 0, -1]   # a POC that occurs twice: the first index
    assert pkg.tpl_cell_log2(1280, 720) == 4 and pkg.tpl_cell_log2(720, 728) == 4 and pkg.tpl_cell_log2(1920, 712) == 3 and pkg.tpl_cell_log2(352, 288) == 3


def bad_argument_cases(pkg, p):
    """(ok, wrong) over a valid three-picture 200 x 136 window: one thing wrong at a time.  `p` is any non-NULL, 8-byte aligned pointer value.  A wrong entry is
    (what to change, the entry points it applies to, a word its text carries)."""
    def params(**kw):
        P = pkg.tpl_synth_params(200, 136, 1000, r0_in=0.5, cell_log2=3)
        for k, v in kw.items(): setattr(P, k, v)
        return P

    def frames(n=3, **kw):
        F = pkg.tpl_window_frames([(p + 4096 * i, p + 65536 * (i + 1), 1, [-1, i - 1, -1, -1, -1, -1, -1, -1] if i else [-1] * 8) for i in range(n)])
        for k, v in kw.items():
            idx, field = k.split("__")
            if field.startswith("rw"): F[int(idx[1:])].ref_window[int(field[2:])] = v
            else: setattr(F[int(idx[1:])], field, v)
        return F

    ok = dict(params=params(), frames=frames(), n_frames=3, frame_idx=1, d_stats=p, d_dep=p + 65536, d_out=p + 8, d_scratch=p + 16)
    every = ("synth", "r0beta", "window", "host")
    wrong = [(dict(params=params(rate=1)), every, "rate must be 0"), (dict(params=params(rate=-1)), every, "rate must be 0"),
             (dict(params=None), every, "bad argument"), (dict(params=params(w=204)), every, "bad argument"), (dict(params=params(h=140)), every, "bad argument"),
             (dict(params=params(w=8)), every, "bad argument"), (dict(params=params(h=0)), every, "bad argument"), (dict(params=params(w=-16)), every, "bad argument"),
             (dict(params=params(cell_log2=2)), every, "bad argument"), (dict(params=params(cell_log2=5)), every, "bad argument"),
             (dict(params=params(sb_size=32)), every, "bad argument"), (dict(params=params(sb_size=96)), every, "bad argument"),
             (dict(params=params(base_rdmult=-1)), every, "bad argument")]
    win = ("synth", "window", "host")
    wrong += [(dict(frames=None), win, "bad argument"), (dict(n_frames=0), win, "bad argument"), (dict(n_frames=-1), win, "bad argument"),
              (dict(frames=frames(61), n_frames=61), win, "bad argument"),
              (dict(frames=frames(f1__d_dep=None)), win, "bad argument"), (dict(frames=frames(f1__d_stats=None)), win, "bad argument"),
              (dict(frames=frames(f0__d_stats=None, f0__on=0)), win, "bad argument"), (dict(frames=frames(f2__d_dep=p + 65536)), win, "bad argument"),
              (dict(frames=frames(f1__rw0=3)), win, "bad argument"), (dict(frames=frames(f1__rw3=-2)), win, "bad argument"),
              (dict(frames=frames(f2__rw7=64)), win, "bad argument")]
    wrong += [(dict(frames=frames(**{f"f{i}__rw{k}": i})), win, "names the picture itself") for i, k in ((1, 1), (2, 4), (0, 7), (1, 2))]
    wrong += [(dict(frame_idx=3), ("synth",), "frame_idx"), (dict(frame_idx=-1), ("synth",), "frame_idx")]
    wrong += [(dict(d_out=None), ("r0beta", "window", "host"), "bad argument"), (dict(d_out=p + 4), ("r0beta", "window", "host"), "bad argument"),
              (dict(d_scratch=None), ("r0beta", "window"), "bad argument"), (dict(d_scratch=p + 2), ("r0beta", "window"), "bad argument"),
              (dict(d_stats=None), ("r0beta",), "bad argument"), (dict(d_dep=None), ("r0beta",), "bad argument")]
    return ok, wrong


def call(L, ctx, which, a):
    P = C.byref(a["params"]) if a["params"] is not None else None
    if which == "synth": return L.svt_hip_tpl_synth_picture_dev(ctx, P, a["frames"], a["n_frames"], a["frame_idx"])
    if which == "r0beta": return L.svt_hip_tpl_r0beta_dev(ctx, P, a["d_stats"], a["d_dep"], a["d_out"], a["d_scratch"])
    if which == "window": return L.svt_hip_tpl_window_dev(ctx, P, a["frames"], a["n_frames"], a["d_out"], a["d_scratch"])
    return L.svt_hip_tpl_window_host(P, a["frames"], a["n_frames"], a["d_out"])


def test_null_context_and_bad_arguments_are_refused(pkg):
    L = pkg.lib()
    buf = (C.c_uint64 * 8)()
    ok, wrong = bad_argument_cases(pkg, C.addressof(buf))
    for which in ("synth", "r0beta", "window"):
        assert call(L, None, which, ok) == BAD_ARG   # NULL context: refused before the (dangling) pointers could be used
    for change, where, _ in wrong:
        a = dict(ok); a.update(change)
        for which in where:
            assert call(L, None, which, a) == BAD_ARG, (which, change)
    # a self-reference through entry 0 is the POC-0 rule, not an error: the host form accepts it (and needs real memory, so it runs in test_tpl_synth_host.py)


def test_sizes(pkg):
    L = pkg.lib()
    dep, out = L.svt_hip_tpl_dep_bytes, L.svt_hip_tpl_r0beta_out_bytes
    assert dep(200, 136, 4) == 13 * 9 * 16 and dep(200, 136, 3) == 26 * 18 * 16
    assert dep(3840, 2160, 4) == 240 * 135 * 16 and dep(720, 728, 4) == 45 * 46 * 16 and dep(16, 16, 3) == 4 * 16
    for bad in ((200, 136, 2), (200, 136, 5), (204, 136, 3), (200, 132, 3), (8, 136, 3), (0, 0, 4), (-8, 16, 4)):
        assert dep(*bad) == 0, bad
    assert out(200, 136, 64) == 24 + 8 * (13 * 9 + 4 * 3) and out(200, 136, 128) == 24 + 8 * (13 * 9 + 2 * 2)
    assert out(3840, 2160, 64) == 24 + 8 * (240 * 135 + 60 * 34) and out(720, 728, 128) == 24 + 8 * (45 * 46 + 6 * 6)
    assert out(200, 136, 32) == 0 and out(204, 136, 64) == 0
    assert C.sizeof(pkg.TplR0BetaHeader) == 24
    assert 16 <= L.svt_hip_tpl_r0beta_scratch_bytes() <= 4096
