"""CPU: the two TPL dispenser entry points have their Context methods (declarations, exports, prototypes and layouts: tests/test_abi_binding.py), calls the
host can see to be wrong are refused with SVT_HIP_ERR_BAD_ARG before anything touches HIP (no device exists here), and the scratch size is
what one decision byte per macroblock needs.  The same bad arguments with a live context are checked in tests/test_tpl_gpu.py."""
import ctypes as C

BAD_ARG = 2   # SVT_HIP_ERR_BAD_ARG


def test_declared_exported_bound(pkg):
    L = pkg.lib()
    assert L.svt_hip_tpl_dispenser_scratch_bytes.restype is C.c_size_t
    assert hasattr(pkg.Context, "tpl_dispenser_picture") and hasattr(pkg.Context, "tpl_recon_to_host") and hasattr(pkg, "tpl_stats_grid")


def test_stats_record_matches_the_numpy_view(pkg):
    import numpy as np
    import tpl_common as T
    assert T.STATS_DTYPE.itemsize == C.sizeof(pkg.TplMbStats) == np.dtype(pkg.TplMbStats).itemsize
    for name, _ in pkg.TplMbStats._fields_:
        assert T.STATS_DTYPE.fields[name][1] == getattr(pkg.TplMbStats, name).offset


def bad_argument_cases(pkg, p):
    """(description, kwargs) pairs over a valid 352x288 call: one thing wrong at a time.  `p` is any non-NULL pointer value."""
    def params(**kw):
        P = pkg.TplParams()
        P.w, P.h, P.pad = 352, 288, 32
        P.q.variant, P.q.log_scale = 2, 0
        P.use_ois = 1
        for k, v in kw.items():
            if k in ("variant", "log_scale"): setattr(P.q, k, v)
            else: setattr(P, k, v)
        return P

    def refs(**kw):
        R = (pkg.TplRef * 7)()
        R[0].d_src, R[0].d_rec, R[0].src_stride, R[0].rec_stride = p, p, 416, 416
        for k, v in kw.items(): setattr(R[0], k, v)
        return R

    ok = dict(params=params(), d_cur=p, cur_stride=352, refs=refs(), d_mv=p, d_ref_mask=p, d_ois_mode=p, d_ois_cost=p, d_recon=p + 64, recon_stride=416, d_stats=p,
              d_scratch=p)
    wrong = [dict(params=params(w=356)), dict(params=params(h=292)), dict(params=params(w=8)), dict(params=params(h=8)), dict(params=params(w=0)),
             dict(params=params(h=-16)), dict(params=params(pad=15)), dict(params=params(pad=0)), dict(params=params(variant=0)), dict(params=params(variant=3)),
             dict(params=params(log_scale=1)), dict(params=None), dict(d_cur=None), dict(cur_stride=351), dict(cur_stride=336), dict(recon_stride=351),
             dict(refs=None), dict(refs=refs(src_stride=351)), dict(refs=refs(rec_stride=351)), dict(refs=refs(d_rec=None)), dict(refs=refs(d_rec=p + 64)),
             dict(d_mv=None), dict(d_ref_mask=None), dict(d_ois_mode=None), dict(d_ois_cost=None), dict(d_recon=None), dict(d_stats=None), dict(d_scratch=None),
             dict(params=params(w=200), cur_stride=200)]
    return ok, wrong


def call(L, ctx, a):
    return L.svt_hip_tpl_dispenser_picture_dev(ctx, C.byref(a["params"]) if a["params"] is not None else None, a["d_cur"], a["cur_stride"], a["refs"], a["d_mv"],
                                               a["d_ref_mask"], a["d_ois_mode"], a["d_ois_cost"], a["d_recon"], a["recon_stride"], a["d_stats"], a["d_scratch"])


def test_null_context_and_bad_arguments_are_refused(pkg):
    L = pkg.lib()
    buf = (C.c_uint8 * 4096)()
    ok, wrong = bad_argument_cases(pkg, C.addressof(buf))
    assert call(L, None, ok) == BAD_ARG   # NULL context
    for c in wrong:
        a = dict(ok); a.update(c)
        assert call(L, None, a) == BAD_ARG, c


def test_scratch_bytes(pkg):
    f = pkg.lib().svt_hip_tpl_dispenser_scratch_bytes
    sizes = [16, 64, 200, 352, 1280, 1920, 3840, 7680]
    for w in sizes:
        for h in sizes:
            n_mb = ((w + 15) // 16) * ((h + 15) // 16)
            assert 0 < f(w, h) <= 64 * n_mb + 4096 and f(w, h) >= n_mb   # no stored coefficient block (1 KB) per macroblock; one decision byte
    for a, b in zip(sizes, sizes[1:]):
        assert f(a, 288) <= f(b, 288) and f(352, a) <= f(352, b)
    assert f(3840, 2160) < 64 * 1024
