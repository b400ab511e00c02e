"""GPU: what the C-ABI layer (csrc/svt_hip_api.cpp) answers to calls it refuses, with a live context: the return code and the exact text svt_hip_last_error()
gives afterwards.  Some refusals carry a text and some leave the context's text as it was; the per-call table (csrc/rtcd_hip.cpp) tells a device failure from a
domain delegation by exactly that, so both are pinned.  The families here are the ones the other live-context tests do not refuse anything in: transforms,
deblocking, the CDEF frame calls, the md_* pictures, pyramids / SAD loops, the temporal filter's three entry points, the 2-D copies and the self-guided unit search, the per-call list and single-unit
forms (percall.hip), plus the zero-size successes that return before anything is enqueued.

No kernel is meant to run.  Every case is built so that a lost check shows as a failed assertion and not as a launch on bad memory: every pointer lies in one
allocation of the context, every count (nblk, n, njobs, n_sb) is 0 and the one wrong thing is a scalar.  The expected values are the ones the entry points had
before their validate / launch / report code was folded into shared helpers."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

OK, BAD_ARG = 0, 2   # SVT_HIP_OK, SVT_HIP_ERR_BAD_ARG (include/svt_hip.h)
SAME = None          # the refusal sets no text: svt_hip_last_error() is what it was before the call
SENTINEL = b"svt_hip_intra_predict_batch_dev: bad argument"
SCRATCH_TEXT = b"scratch smaller than svt_hip_sgr_search_units_scratch_bytes()"
BUF_BYTES = 2 << 20


class Env:
    """One device allocation every pointer argument points into, and the host-side structures the entry points read."""

    def __init__(self, hip, pkg):
        self.hip, self.pkg, self.L, self.h = hip, pkg, hip.L, hip.h
        self.base = hip.empty(BUF_BYTES)
        self.d = self.at(0)
        self.host = (C.c_uint8 * 65536)()
        self.hp = C.cast(self.host, C.c_void_p)

    def at(self, off):
        assert 0 <= off < BUF_BYTES and off % 256 == 0
        return C.c_void_p(self.base.value + off)

    def p3(self, n=3):
        return (C.c_void_p * 3)(*[self.at(65536 * (i + 1)).value if i < n else None for i in range(3)])

    def qp(self, **kw):
        q = self.pkg.QuantParams()
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def scans(self):
        st = self.pkg.ScanTables()
        st.iscan[0] = self.d.value
        return st

    def fwd_job(self, tx_size=0, **qp):
        d = self.d.value
        return self.pkg.FwdTxJob(tx_size=tx_size, nblk=0, d_src=d, src_stride=64, d_pred=d, pred_stride=64, d_descs=d, qp=self.qp(**qp), scans=self.scans(), d_coeff=None,
                                 d_qcoeff=d, d_dqcoeff=d, d_eob=d, d_cul_level=d, d_energy=None)

    def last(self):
        return self.L.svt_hip_last_error(self.h)

    def set_sentinel(self):
        assert self.L.svt_hip_intra_predict_batch_dev(self.h, 3, 8, self.d, self.d, 0, self.d, 64) == BAD_ARG and self.last() == SENTINEL


@pytest.fixture(scope="module")
def env(hip, pkg):
    e = Env(hip, pkg)
    yield e
    hip.check(hip.L.svt_hip_sync(hip.h), "sync")
    hip.free(e.base)


I3 = C.c_int * 3


def i3(a, b=None, c=None):
    return I3(a, a if b is None else b, a if c is None else c)


# ---- transforms
def fwd_batch(e, tx_size=0, pix_bytes=1, **qp):
    q, st, d = e.qp(**qp), e.scans(), e.d
    return e.L.svt_hip_fwd_txfm_quant_batch_dev(e.h, tx_size, pix_bytes, d, 64, d, 64, d, 0, C.byref(q), C.byref(st), None, d, d, d, d, None)


def fwd_multi(e, pix_bytes=1, njobs=1, **job):
    jobs = (e.pkg.FwdTxJob * 1)(e.fwd_job(**job))
    return e.L.svt_hip_fwd_txfm_quant_multi_dev(e.h, pix_bytes, C.cast(jobs, C.c_void_p), njobs)


def enc_multi(e, pix_bytes=1, bd=8, njobs=1, **job):
    jobs = (e.pkg.EncTxJob * 1)(e.pkg.EncTxJob(fwd=e.fwd_job(**job), d_recon=e.d.value, recon_stride=64))
    return e.L.svt_hip_enc_txfm_multi_dev(e.h, pix_bytes, bd, jobs, njobs)


def inv_multi(e, pix_bytes=1, bd=8, njobs=1, tx_size=0):
    d = e.d.value
    jobs = (e.pkg.InvTxJob * 1)(e.pkg.InvTxJob(tx_size=tx_size, nblk=0, d_dqcoeff=d, d_pred=d, pred_stride=64, d_recon=d, recon_stride=64, d_descs=d))
    return e.L.svt_hip_inv_txfm_add_multi_dev(e.h, pix_bytes, bd, C.cast(jobs, C.c_void_p), njobs)


def quantize(e, n_coeffs=16, **qp):
    q, d = e.qp(**qp), e.d
    return e.L.svt_hip_quantize_batch_dev(e.h, d, n_coeffs, 0, C.byref(q), d, d, d, d)


# ---- deblocking
def deblock_frame(e, bd=8, sharpness=0, units_w0=0):
    return e.L.svt_hip_deblock_frame_dev(e.h, e.p3(), 1, i3(64), bd, e.p3(), e.p3(), i3(units_w0, 0, 0), i3(0), sharpness)


def deblock_fused(e, bd=8, plane_w0=4):
    src, dst = e.p3(1), (C.c_void_p * 3)(e.at(65536 * 8).value, None, None)
    return e.L.svt_hip_deblock_frame_fused_dev(e.h, src, dst, 1, i3(64), bd, i3(plane_w0, 4, 4), i3(4), e.p3(), e.p3(), i3(1), i3(1), 0)


def build_edges(e, ss_x=1, filt_units_w0=0):
    return e.L.svt_hip_dlf_build_edges_picture_dev(e.h, e.d, 1, 1, ss_x, 1, i3(4), i3(4), i3(filt_units_w0, 0, 0), i3(0), None, e.p3(), e.p3())


def dlf_plane(e, plane_w=8):
    d = e.d.value
    return e.pkg.DlfSearchPlane(q=e.pkg.DlfSearch(), d_recon=d, d_tmp=(C.c_void_p * 2)(e.at(65536).value, e.at(131072).value), stride=64, plane_w=plane_w, plane_h=8, d_src=d,
                                src_stride=64, d_edges_v=d, d_edges_h=d, units_w=(plane_w + 3) // 4, units_h=2)


def dlf_levels_picture(e, pix_bytes=1, plane_w=8):
    planes = (e.pkg.DlfSearchPlane * 1)(dlf_plane(e, plane_w))
    best = (C.c_int * 3)()
    return e.L.svt_hip_dlf_search_levels_picture_dev(e.h, 1, C.cast(planes, C.c_void_p), pix_bytes, 8, e.d, C.cast(best, C.c_void_p), None)


def dlf_level(e, bd=8):
    q, best, d = e.pkg.DlfSearch(), C.c_int(0), e.d
    return e.L.svt_hip_dlf_search_level_dev(e.h, C.byref(q), d, e.at(65536), 1, 64, bd, 8, 8, d, 64, d, d, 2, 2, e.at(131072), C.byref(best), None)


# ---- CDEF frame calls
def cdef_search(e, pix_bytes=1, w=64, bd=8):
    d = e.d
    return e.L.svt_hip_cdef_search_frame_dev(e.h, pix_bytes, e.p3(), i3(64), e.p3(), i3(64), w, 64, d, 3, bd, d, d, d)


def cdef_apply(e, bd=8, h=64):
    d = e.d
    return e.L.svt_hip_cdef_apply_frame_dev(e.h, 1, e.p3(), e.p3(), i3(64), 64, h, d, d, d, 3, bd, d, d)


# ---- the md_* pictures: the lists are host arrays
def md_lists(e, pu_w=8, pu_x=0, ref_stride=64):
    pus = (e.pkg.MdPu * 1)(e.pkg.MdPu(x=pu_x, y=0, w=pu_w, h=8))
    refs = (e.pkg.MdRefPlane * 1)(e.pkg.MdRefPlane(d_plane=e.d.value, stride=ref_stride, x_min=0, y_min=0, x_max=63, y_max=63))
    return pus, refs


def md_sad(e, fn="svt_hip_md_fullpel_sad_picture_dev", n_pus=1, n_refs=1, **lists):
    pus, refs = md_lists(e, **lists)
    return getattr(e.L, fn)(e.h, e.d, 64, 64, 64, 1, 0, n_pus, C.cast(pus, C.c_void_p), n_refs, C.cast(refs, C.c_void_p), e.d, e.d)


def md_avg(e, fn="svt_hip_md_fullpel_avg_sad_picture_dev", n_pairs=1, pair0=0, **lists):
    pus, refs = md_lists(e, **lists)
    pairs = (C.c_uint8 * 2)(pair0, 0)
    return getattr(e.L, fn)(e.h, e.d, 64, 64, 64, 1, 0, 1, C.cast(pus, C.c_void_p), 1, C.cast(refs, C.c_void_p), e.d, n_pairs, C.cast(pairs, C.c_void_p), e.d)


def md_grid(e, fn="svt_hip_md_subpel_grid_picture_dev", bank=0, n_refs=1, **lists):
    pus, refs = md_lists(e, **lists)
    return getattr(e.L, fn)(e.h, e.d, 64, 64, 64, 1, 0, 1, C.cast(pus, C.c_void_p), n_refs, C.cast(refs, C.c_void_p), e.d, bank, e.d)


# ---- the self-guided unit search on a real 64 x 64 plane with unit_size 64
SGR_DGD, SGR_SCRATCH = 65536, 262144   # the plane leaves room for the three samples the filter reads beyond each border


def sgr_need(e):
    return e.L.svt_hip_sgr_search_units_scratch_bytes(64, 64, 64)


def sgr_plane(e, short=0, pix_bytes=1, bd=8, unit_size=64, ep_mask=0xFFFF, ss_y=0):
    d = e.d
    return e.L.svt_hip_sgr_search_units_plane_dev(e.h, pix_bytes, bd, e.at(SGR_DGD), 128, d, 64, 64, 64, unit_size, ss_y, ep_mask, d, d, d, d, e.at(SGR_SCRATCH), sgr_need(e) - short)


def sgr_picture(e, short=0, n_planes=1, bd=8, unit_size=64, ep_mask=0xFFFF):
    d = e.d.value
    pl = (e.pkg.SgrUnitsPlaneDev * 1)(e.pkg.SgrUnitsPlaneDev(d_dgd=e.at(SGR_DGD).value, stride=128, d_src=d, src_stride=64, pw=64, ph=64, unit_size=unit_size, ss_y=0, ep_mask=ep_mask,
                                                            d_xqd=d, d_err=d, d_best_ep=d, d_best_xqd=d, d_scratch=e.at(SGR_SCRATCH).value, scratch_bytes=sgr_need(e) - short))
    return e.L.svt_hip_sgr_search_units_picture_dev(e.h, 1, bd, n_planes, pl)


def wiener_walk(e, wiener_win=7, unit_size=64):
    d = e.d
    return e.L.svt_hip_wiener_walk_units_dev(e.h, 1, 8, e.at(SGR_DGD), 128, 64, 64, unit_size, 0, None, 0, d, 64, d, d, wiener_win, d, None)


def wiener_walk_picture(e, n_planes=1, ss_y=0):
    d = e.d.value
    pl = (e.pkg.WienerWalkPlane * 1)(e.pkg.WienerWalkPlane(d_dgd=e.at(SGR_DGD).value, stride=128, pw=64, ph=64, unit_size=64, ss_y=ss_y, d_dbl=None, dbl_stride=0, d_src=d, src_stride=64,
                                                          d_unit_wiener=d, d_active=d, wiener_win=7, d_err=d, d_probes=None))
    return e.L.svt_hip_wiener_walk_units_picture_dev(e.h, 1, 8, n_planes, pl)


def copy2d(e, fn, wbytes=64, rows=4, dpitch=64, hpitch=64):
    if "h2d" in fn:
        return getattr(e.L, fn)(e.h, e.d, dpitch, e.hp, hpitch, wbytes, rows)
    return getattr(e.L, fn)(e.h, e.hp, hpitch, e.d, dpitch, wbytes, rows)


# ---- the temporal filter: a one-frame window (the central picture alone), no jobs
def tf_filter(e, pix_bytes=1, bd=8, ss=(1, 1), decay=4, n_refs=1, src0=True, pred0=True):
    refs = (e.pkg.TfRef * 1)()
    if not pred0:            # a frame with block records and no predictor plane
        refs[0].blocks = e.d.value
    nl = (C.c_double * 3)(1.0, 1.0, 1.0)
    src = e.p3() if src0 else (C.c_void_p * 3)(None, e.at(65536).value, e.at(131072).value)
    return e.L.svt_hip_tf_filter_frame_dev(e.h, pix_bytes, bd, src, i3(64, 32, 32), e.p3(), i3(64, 32, 32), 64, 64, ss[0], ss[1], 1, refs, n_refs, nl, decay, 64, e.at(65536 * 8))


def tf_noise(e, pix_bytes=1, bd=8, width=64, stride=64):
    return e.L.svt_hip_tf_estimate_noise_dev(e.h, e.d, pix_bytes, bd, width, 8, stride, e.at(65536))


def tf_subpel(e, pix_bytes=1, bd=8, ref0=True):
    ref = e.p3() if ref0 else (C.c_void_p * 3)(None, e.at(65536).value, e.at(131072).value)
    return e.L.svt_hip_tf_subpel_frame_dev(e.h, pix_bytes, bd, e.p3(), i3(64, 32, 32), ref, i3(64, 32, 32), e.p3(), i3(64, 32, 32), 16, 16, 0, 1, 1, e.d, 0, e.at(65536 * 8))


TF_FILTER_TEXT, TF_SUBPEL_TEXT = b"svt_hip_tf_filter_frame_dev: bad argument", b"svt_hip_tf_subpel_frame_dev: bad argument"

COPIES_2D = ("svt_hip_memcpy2d_h2d", "svt_hip_memcpy2d_d2h", "svt_hip_memcpy2d_h2d_async", "svt_hip_memcpy2d_d2h_async")

# (id, call, return code, text afterwards)
CASES = [
    # transforms
    ("fwd_batch-tx_size", lambda e: fwd_batch(e, tx_size=19), BAD_ARG, b"svt_hip_fwd_txfm_quant_batch_dev: bad argument"),
    ("fwd_batch-pix_bytes", lambda e: fwd_batch(e, pix_bytes=3), BAD_ARG, b"svt_hip_fwd_txfm_quant_batch_dev: bad argument"),
    ("fwd_batch-qp.variant", lambda e: fwd_batch(e, variant=4), BAD_ARG, b"svt_hip_fwd_txfm_quant_batch_dev: bad argument"),
    ("fwd_batch-qp.log_scale", lambda e: fwd_batch(e, log_scale=3), BAD_ARG, b"svt_hip_fwd_txfm_quant_batch_dev: bad argument"),
    ("fwd_batch-qp.coeff_shape", lambda e: fwd_batch(e, coeff_shape=4), BAD_ARG, b"svt_hip_fwd_txfm_quant_batch_dev: bad argument"),
    ("inv_batch-bd", lambda e: e.L.svt_hip_inv_txfm_add_batch_dev(e.h, 0, 1, 9, e.d, e.d, 64, e.d, 64, e.d, 0), BAD_ARG, b"svt_hip_inv_txfm_add_batch_dev: bad argument"),
    ("inv_batch-8bit-bytes-bd10", lambda e: e.L.svt_hip_inv_txfm_add_batch_dev(e.h, 0, 1, 10, e.d, e.d, 64, e.d, 64, e.d, 0), BAD_ARG, b"svt_hip_inv_txfm_add_batch_dev: bad argument"),
    ("inv_batch-tx_size", lambda e: e.L.svt_hip_inv_txfm_add_batch_dev(e.h, 19, 1, 8, e.d, e.d, 64, e.d, 64, e.d, 0), BAD_ARG, b"svt_hip_inv_txfm_add_batch_dev: bad argument"),
    ("iwht-pix_bytes", lambda e: e.L.svt_hip_iwht4x4_add_batch_dev(e.h, 3, 8, e.d, e.d, e.d, 64, e.d, 64, e.d, 0), BAD_ARG, b"svt_hip_iwht4x4_add_batch_dev: bad argument"),
    ("fwd_multi-pix_bytes", lambda e: fwd_multi(e, pix_bytes=3, njobs=0), BAD_ARG, SAME),
    ("fwd_multi-job.tx_size", lambda e: fwd_multi(e, tx_size=19), BAD_ARG, b"svt_hip_fwd_txfm_quant_multi_dev: bad job"),
    ("fwd_multi-job.qp.variant", lambda e: fwd_multi(e, variant=-1), BAD_ARG, b"svt_hip_fwd_txfm_quant_multi_dev: bad job"),
    ("fwd_multi-job.qp.coeff_shape", lambda e: fwd_multi(e, coeff_shape=4), BAD_ARG, b"svt_hip_fwd_txfm_quant_multi_dev: bad job"),
    ("enc_multi-bd", lambda e: enc_multi(e, bd=9, njobs=0), BAD_ARG, SAME),
    ("enc_multi-job.tx_size", lambda e: enc_multi(e, tx_size=19), BAD_ARG, b"svt_hip_enc_txfm_multi_dev: bad job"),
    ("enc_multi-job.qp.log_scale", lambda e: enc_multi(e, log_scale=3), BAD_ARG, b"svt_hip_enc_txfm_multi_dev: bad job"),
    ("inv_multi-pix_bytes", lambda e: inv_multi(e, pix_bytes=3, njobs=0), BAD_ARG, SAME),
    ("inv_multi-job.tx_size", lambda e: inv_multi(e, tx_size=19), BAD_ARG, b"svt_hip_inv_txfm_add_multi_dev: bad job"),
    ("quantize-qp.variant", lambda e: quantize(e, variant=4), BAD_ARG, SAME),
    ("quantize-qp.log_scale", lambda e: quantize(e, log_scale=3), BAD_ARG, SAME),
    ("quantize-n_coeffs", lambda e: quantize(e, n_coeffs=4097), BAD_ARG, SAME),
    ("transform64-tx_size", lambda e: e.L.svt_hip_handle_transform64_batch_dev(e.h, 3, e.d, 0, e.d), BAD_ARG, SAME),
    # deblocking
    ("deblock_plane-pix_bytes", lambda e: e.L.svt_hip_deblock_plane_dev(e.h, e.d, 3, 64, 8, e.d, e.d, 0, 0, 0), BAD_ARG, b"svt_hip_deblock_plane_dev: bad argument"),
    ("deblock_plane-sharpness", lambda e: e.L.svt_hip_deblock_plane_dev(e.h, e.d, 1, 64, 8, e.d, e.d, 0, 0, 8), BAD_ARG, b"svt_hip_deblock_plane_dev: bad argument"),
    ("deblock_frame-bd", lambda e: deblock_frame(e, bd=9), BAD_ARG, b"svt_hip_deblock_frame_dev: bad argument"),
    ("deblock_frame-units_w", lambda e: deblock_frame(e, units_w0=-1), BAD_ARG, SAME),
    ("deblock_fused-bd", lambda e: deblock_fused(e, bd=9), BAD_ARG, b"svt_hip_deblock_frame_fused_dev: bad argument"),
    ("deblock_fused-plane_w", lambda e: deblock_fused(e, plane_w0=0), BAD_ARG, b"svt_hip_deblock_frame_fused_dev: bad plane argument (the fused form is out of place)"),
    ("build_edges-ss_x", lambda e: build_edges(e, ss_x=2), BAD_ARG, b"svt_hip_dlf_build_edges_picture_dev: bad argument"),
    ("build_edges-filt_units_w", lambda e: build_edges(e, filt_units_w0=-1), BAD_ARG, b"svt_hip_dlf_build_edges_picture_dev: bad plane argument"),
    ("lpf_edges-bd", lambda e: e.L.svt_hip_lpf_edges_batch_dev(e.h, 1, 9, e.d, 64, e.d, 0), BAD_ARG, SAME),
    ("dlf_levels_picture-pix_bytes", lambda e: dlf_levels_picture(e, pix_bytes=3), BAD_ARG, SAME),
    ("dlf_levels_picture-plane_w", lambda e: dlf_levels_picture(e, plane_w=0), BAD_ARG, b"svt_hip_dlf_search_levels_picture_dev: bad plane"),
    ("dlf_level-bd", lambda e: dlf_level(e, bd=9), BAD_ARG, b"svt_hip_dlf_search_level_dev: bad argument"),
    ("plane_sse-pix_bytes", lambda e: e.L.svt_hip_plane_sse_dev(e.h, 3, e.d, 64, e.d, 64, 8, 8, e.d), BAD_ARG, b"svt_hip_plane_sse_dev: bad argument"),
    # CDEF
    ("cdef_search-pix_bytes", lambda e: cdef_search(e, pix_bytes=3), BAD_ARG, b"svt_hip_cdef_search_frame_dev: bad argument"),
    ("cdef_search-bd", lambda e: cdef_search(e, bd=9), BAD_ARG, b"svt_hip_cdef_search_frame_dev: bad argument"),
    ("cdef_search-w", lambda e: cdef_search(e, w=60), BAD_ARG, b"svt_hip_cdef_search_frame_dev: bad argument"),
    ("cdef_apply-bd", lambda e: cdef_apply(e, bd=9), BAD_ARG, b"svt_hip_cdef_apply_frame_dev: bad argument"),
    ("cdef_apply-h", lambda e: cdef_apply(e, h=0), BAD_ARG, b"svt_hip_cdef_apply_frame_dev: bad argument"),
    ("cdef_dist-coeff_shift", lambda e: e.L.svt_hip_cdef_dist_dev(e.h, 1, e.d, 64, e.d, e.d, 0, 3, 3, 5, 0, e.d), BAD_ARG, SAME),
    ("cdef_find_dir-coeff_shift", lambda e: e.L.svt_hip_cdef_find_dir_batch_dev(e.h, e.d, 64, e.d, 0, 5, e.d, e.d), BAD_ARG, SAME),
    ("cdef_finish-sb_count", lambda e: e.L.svt_hip_cdef_finish_dev(e.h, e.d, e.d, -1, e.d, 0, None, e.d, None, None, None), BAD_ARG, SAME),
    ("cdef_select-end_gi", lambda e: e.L.svt_hip_cdef_strength_select_dev(e.h, e.d, e.d, 0, 0, 65, e.d, e.pkg.CDEF_SELECT_STATE_BYTES), BAD_ARG, SAME),
    # the per-call list and single-unit forms: none of their refusals sets a text (the per-call table reads that as "delegate", not as a device failure)
    ("ext_all_sad-n", lambda e: e.L.svt_hip_ext_all_sad_8x8_16x16_batch_dev(e.h, e.d, 64, e.d, 64, e.d, -1, e.d), BAD_ARG, SAME),
    ("ext_all_sad-empty", lambda e: e.L.svt_hip_ext_all_sad_8x8_16x16_batch_dev(e.h, e.d, 64, e.d, 64, e.d, 0, e.d), OK, SAME),
    ("ext_eight_sad-n", lambda e: e.L.svt_hip_ext_eight_sad_32x32_64x64_batch_dev(e.h, e.d, -1, e.d), BAD_ARG, SAME),
    ("ext_eight_sad-empty", lambda e: e.L.svt_hip_ext_eight_sad_32x32_64x64_batch_dev(e.h, e.d, 0, e.d), OK, SAME),
    ("interm_var-n", lambda e: e.L.svt_hip_interm_var_four8x8_batch_dev(e.h, e.d, 64, e.d, -1, e.d, e.d), BAD_ARG, SAME),
    ("interm_var-empty", lambda e: e.L.svt_hip_interm_var_four8x8_batch_dev(e.h, e.d, 64, e.d, 0, e.d, e.d), OK, SAME),
    ("upsampled_pred-n", lambda e: e.L.svt_hip_upsampled_pred_batch_dev(e.h, e.d, 64, e.d, e.d, -1), BAD_ARG, SAME),
    ("upsampled_pred-empty", lambda e: e.L.svt_hip_upsampled_pred_batch_dev(e.h, e.d, 64, e.d, e.d, 0), OK, SAME),
    ("cdef_filter_block-n", lambda e: e.L.svt_hip_cdef_filter_block_batch_dev(e.h, e.d, 144, e.d, -1, e.d, None, 64), BAD_ARG, SAME),
    ("cdef_filter_block-empty", lambda e: e.L.svt_hip_cdef_filter_block_batch_dev(e.h, e.d, 144, e.d, 0, None, e.d, 64), OK, SAME),
    ("search_one_dual-nb_strengths", lambda e: e.L.svt_hip_cdef_search_one_dual_dev(e.h, e.d, e.d, 0, e.d, e.d, 8, 0, 64, e.d), BAD_ARG, SAME),
    ("search_one_dual-end_gi", lambda e: e.L.svt_hip_cdef_search_one_dual_dev(e.h, e.d, e.d, 0, e.d, e.d, 0, 0, 65, e.d), BAD_ARG, SAME),
    ("search_one_dual-start_gi", lambda e: e.L.svt_hip_cdef_search_one_dual_dev(e.h, e.d, e.d, 0, e.d, e.d, 0, 17, 16, e.d), BAD_ARG, SAME),
    ("search_one_dual-sb_count", lambda e: e.L.svt_hip_cdef_search_one_dual_dev(e.h, e.d, e.d, -1, e.d, e.d, 0, 0, 64, e.d), BAD_ARG, SAME),
    ("convolve8-step", lambda e: e.L.svt_hip_convolve8_dev(e.h, 0, e.d, 64, e.d, 64, e.d, 0, 65, 8, 8), BAD_ARG, SAME),
    ("convolve8-q0", lambda e: e.L.svt_hip_convolve8_dev(e.h, 1, e.d, 64, e.d, 64, e.d, 16, 16, 8, 8), BAD_ARG, SAME),
    ("convolve8-w", lambda e: e.L.svt_hip_convolve8_dev(e.h, 0, e.d, 64, e.d, 64, e.d, 0, 16, 0, 8), BAD_ARG, SAME),
    ("wiener_convolve-round_0", lambda e: e.L.svt_hip_wiener_convolve_add_src_dev(e.h, 1, 8, e.d, 64, e.d, 64, e.d, 8, 8, 8, 11), BAD_ARG, SAME),
    ("wiener_convolve-bd", lambda e: e.L.svt_hip_wiener_convolve_add_src_dev(e.h, 2, 13, e.d, 64, e.d, 64, e.d, 8, 8, 3, 11), BAD_ARG, SAME),
    ("wiener_convolve-h", lambda e: e.L.svt_hip_wiener_convolve_add_src_dev(e.h, 1, 8, e.d, 64, e.d, 64, e.d, 8, 0, 3, 11), BAD_ARG, SAME),
    ("jnt_convolve-variant", lambda e: e.L.svt_hip_jnt_convolve_dev(e.h, 1, 8, 4, e.d, 64, e.d, 64, e.d, 64, e.d, 8, 8, 3, 7, 0, 0, 0, 0), BAD_ARG, SAME),
    ("jnt_convolve-round_0", lambda e: e.L.svt_hip_jnt_convolve_dev(e.h, 1, 8, 0, e.d, 64, e.d, 64, e.d, 64, e.d, 8, 8, 2, 7, 0, 0, 0, 0), BAD_ARG, SAME),
    ("jnt_convolve-round_1", lambda e: e.L.svt_hip_jnt_convolve_dev(e.h, 2, 10, 0, e.d, 64, e.d, 64, e.d, 64, e.d, 8, 8, 5, 10, 0, 0, 0, 0), BAD_ARG, SAME),
    ("jnt_convolve-8bit-bytes-bd10", lambda e: e.L.svt_hip_jnt_convolve_dev(e.h, 1, 10, 0, e.d, 64, e.d, 64, e.d, 64, e.d, 8, 8, 3, 7, 0, 0, 0, 0), BAD_ARG, SAME),
    ("diffwtd_mask-round", lambda e: e.L.svt_hip_diffwtd_mask_dev(e.h, 2, e.d, e.d, 64, e.d, 64, 8, 8, 0, 16, 0), BAD_ARG, SAME),
    ("diffwtd_mask-shift", lambda e: e.L.svt_hip_diffwtd_mask_dev(e.h, 2, e.d, e.d, 64, e.d, 64, 8, 8, 0, 0, 9), BAD_ARG, SAME),
    ("diffwtd_mask-elem_bytes", lambda e: e.L.svt_hip_diffwtd_mask_dev(e.h, 3, e.d, e.d, 64, e.d, 64, 8, 8, 0, 0, 0), BAD_ARG, SAME),
    ("blend_a64_d16-round_0", lambda e: e.L.svt_hip_blend_a64_d16_dev(e.h, 1, 8, e.d, 64, e.d, 64, e.d, 64, e.d, 64, 8, 8, 0, 0, 6, 7), BAD_ARG, SAME),
    ("blend_a64_d16-bd", lambda e: e.L.svt_hip_blend_a64_d16_dev(e.h, 2, 13, e.d, 64, e.d, 64, e.d, 64, e.d, 64, 8, 8, 0, 0, 3, 7), BAD_ARG, SAME),
    ("blend_a64_d16-w", lambda e: e.L.svt_hip_blend_a64_d16_dev(e.h, 1, 8, e.d, 64, e.d, 64, e.d, 64, e.d, 64, 0, 8, 0, 0, 3, 7), BAD_ARG, SAME),
    ("sgr_flt_proj-mode", lambda e: e.L.svt_hip_sgr_flt_proj_dev(e.h, 1, e.d, 64, e.d, 64, e.d, 64, e.d, 64, 8, 8, 2, 1, 2, e.hp, e.d, e.d), BAD_ARG, SAME),
    ("sgr_flt_proj-pix_bytes", lambda e: e.L.svt_hip_sgr_flt_proj_dev(e.h, 3, e.d, 64, e.d, 64, e.d, 64, e.d, 64, 8, 8, 2, 1, 0, e.hp, e.d, e.d), BAD_ARG, SAME),
    ("sgr_flt_proj-w", lambda e: e.L.svt_hip_sgr_flt_proj_dev(e.h, 1, e.d, 64, e.d, 64, e.d, 64, e.d, 64, 0, 8, 2, 1, 1, e.hp, e.d, e.d), BAD_ARG, SAME),
    # md pictures
    ("md_sad-n_pus", lambda e: md_sad(e, n_pus=0), BAD_ARG, SAME),
    ("md_sad-n_refs", lambda e: md_sad(e, n_refs=0), BAD_ARG, SAME),
    ("md_sad-pu.w", lambda e: md_sad(e, pu_w=6), BAD_ARG, SAME),
    ("md_sad-pu.x", lambda e: md_sad(e, pu_x=60), BAD_ARG, SAME),
    ("md_sad-ref.stride", lambda e: md_sad(e, ref_stride=0), BAD_ARG, SAME),
    ("md_sad_hbd-pu.w", lambda e: md_sad(e, fn="svt_hip_md_fullpel_sad_picture_hbd_dev", pu_w=6), BAD_ARG, SAME),
    ("md_avg-n_pairs", lambda e: md_avg(e, n_pairs=0), BAD_ARG, SAME),
    ("md_avg-pair", lambda e: md_avg(e, pair0=1), BAD_ARG, SAME),
    ("md_avg-pu.w", lambda e: md_avg(e, pu_w=6), BAD_ARG, SAME),
    ("md_avg_hbd-ref.stride", lambda e: md_avg(e, fn="svt_hip_md_fullpel_avg_sad_picture_hbd_dev", ref_stride=0), BAD_ARG, SAME),
    ("md_grid-bank", lambda e: md_grid(e, bank=6), BAD_ARG, SAME),
    ("md_grid-pu.x", lambda e: md_grid(e, pu_x=60), BAD_ARG, SAME),
    ("md_grid-ref.stride", lambda e: md_grid(e, ref_stride=0), BAD_ARG, SAME),
    ("md_halfpel_grid-n_refs", lambda e: md_grid(e, fn="svt_hip_md_halfpel_grid_picture_dev", n_refs=0), BAD_ARG, SAME),
    # pyramids / SAD loops
    ("me_fullpel-stride", lambda e: e.L.svt_hip_me_fullpel_frame_dev(e.h, e.d, e.d, 6, 0, 0, e.d, 0, 0, e.d, e.d), BAD_ARG,
     b"svt_hip_me_fullpel_frame_dev: bad argument (stride must be a multiple of 4)"),
    ("variance_pyramid-stride", lambda e: e.L.svt_hip_variance_pyramid_dev(e.h, e.d, 12, 1, 0, 0, e.d, e.d), BAD_ARG,
     b"svt_hip_variance_pyramid_dev: bad argument (plane and stride must be 8-byte aligned)"),
    ("downsample-step", lambda e: e.L.svt_hip_downsample_2d_dev(e.h, e.d, 64, 8, 8, e.at(65536), 64, 3, 0), BAD_ARG, SAME),
    ("sad_loop-n", lambda e: e.L.svt_hip_sad_loop_batch_dev(e.h, e.d, 64, e.d, 64, e.d, -1, e.d, e.d), BAD_ARG, SAME),
    ("sad_loop16-n", lambda e: e.L.svt_hip_sad_loop16_batch_dev(e.h, e.d, 64, e.d, 64, e.d, -1, e.d, e.d), BAD_ARG, SAME),
    ("block_sad-pix_bytes", lambda e: e.L.svt_hip_block_sad_batch_dev(e.h, 3, e.d, 64, e.d, 64, e.d, 0, e.d), BAD_ARG, SAME),
    ("block_sse-pix_bytes", lambda e: e.L.svt_hip_block_sse_batch_dev(e.h, 3, e.d, 64, e.d, 64, e.d, 0, e.d), BAD_ARG, SAME),
    ("block_variance-bd12", lambda e: e.L.svt_hip_block_variance_batch_dev(e.h, 2, 12, e.d, 64, e.d, 64, e.d, 0, e.d, e.d), BAD_ARG, SAME),
    ("block_variance-8bit-bytes-bd16", lambda e: e.L.svt_hip_block_variance_batch_dev(e.h, 1, 16, e.d, 64, e.d, 64, e.d, 0, e.d, e.d), BAD_ARG, SAME),
    ("subpel_predict-bd", lambda e: e.L.svt_hip_subpel_predict_batch_dev(e.h, 2, 12, e.d, 64, e.d, 64, e.d, 0), BAD_ARG, b"svt_hip_subpel_predict_batch_dev: bad argument"),
    # temporal filter
    ("tf_filter-bd7", lambda e: tf_filter(e, pix_bytes=2, bd=7), BAD_ARG, TF_FILTER_TEXT),
    ("tf_filter-bd13", lambda e: tf_filter(e, pix_bytes=2, bd=13), BAD_ARG, TF_FILTER_TEXT),
    ("tf_filter-ss_y-without-ss_x", lambda e: tf_filter(e, ss=(0, 1)), BAD_ARG, TF_FILTER_TEXT),
    ("tf_filter-decay_control", lambda e: tf_filter(e, decay=0), BAD_ARG, TF_FILTER_TEXT),
    ("tf_filter-n_refs0", lambda e: tf_filter(e, n_refs=0), BAD_ARG, TF_FILTER_TEXT),
    ("tf_filter-n_refs17", lambda e: tf_filter(e, n_refs=17), BAD_ARG, TF_FILTER_TEXT),
    ("tf_filter-src-plane", lambda e: tf_filter(e, src0=False), BAD_ARG, SAME),
    ("tf_filter-pred-plane", lambda e: tf_filter(e, pred0=False), BAD_ARG, SAME),
    ("tf_noise-bd7", lambda e: tf_noise(e, pix_bytes=2, bd=7), BAD_ARG, SAME),
    ("tf_noise-bd13", lambda e: tf_noise(e, pix_bytes=2, bd=13), BAD_ARG, SAME),
    ("tf_noise-stride", lambda e: tf_noise(e, width=64, stride=63), BAD_ARG, SAME),
    ("tf_subpel-bd12", lambda e: tf_subpel(e, pix_bytes=2, bd=12), BAD_ARG, TF_SUBPEL_TEXT),
    ("tf_subpel-bd7", lambda e: tf_subpel(e, pix_bytes=2, bd=7), BAD_ARG, TF_SUBPEL_TEXT),
    ("tf_subpel-ref-plane", lambda e: tf_subpel(e, ref0=False), BAD_ARG, SAME),
    # copies and the zero-size successes: nothing is enqueued
    *[("%s-dpitch" % fn[8:], lambda e, fn=fn: copy2d(e, fn, dpitch=32), BAD_ARG, SAME) for fn in COPIES_2D],
    *[("%s-hpitch" % fn[8:], lambda e, fn=fn: copy2d(e, fn, hpitch=32), BAD_ARG, SAME) for fn in COPIES_2D],
    *[("%s-no-rows" % fn[8:], lambda e, fn=fn: copy2d(e, fn, rows=0), OK, SAME) for fn in COPIES_2D],
    *[("%s-no-width" % fn[8:], lambda e, fn=fn: copy2d(e, fn, wbytes=0), OK, SAME) for fn in COPIES_2D],
    ("memcpy_h2d_async-empty", lambda e: e.L.svt_hip_memcpy_h2d_async(e.h, e.d, e.hp, 0), OK, SAME),
    ("memcpy_d2h_async-empty", lambda e: e.L.svt_hip_memcpy_d2h_async(e.h, e.hp, e.d, 0), OK, SAME),
    ("memcpy_h2d_async-empty-null", lambda e: e.L.svt_hip_memcpy_h2d_async(e.h, None, None, 0), OK, SAME),
    ("memcpy_d2h_async-empty-null", lambda e: e.L.svt_hip_memcpy_d2h_async(e.h, None, None, 0), OK, SAME),
    ("memcpy_d2d-empty", lambda e: e.L.svt_hip_memcpy_d2d(e.h, e.at(65536), e.d, 0), OK, SAME),
    ("residual-no-width", lambda e: e.L.svt_hip_residual_dev(e.h, 1, e.d, 64, e.d, 64, e.at(65536), 64, 0, 8), OK, SAME),
    ("residual-no-height", lambda e: e.L.svt_hip_residual_dev(e.h, 2, e.d, 64, e.d, 64, e.at(65536), 64, 8, 0), OK, SAME),
    ("residual-pix_bytes", lambda e: e.L.svt_hip_residual_dev(e.h, 3, e.d, 64, e.d, 64, e.at(65536), 64, 0, 0), BAD_ARG, SAME),
    ("residual-w", lambda e: e.L.svt_hip_residual_dev(e.h, 1, e.d, 64, e.d, 64, e.at(65536), 64, -1, 0), BAD_ARG, SAME),
    # restoration
    ("sgr_units_plane-pix_bytes", lambda e: sgr_plane(e, pix_bytes=3), BAD_ARG, b"svt_hip_sgr_search_units_plane_dev: bad argument"),
    ("sgr_units_plane-bd", lambda e: sgr_plane(e, bd=9), BAD_ARG, b"svt_hip_sgr_search_units_plane_dev: bad argument"),
    ("sgr_units_plane-unit_size", lambda e: sgr_plane(e, unit_size=96), BAD_ARG, b"svt_hip_sgr_search_units_plane_dev: bad argument"),
    ("sgr_units_plane-ss_y", lambda e: sgr_plane(e, ss_y=2), BAD_ARG, b"svt_hip_sgr_search_units_plane_dev: bad argument"),
    ("sgr_units_plane-ep_mask", lambda e: sgr_plane(e, ep_mask=0x10000), BAD_ARG, b"svt_hip_sgr_search_units_plane_dev: bad argument"),
    ("sgr_units_picture-n_planes", lambda e: sgr_picture(e, n_planes=0), BAD_ARG, SAME),
    ("sgr_units_picture-bd", lambda e: sgr_picture(e, bd=9), BAD_ARG, b"svt_hip_sgr_search_units_picture_dev: bad plane"),
    ("sgr_units_picture-unit_size", lambda e: sgr_picture(e, unit_size=32), BAD_ARG, b"svt_hip_sgr_search_units_picture_dev: bad plane"),
    ("sgr_units_picture-ep_mask", lambda e: sgr_picture(e, ep_mask=0), BAD_ARG, b"svt_hip_sgr_search_units_picture_dev: bad plane"),
    ("sgr_search_plane-unit_size", lambda e: e.L.svt_hip_sgr_search_plane_dev(e.h, 1, 8, e.at(SGR_DGD), 128, e.d, 64, 64, 64, 32, 0, 0xFFFF, e.at(SGR_SCRATCH)), BAD_ARG, SAME),
    ("lr_apply-ss_y", lambda e: e.L.svt_hip_lr_apply_plane_dev(e.h, 1, 8, e.at(SGR_DGD), 128, e.at(SGR_SCRATCH), 64, 64, 64, 64, 2, None, 0, e.d, e.d, None), BAD_ARG, SAME),
    ("sgr_filter-ep", lambda e: e.L.svt_hip_sgr_filter_plane_dev(e.h, 1, 8, e.at(SGR_DGD), 128, 64, 64, 16, e.d, e.at(SGR_SCRATCH), 64), BAD_ARG, SAME),
    ("wiener_walk-wiener_win", lambda e: wiener_walk(e, wiener_win=4), BAD_ARG, b"svt_hip_wiener_walk_units_dev: bad argument"),
    ("wiener_walk-unit_size", lambda e: wiener_walk(e, unit_size=0), BAD_ARG, b"svt_hip_wiener_walk_units_dev: bad argument"),
    ("wiener_walk_picture-n_planes", lambda e: wiener_walk_picture(e, n_planes=4), BAD_ARG, SAME),
    ("wiener_walk_picture-ss_y", lambda e: wiener_walk_picture(e, ss_y=2), BAD_ARG, b"svt_hip_wiener_walk_units_picture_dev: bad plane"),
]


def check(e, call, rc, text):
    """SAME cases start from a text of another entry point, so that a text set by mistake cannot equal the one that was there."""
    if text is SAME:
        e.set_sentinel()
    before = e.last()
    assert call(e) == rc
    assert e.last() == (before if text is SAME else text)


@pytest.mark.parametrize("call,rc,text", [pytest.param(*c[1:], id=c[0]) for c in CASES])
def test_refused_call(env, call, rc, text):
    check(env, call, rc, text)


def test_case_ids_are_unique():
    assert len({c[0] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("packed", [None, "1"], ids=["sgr-6-byte", "sgr-packed"])
def test_sgr_scratch_one_byte_short(env, monkeypatch, packed):
    """The unit search refuses a scratch one byte smaller than svt_hip_sgr_search_units_scratch_bytes() asks for, in both forms of SVT_HIP_SGR_PACKED: the size
    that is checked belongs to the form that would be launched.  The switch is read on every call."""
    monkeypatch.delenv("SVT_HIP_SGR_PACKED", raising=False)
    plain = sgr_need(env)
    if packed:
        monkeypatch.setenv("SVT_HIP_SGR_PACKED", packed)
    need = sgr_need(env)
    assert need > plain if packed else need == plain
    assert 0 < need <= BUF_BYTES - SGR_SCRATCH   # the whole size is really there
    check(env, lambda e: sgr_plane(e, short=1), BAD_ARG, b"svt_hip_sgr_search_units_plane_dev: " + SCRATCH_TEXT)
    check(env, lambda e: sgr_picture(e, short=1), BAD_ARG, b"svt_hip_sgr_search_units_picture_dev: " + SCRATCH_TEXT)
    # at bit depth 10 there is no packed form: the 6-byte size is what both settings ask for
    check(env, lambda e: sgr_plane(e, short=need - plain + 1, pix_bytes=2, bd=10), BAD_ARG, b"svt_hip_sgr_search_units_plane_dev: " + SCRATCH_TEXT)
    if packed:   # ... and at bit depth 8 the 6-byte size is too small while the switch is on
        check(env, lambda e: sgr_plane(e, short=need - plain), BAD_ARG, b"svt_hip_sgr_search_units_plane_dev: " + SCRATCH_TEXT)
        check(env, lambda e: sgr_picture(e, short=need - plain), BAD_ARG, b"svt_hip_sgr_search_units_picture_dev: " + SCRATCH_TEXT)
