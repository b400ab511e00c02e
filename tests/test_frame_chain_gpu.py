"""GPU parity of the WHOLE bench step on a small frame: ME -> fwd txfm + quant -> inv txfm + recon ->
deblock -> CDEF search -> CDEF apply -> self-guided search -> self-guided apply (stripe-aware), every stage fed by the
previous stage's GPU output and compared with the oracle running the same chain (workload identical to bench.py's, tests/workload.py).
The same chain runs on 8-bit samples in 16-bit planes (pix_bytes 2, bd 8: what the encoder's 16-bit pipeline hands over for 8-bit video), against the
oracle at (2, 8) and against the 8-bit chain's outputs widened."""
import ctypes as C

import numpy as np
import pytest

from conftest import ptr
import me_common as mc
import txfm_common as tc
import workload
import fmt_common as fc
from test_txfm_gpu import oracle_block

pytestmark = pytest.mark.gpu
P3, I3 = C.c_void_p * 3, C.c_int * 3


def test_chain_small_frame(hip, pkg, orc):
    _chain(hip, pkg, orc, np.uint8)


def test_chain_small_frame_8bit_samples_in_16bit_planes(hip, pkg, orc):
    """ME stays 8-bit (it has no 16-bit form); every later stage runs at (pix_bytes 2, bd 8) on the widened planes, is fed by the previous stage's GPU output, and is
    compared with the oracle at (2, 8) (the transform stage block by block: orc_txfm_chain_8bit is 8-bit only) and with the 8-bit chain's output widened."""
    wide = _chain(hip, pkg, orc, np.uint16, extremes=True)
    narrow = _chain(hip, pkg, orc, np.uint8, extremes=True)
    assert wide.keys() == narrow.keys()
    for k in wide:
        a, b = wide[k], narrow[k]
        if b.dtype == np.uint8 and a.dtype == np.uint16:
            fc.check_8bit_range(a)          # every stage's samples stay inside 0 .. 255 and reach both ends
            b = b.astype(np.uint16)
        assert a.dtype == b.dtype and np.array_equal(a, b), k


def _plant(cur, ref):
    """in every plane of the current and the predicted picture: all max in both, all 0 in both (no residual: the reconstruction sits on the end of the range), and a
    0 / max checkerboard against its complement (residuals of +-max sample by sample: the inverse transform overshoots both ends and the clip decides)"""
    yy, xx = np.mgrid[0:32, 0:32]
    for c, r in zip(cur, ref):
        c[:32, :32] = 255; r[:32, :32] = 255
        c[:32, 32:64] = 0; r[:32, 32:64] = 0
        c[32:64, :32] = ((yy + xx) & 1) * 255; r[32:64, :32] = (1 - ((yy + xx) & 1)) * 255


def _oracle_txfm_blocks(orc, F, cur, ref, recon, plane, ts, descs, scans):
    """the transform stage of one (plane, size) list at (2, 8), block by block with the oracle calls of tests/test_txfm_gpu.py: residual, forward transform, quantiser
    variant 0, inverse transform + reconstruction on the 16-bit prediction"""
    w, h = tc.TXW[ts], tc.TXH[ts]
    nk = min(w, 32) * min(h, 32)
    q = np.zeros((len(descs), nk), np.int32); eob = np.zeros(len(descs), np.uint16)
    for i, d in enumerate(descs):
        x, y, tt = int(d) & 0x3FFF, (int(d) >> 14) & 0x3FFF, int(d) >> 28
        cls = tc.SCAN_CLASS[tt] if w <= 16 and h <= 16 else 0
        _, _, q[i], dq, eob[i], _ = oracle_block(orc, ts, tt, 8, cur[plane], ref[plane], x, y, F.qp[plane], 0, scans[cls])
        exp = np.zeros((h, w), np.uint16)
        orc.orc_inv_txfm2d_add(ptr(np.ascontiguousarray(dq)), ptr(np.ascontiguousarray(ref[plane][y:y + h, x:x + w])), w, ptr(exp), w, tt, ts, 8)
        recon[plane][y:y + h, x:x + w] = exp
    return q, eob


def _chain(hip, pkg, orc, dt, extremes=False):
    """-> {stage: device output} of the chain on planes of sample type dt (uint8, or uint16 holding the same 8-bit samples)"""
    W, H = 336, 208     # 6 x 4 SBs, ragged last column (16 px) / row (16 px)
    F = workload.Frame(W, H, seed=5)
    L = hip.L
    pb = np.dtype(dt).itemsize
    cur, ref = [p.astype(dt) for p in F.cur], [p.astype(dt) for p in F.ref]
    if extremes: _plant(cur, ref)
    out = {}
    # ---------------- oracle chain
    sbs = mc.windows(orc, W, H, 64, 64)
    o_sad, o_mv = mc.oracle_frame(orc, F.cur_y_p, F.ref_y_p, F.cur_y_p.shape[1], F.pad, sbs, 0)
    o_recon = [p.copy() for p in ref]
    o_q = {}
    for (kind, ts), descs in sorted(F.descs.items()):
        nk = min(tc.TXW[ts], 32) * min(tc.TXH[ts], 32)
        scans = F.scans(ts)
        SC = (C.c_void_p * 3)(*[s.ctypes.data if s is not None else None for s in scans])
        for plane in ([0] if kind == 0 else [1, 2]):
            q = np.zeros((len(descs), nk), np.int32); eob = np.zeros(len(descs), np.uint16)
            if pb == 1:
                orc.orc_txfm_chain_8bit(ptr(cur[plane]), cur[plane].shape[1], ptr(ref[plane]), ref[plane].shape[1], ptr(o_recon[plane]),
                                        o_recon[plane].shape[1], ptr(descs), 0, len(descs), ts, 0, ptr(F.qp[plane]), SC, tc.TX_SCALE[ts], ptr(q), ptr(eob))
            else:
                q, eob = _oracle_txfm_blocks(orc, F, cur, ref, o_recon, plane, ts, descs, scans)
            o_q[(plane, ts)] = (q, eob)
    o_dlf = [p.copy() for p in o_recon]
    for p in range(3):
        ev, eh = F.edges[p]
        orc.orc_deblock_plane(ptr(o_dlf[p]), pb, o_dlf[p].shape[1], 8, ptr(ev), ptr(eh), ev.shape[1], ev.shape[0], 0)
    o_mse = np.zeros((2, F.n_sb, 64), np.uint64)
    orc.orc_cdef_search_frame(P3(*[p.ctypes.data for p in o_dlf]), I3(*[p.shape[1] for p in o_dlf]), P3(*[p.ctypes.data for p in cur]),
                              I3(*[p.shape[1] for p in cur]), pb, W, H, ptr(F.skip8), F.cdef_damping, 8, 0, ptr(o_mse), 0, F.n_sb)
    o_out = [p.copy() for p in o_dlf]
    orc.orc_cdef_apply_frame(P3(*[p.ctypes.data for p in o_dlf]), P3(*[p.ctypes.data for p in o_out]), I3(*[p.shape[1] for p in o_dlf]), pb, W, H,
                             ptr(F.skip8), ptr(F.cdef_y), ptr(F.cdef_uv), F.cdef_damping, 8)
    # ---------------- HIP chain
    g_sad, g_mv = mc.hip_frame(hip, F.cur_y_p, F.ref_y_p, F.cur_y_p.shape[1], F.pad, sbs, 0)
    assert np.array_equal(g_sad, o_sad) and np.array_equal(g_mv, o_mv)
    d_cur = [hip.to_device(p) for p in cur]; d_pred = [hip.to_device(p) for p in ref]
    d_rec = [hip.to_device(p) for p in ref]
    strides = [p.shape[1] for p in cur]
    for (kind, ts), descs in sorted(F.descs.items()):
        nk = min(tc.TXW[ts], 32) * min(tc.TXH[ts], 32)
        d_desc = hip.to_device(descs)
        st = pkg.ScanTables(); keep = []
        for c, s in enumerate(F.scan_tables(ts)):
            if s is not None:
                p = hip.to_device(s); keep.append(p); st.iscan[c] = p.value
        for plane in ([0] if kind == 0 else [1, 2]):
            qs = pkg.QuantParams(); qp = F.qp[plane]
            for name, row in (("zbin", qp[0]), ("round", qp[1]), ("quant", qp[2]), ("quant_shift", qp[3]), ("dequant", qp[4])):
                getattr(qs, name)[0] = int(row[0]); getattr(qs, name)[1] = int(row[1])
            qs.log_scale = tc.TX_SCALE[ts]; qs.variant = 0
            n = len(descs)
            d_q, d_dq, d_eob = hip.empty(n * nk * 4), hip.empty(n * nk * 4), hip.empty(n * 2)
            hip.check(L.svt_hip_fwd_txfm_quant_batch_dev(hip.h, ts, pb, d_cur[plane], strides[plane], d_pred[plane], strides[plane], d_desc, n,
                                                        C.byref(qs), C.byref(st), None, d_q, d_dq, d_eob, None, None))
            hip.check(L.svt_hip_inv_txfm_add_batch_dev(hip.h, ts, pb, 8, d_dq, d_pred[plane], strides[plane], d_rec[plane], strides[plane], d_desc, n))
            q = hip.to_host(d_q, (n, nk), np.int32); eob = hip.to_host(d_eob, (n,), np.uint16)
            assert np.array_equal(q, o_q[(plane, ts)][0]) and np.array_equal(eob, o_q[(plane, ts)][1]), (plane, ts)
            out[f"q {plane} {ts}"] = q; out[f"eob {plane} {ts}"] = eob
            hip.free(d_q, d_dq, d_eob)
        hip.free(d_desc, *keep)
    for p in range(3):
        out[f"recon {p}"] = hip.to_host(d_rec[p], ref[p].shape, dt)
        assert np.array_equal(out[f"recon {p}"], o_recon[p]), ("recon", p)
        ev, eh = F.edges[p]
        d_ev, d_eh = hip.to_device(ev), hip.to_device(eh)
        hip.check(L.svt_hip_deblock_plane_dev(hip.h, d_rec[p], pb, strides[p], 8, d_ev, d_eh, ev.shape[1], ev.shape[0], 0))
        out[f"deblock {p}"] = hip.to_host(d_rec[p], ref[p].shape, dt)
        assert np.array_equal(out[f"deblock {p}"], o_dlf[p]), ("deblock", p)
        hip.free(d_ev, d_eh)
    d_skip = hip.to_device(F.skip8)
    d_mse = hip.to_device(np.zeros((2, F.n_sb, 64), np.uint64)); d_dir = hip.empty(F.n_sb * 64); d_var = hip.empty(F.n_sb * 256)
    hip.check(L.svt_hip_cdef_search_frame_dev(hip.h, pb, P3(*[p.value for p in d_rec]), I3(*strides), P3(*[p.value for p in d_cur]), I3(*strides),
                                             W, H, d_skip, F.cdef_damping, 8, d_mse, d_dir, d_var))
    out["cdef mse"] = hip.to_host(d_mse, (2, F.n_sb, 64), np.uint64)
    assert np.array_equal(out["cdef mse"], o_mse)
    d_out = [hip.to_device(p) for p in o_dlf]
    d_cy, d_cuv = hip.to_device(F.cdef_y), hip.to_device(F.cdef_uv)
    hip.check(L.svt_hip_cdef_apply_frame_dev(hip.h, pb, P3(*[p.value for p in d_rec]), P3(*[p.value for p in d_out]), I3(*strides), W, H, d_skip,
                                            d_cy, d_cuv, F.cdef_damping, 8, d_dir, d_var))
    for p in range(3):
        out[f"cdef {p}"] = hip.to_host(d_out[p], ref[p].shape, dt)
        assert np.array_equal(out[f"cdef {p}"], o_out[p]), ("cdef apply", p)
    # ---------------- loop restoration on the CDEF output; stripe context rows come from the deblocked picture (d_rec)
    EXT, US = 3, 64
    rng = np.random.default_rng(77)
    for p in range(3):
        ss = int(p > 0)
        ph, pw = o_out[p].shape
        ext = np.ascontiguousarray(np.pad(o_out[p], EXT, mode="edge")); st = ext.shape[1]; off = (EXT * st + EXT) * pb
        nu = max((pw + US // 2) // US, 1) * max((ph + US // 2) // US, 1)
        e_sums = np.zeros((nu, 16, 5), np.int64)
        orc.orc_sgr_search_plane(C.c_void_p(ext.ctypes.data + off), pb, st, ptr(cur[p]), cur[p].shape[1], pw, ph, ss, ss, US, 8, 0xFFFF, ptr(e_sums))
        u_ep = rng.integers(0, 16, nu).astype(np.uint8); u_ep[nu // 2] = 255
        u_xqd = np.stack([rng.integers(-96, 32, nu), rng.integers(-32, 96, nu)], 1).astype(np.int32)
        e_dst = np.zeros((ph, pw), dt)
        work = ext.copy()
        orc.orc_sgr_apply_plane(ptr(o_dlf[p]), o_dlf[p].shape[1], C.c_void_p(work.ctypes.data + off), st, pb, pw, ph, ss, ss, US, 8, ptr(u_ep), ptr(u_xqd), ptr(e_dst), pw)
        d_ext, d_sums, d_dst, d_ep, d_xqd = hip.to_device(ext), hip.to_device(np.zeros_like(e_sums)), hip.to_device(np.zeros_like(e_dst)), hip.to_device(u_ep), hip.to_device(u_xqd)
        hip.check(L.svt_hip_sgr_search_plane_dev(hip.h, pb, 8, d_ext.value + off, st, d_cur[p], strides[p], pw, ph, US, ss, 0xFFFF, d_sums), "sgr search")
        out[f"sgr sums {p}"] = hip.to_host(d_sums, e_sums.shape, np.int64)
        assert np.array_equal(out[f"sgr sums {p}"], e_sums), ("sgr search", p)
        hip.check(L.svt_hip_sgr_apply_plane_dev(hip.h, pb, 8, d_ext.value + off, st, d_dst, pw, pw, ph, US, ss, d_rec[p], strides[p], d_ep, d_xqd), "sgr apply")
        out[f"sgr {p}"] = hip.to_host(d_dst, e_dst.shape, dt)
        assert np.array_equal(out[f"sgr {p}"], e_dst), ("sgr apply", p)
        hip.free(d_ext, d_sums, d_dst, d_ep, d_xqd)
    hip.free(*d_cur, *d_pred, *d_rec, *d_out, d_skip, d_mse, d_dir, d_var, d_cy, d_cuv)
    return out
