"""svt-av1_amd — host-side Python binding (ctypes) of libsvtav1_hip.so.

The product is the C-ABI shared library declared in include/svt_hip.h (built from csrc/ by
__graft_entry__.build()).  This module only loads it and mirrors the prototypes so that tests and
bench.py can drive it; there is NO CPU fallback here: if the library is missing, or no gfx950
device is present, loading / svt_hip_init fails loudly.

The directory name contains a '-', so import it through `load_package()` in tests/conftest.py
(importlib, module name `svt_av1_amd`).
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsvtav1_hip.so")

SQUARE_PU_COUNT = 85
MAX_SAD_VALUE = 128 * 128 * 255


class SbSearch(C.Structure):
    """SvtHipSbSearch (include/svt_hip.h)."""
    _fields_ = [("sb_x", C.c_int32), ("sb_y", C.c_int32), ("x_origin", C.c_int16), ("y_origin", C.c_int16),
                ("width", C.c_int16), ("height", C.c_int16)]


class QuantParams(C.Structure):
    """SvtHipQuantParams (include/svt_hip.h)."""
    _fields_ = [("zbin", C.c_int32 * 2), ("round", C.c_int32 * 2), ("quant", C.c_int32 * 2), ("quant_shift", C.c_int32 * 2),
                ("dequant", C.c_int32 * 2), ("log_scale", C.c_int32), ("variant", C.c_int32), ("coeff_shape", C.c_int32)]


class SgrSearchPlane(C.Structure):
    """SvtHipSgrSearchPlane (include/svt_hip.h)."""
    _fields_ = [("d_dgd", C.c_void_p), ("stride", C.c_int32), ("d_src", C.c_void_p), ("src_stride", C.c_int32), ("pw", C.c_int32), ("ph", C.c_int32),
                ("unit_size", C.c_int32), ("ss_y", C.c_int32), ("ep_mask", C.c_uint32), ("xqd_out", C.c_void_p), ("err_out", C.c_void_p),
                ("best_ep", C.c_void_p)]


class ScanTables(C.Structure):
    """SvtHipScanTables (include/svt_hip.h): device pointers."""
    _fields_ = [("iscan", C.c_void_p * 3)]


class DlfModeInfo(C.Structure):
    """SvtHipDlfModeInfo (include/svt_hip.h)."""
    _fields_ = [("tx_w_log2", C.c_uint8), ("tx_h_log2", C.c_uint8), ("uv_tx_w_log2", C.c_uint8), ("uv_tx_h_log2", C.c_uint8),
                ("bw_log2", C.c_uint8), ("bh_log2", C.c_uint8), ("skip_inter", C.c_uint8), ("level", (C.c_uint8 * 2) * 3)]


class ConvBlk(C.Structure):
    """SvtHipConvBlk (include/svt_hip.h)."""
    _fields_ = [("src_x", C.c_int32), ("src_y", C.c_int32), ("dst_x", C.c_int32), ("dst_y", C.c_int32), ("w", C.c_uint8), ("h", C.c_uint8),
                ("bank_x", C.c_uint8), ("bank_y", C.c_uint8), ("subpel_x", C.c_uint8), ("subpel_y", C.c_uint8), ("mode", C.c_uint8),
                ("reserved", C.c_uint8)]


class WienerWalkPlane(C.Structure):
    """SvtHipWienerWalkPlane (include/svt_hip.h)"""
    _fields_ = [("d_dgd", C.c_void_p), ("stride", C.c_int32), ("pw", C.c_int32), ("ph", C.c_int32), ("unit_size", C.c_int32), ("ss_y", C.c_int32), ("d_dbl", C.c_void_p),
                ("dbl_stride", C.c_int32), ("d_src", C.c_void_p), ("src_stride", C.c_int32), ("d_unit_wiener", C.c_void_p), ("d_active", C.c_void_p), ("wiener_win", C.c_int32),
                ("d_err", C.c_void_p), ("d_probes", C.c_void_p)]


class MdPu(C.Structure):
    """SvtHipMdPu (include/svt_hip.h)."""
    _fields_ = [("x", C.c_uint8), ("y", C.c_uint8), ("w", C.c_uint8), ("h", C.c_uint8)]


class MdRefPlane(C.Structure):
    """SvtHipMdRefPlane (include/svt_hip.h)."""
    _fields_ = [("d_plane", C.c_void_p), ("stride", C.c_int32), ("x_min", C.c_int32), ("y_min", C.c_int32), ("x_max", C.c_int32), ("y_max", C.c_int32)]


class UpsampledBlk(C.Structure):
    """SvtHipUpsampledBlk (include/svt_hip.h)."""
    _fields_ = [("ref_off", C.c_int32), ("dst_off", C.c_int32), ("w", C.c_uint8), ("h", C.c_uint8), ("subpel_x_q3", C.c_uint8), ("subpel_y_q3", C.c_uint8), ("bank", C.c_uint8),
                ("reserved", C.c_uint8 * 3)]


class BlkPair(C.Structure):
    """SvtHipBlkPair (include/svt_hip.h)."""
    _fields_ = [("a_x", C.c_int32), ("a_y", C.c_int32), ("b_x", C.c_int32), ("b_y", C.c_int32), ("w", C.c_uint16), ("h", C.c_uint16)]


class SadLoop(C.Structure):
    """SvtHipSadLoop (include/svt_hip.h)."""
    _fields_ = [("src_x", C.c_int32), ("src_y", C.c_int32), ("ref_x", C.c_int32), ("ref_y", C.c_int32), ("bw", C.c_int16), ("bh", C.c_int16),
                ("sa_w", C.c_int16), ("sa_h", C.c_int16), ("row_step", C.c_int16), ("reserved", C.c_int16)]


class FwdTxJob(C.Structure):
    """SvtHipFwdTxJob (include/svt_hip.h)."""
    _fields_ = [("tx_size", C.c_int32), ("nblk", C.c_int32), ("d_src", C.c_void_p), ("src_stride", C.c_int32), ("d_pred", C.c_void_p),
                ("pred_stride", C.c_int32), ("d_descs", C.c_void_p), ("qp", QuantParams), ("scans", ScanTables), ("d_coeff", C.c_void_p),
                ("d_qcoeff", C.c_void_p), ("d_dqcoeff", C.c_void_p), ("d_eob", C.c_void_p), ("d_cul_level", C.c_void_p), ("d_energy", C.c_void_p)]


class EncTxJob(C.Structure):
    """SvtHipEncTxJob (include/svt_hip.h)."""
    _fields_ = [("fwd", FwdTxJob), ("d_recon", C.c_void_p), ("recon_stride", C.c_int32)]


class InvTxJob(C.Structure):
    """SvtHipInvTxJob (include/svt_hip.h)."""
    _fields_ = [("tx_size", C.c_int32), ("nblk", C.c_int32), ("d_dqcoeff", C.c_void_p), ("d_pred", C.c_void_p), ("pred_stride", C.c_int32),
                ("d_recon", C.c_void_p), ("recon_stride", C.c_int32), ("d_descs", C.c_void_p)]


class SgrUnitsPlaneDev(C.Structure):   # SvtHipSgrUnitsPlaneDev
    _fields_ = [("d_dgd", C.c_void_p), ("stride", C.c_int32), ("d_src", C.c_void_p), ("src_stride", C.c_int32), ("pw", C.c_int32), ("ph", C.c_int32),
                ("unit_size", C.c_int32), ("ss_y", C.c_int32), ("ep_mask", C.c_uint32), ("d_xqd", C.c_void_p), ("d_err", C.c_void_p), ("d_best_ep", C.c_void_p),
                ("d_best_xqd", C.c_void_p), ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


class TfBlk64(C.Structure):   # SvtHipTfBlk64
    _fields_ = [("mv16_x", C.c_int16 * 16), ("mv16_y", C.c_int16 * 16), ("err16", C.c_uint64 * 16),
                ("mv32_x", C.c_int16 * 4), ("mv32_y", C.c_int16 * 4), ("err32", C.c_uint64 * 4), ("split", C.c_int32 * 4)]


class TfSubpelBlk(C.Structure):   # SvtHipTfSubpelBlk
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("dst_x", C.c_int32), ("dst_y", C.c_int32), ("blk_index", C.c_int32),
                ("mv32", C.c_uint32 * 4), ("mv16", C.c_uint32 * 16)]


class TfRef(C.Structure):     # SvtHipTfRef
    _fields_ = [("pred", C.c_void_p * 3), ("pred_stride", C.c_int * 3), ("blocks", C.c_void_p)]


class CompBlk(C.Structure):
    """SvtHipCompBlk (include/svt_hip.h)."""
    _fields_ = [("src0_x", C.c_int32), ("src0_y", C.c_int32), ("src1_x", C.c_int32), ("src1_y", C.c_int32), ("dst_x", C.c_int32), ("dst_y", C.c_int32),
                ("w", C.c_uint8), ("h", C.c_uint8), ("bank_x", C.c_uint8), ("bank_y", C.c_uint8),
                ("subpel0_x", C.c_uint8), ("subpel0_y", C.c_uint8), ("subpel1_x", C.c_uint8), ("subpel1_y", C.c_uint8),
                ("type", C.c_uint8), ("fwd_offset", C.c_uint8), ("bck_offset", C.c_uint8), ("mask_type", C.c_uint8),
                ("mask_sub", C.c_uint8), ("reserved", C.c_uint8 * 3), ("mask_off", C.c_int32), ("mask_stride", C.c_int32)]


class ObmcBlk(C.Structure):
    """SvtHipObmcBlk (include/svt_hip.h)."""
    _fields_ = [("pre_x", C.c_int32), ("pre_y", C.c_int32), ("w", C.c_uint8), ("h", C.c_uint8), ("xoffset", C.c_uint8), ("yoffset", C.c_uint8), ("wm_off", C.c_int32)]


class ObmcTargetJob(C.Structure):
    """SvtHipObmcTargetJob (include/svt_hip.h)."""
    _fields_ = [("bsize", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("n_above", C.c_int32), ("above_rel", C.c_int32 * 4), ("above_len", C.c_int32 * 4),
                ("n_left", C.c_int32), ("left_rel", C.c_int32 * 4), ("left_len", C.c_int32 * 4), ("above_off", C.c_int32), ("above_stride", C.c_int32),
                ("left_off", C.c_int32), ("left_stride", C.c_int32), ("wm_off", C.c_int32)]


class ObmcSearchJob(C.Structure):
    """SvtHipObmcSearchJob (include/svt_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("bsize", "mi_row", "mi_col", "wm_off", "mv_row", "mv_col", "ref_mv_row", "ref_mv_col", "sad_per_bit", "error_per_bit", "allow_hp")]


class ObmcSearchResult(C.Structure):
    """SvtHipObmcSearchResult (include/svt_hip.h)."""
    _fields_ = [(n, C.c_uint32 if n in ("besterr", "sse") else C.c_int32) for n in ("status", "full_row", "full_col", "refining", "steps", "bestsme", "row", "col", "besterr",
                                                                                   "distortion", "sse", "rate_mv")]


class WarpBlk(C.Structure):
    """SvtHipWarpBlk (include/svt_hip.h)."""
    _fields_ = [("mat", C.c_int32 * 6), ("alpha", C.c_int16), ("beta", C.c_int16), ("gamma", C.c_int16), ("delta", C.c_int16),
                ("p_col", C.c_int32), ("p_row", C.c_int32), ("p_width", C.c_uint8), ("p_height", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class WarpCompBlk(C.Structure):
    """SvtHipWarpCompBlk (include/svt_hip.h)."""
    _fields_ = [("blk", WarpBlk), ("cb_off", C.c_int32), ("cb_stride", C.c_int32), ("do_average", C.c_uint8), ("use_jnt_comp_avg", C.c_uint8),
                ("fwd_offset", C.c_uint8), ("bck_offset", C.c_uint8)]


class BlendBlk(C.Structure):
    """SvtHipBlendBlk (include/svt_hip.h)."""
    _fields_ = [("src0_x", C.c_int32), ("src0_y", C.c_int32), ("src1_x", C.c_int32), ("src1_y", C.c_int32), ("dst_x", C.c_int32), ("dst_y", C.c_int32),
                ("w", C.c_uint8), ("h", C.c_uint8), ("mode", C.c_uint8), ("subw", C.c_uint8), ("subh", C.c_uint8), ("reserved", C.c_uint8 * 3),
                ("mask_off", C.c_int32), ("mask_stride", C.c_int32)]


class ExtSadJob(C.Structure):
    """SvtHipExtSadJob (include/svt_hip.h)."""
    _fields_ = [("src_off", C.c_int32), ("ref_off", C.c_int32), ("mv", C.c_uint32), ("sub_sad", C.c_int32)]


class CdefSelectResult(C.Structure):
    """SvtHipCdefSelectResult (include/svt_hip.h): the head of the selection's state."""
    _fields_ = [("lev0", (C.c_int32 * 8) * 4), ("lev1", (C.c_int32 * 8) * 4), ("status", C.c_uint32 * 4), ("tot_mse", C.c_uint64 * 4)]


CDEF_SELECT_STATE_BYTES = C.sizeof(CdefSelectResult) + 8192 + 4 * 128 * 4096 * 8   # SVT_HIP_CDEF_SELECT_STATE_BYTES


class CdefFinish(C.Structure):
    """SvtHipCdefFinish (include/svt_hip.h)."""
    _fields_ = [("cdef_bits", C.c_int32), ("nb_strengths", C.c_int32), ("y_strength", C.c_int32 * 8), ("uv_strength", C.c_int32 * 8), ("best_cost", C.c_uint64)]


class CdefBlk(C.Structure):
    """SvtHipCdefBlk (include/svt_hip.h)."""
    _fields_ = [("in_off", C.c_int32), ("dst_off", C.c_int32), ("pri_strength", C.c_int32), ("sec_strength", C.c_int32), ("dir", C.c_int32),
                ("pri_damping", C.c_int32), ("sec_damping", C.c_int32), ("bw_log2", C.c_int32), ("bh_log2", C.c_int32), ("coeff_shift", C.c_int32)]


class LpfEdge(C.Structure):
    """SvtHipLpfEdge (include/svt_hip.h)."""
    _fields_ = [("off", C.c_int32), ("dir", C.c_uint8), ("len", C.c_uint8), ("blimit", C.c_uint8), ("limit", C.c_uint8), ("thresh", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class DlfSearch(C.Structure):
    """SvtHipDlfSearch (include/svt_hip.h)."""
    _fields_ = [("plane", C.c_int), ("dir", C.c_int), ("other_level", C.c_int), ("start_level", C.c_int), ("loop_filter_mode", C.c_int),
                ("tx_mode_only_4x4", C.c_int), ("sharpness", C.c_int)]


class DlfSearchPlane(C.Structure):
    """SvtHipDlfSearchPlane (include/svt_hip.h)."""
    _fields_ = [("q", DlfSearch), ("d_recon", C.c_void_p), ("d_tmp", C.c_void_p * 2), ("stride", C.c_int), ("plane_w", C.c_int), ("plane_h", C.c_int), ("d_src", C.c_void_p),
                ("src_stride", C.c_int), ("d_edges_v", C.c_void_p), ("d_edges_h", C.c_void_p), ("units_w", C.c_int), ("units_h", C.c_int)]


class IntraJob(C.Structure):
    """SvtHipIntraJob (include/svt_hip.h)."""
    _fields_ = [("edge_off", C.c_uint32), ("dst_x", C.c_int32), ("dst_y", C.c_int32), ("tx_size", C.c_uint8), ("mode", C.c_uint8), ("angle_delta", C.c_int8),
                ("dc_have", C.c_uint8), ("corner_filter", C.c_uint8), ("strength_above", C.c_uint8), ("strength_left", C.c_uint8), ("npx_above", C.c_uint8),
                ("npx_left", C.c_uint8), ("start_m1", C.c_uint8), ("upsample_above", C.c_uint8), ("upsample_left", C.c_uint8), ("up_npx_above", C.c_uint8),
                ("up_npx_left", C.c_uint8)]


class CflJob(C.Structure):
    """SvtHipCflJob (include/svt_hip.h)."""
    _fields_ = [("luma_x", C.c_int32), ("luma_y", C.c_int32), ("dst_x", C.c_int32), ("dst_y", C.c_int32), ("edge_off", C.c_uint32 * 2), ("alpha_q3", C.c_int8 * 2),
                ("tx_size", C.c_uint8), ("plane_mask", C.c_uint8), ("dc_from_edges", C.c_uint8), ("dc_have", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class FilterIntraJob(C.Structure):
    """SvtHipFilterIntraJob (include/svt_hip.h)."""
    _fields_ = [("edge_off", C.c_uint32), ("dst_x", C.c_int32), ("dst_y", C.c_int32), ("tx_size", C.c_uint8), ("mode", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class TplRef(C.Structure):
    """SvtHipTplRef (include/svt_hip.h): device pointers to sample (0, 0)."""
    _fields_ = [("d_src", C.c_void_p), ("d_rec", C.c_void_p), ("src_stride", C.c_int32), ("rec_stride", C.c_int32)]


class TplParams(C.Structure):
    """SvtHipTplParams (include/svt_hip.h)."""
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("pad", C.c_int32), ("q", QuantParams), ("use_ois", C.c_uint8), ("add_residual", C.c_uint8),
                ("rate", C.c_uint8), ("best_ref_only", C.c_uint8)]


class TplMbStats(C.Structure):
    """SvtHipTplMbStats (include/svt_hip.h)."""
    _fields_ = [("srcrf_dist", C.c_int64), ("recrf_dist", C.c_int64), ("srcrf_rate", C.c_int64), ("recrf_rate", C.c_int64), ("mv_row", C.c_int16),
                ("mv_col", C.c_int16), ("rf_idx", C.c_int8), ("is_inter", C.c_uint8), ("mode", C.c_uint8), ("pad0", C.c_uint8), ("eob", C.c_uint16),
                ("pad1", C.c_uint16)]


class TplWindowFrame(C.Structure):
    """SvtHipTplWindowFrame (include/svt_hip.h): d_stats / d_dep are device pointers for the *_dev entry points, host pointers for tpl_window_host."""
    _fields_ = [("d_stats", C.c_void_p), ("d_dep", C.c_void_p), ("on", C.c_int32), ("ref_window", C.c_int32 * 8), ("reserved", C.c_int32)]


class TplSynthParams(C.Structure):
    """SvtHipTplSynthParams (include/svt_hip.h)."""
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("cell_log2", C.c_int32), ("sb_size", C.c_int32), ("base_rdmult", C.c_int32), ("rate", C.c_int32),
                ("r0_in", C.c_double)]


class TplR0BetaHeader(C.Structure):
    """SvtHipTplR0BetaHeader (include/svt_hip.h)."""
    _fields_ = [("r0", C.c_double), ("intra_cost_base", C.c_int64), ("mc_dep_cost_base", C.c_int64)]


class GmModel(C.Structure):
    """SvtHipGmModel (include/svt_hip.h)."""
    _fields_ = [("mat", C.c_int32 * 6), ("alpha", C.c_int16), ("beta", C.c_int16), ("gamma", C.c_int16), ("delta", C.c_int16), ("valid", C.c_int32)]


class GmRef(C.Structure):
    """SvtHipGmRef (include/svt_hip.h): device pointer to sample (0, 0)."""
    _fields_ = [("d_plane", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("reserved", C.c_int32)]


class GmJob(C.Structure):
    """SvtHipGmJob (include/svt_hip.h)."""
    _fields_ = [("ref", C.c_int32), ("wmtype", C.c_int32), ("wmmat", C.c_int32 * 8), ("n_refinements", C.c_int32), ("reserved", C.c_int32),
                ("best_frame_error", C.c_int64)]


class GmResult(C.Structure):
    """SvtHipGmResult (include/svt_hip.h)."""
    _fields_ = [("wmmat", C.c_int32 * 8), ("wmtype", C.c_int32), ("probes", C.c_int32), ("best_error", C.c_int64), ("rounds", C.c_int32),
                ("invalid_probes", C.c_int32)]


class GmFitJob(C.Structure):
    """SvtHipGmFitJob (include/svt_hip.h)."""
    _fields_ = [("ref", C.c_int32), ("type", C.c_int32)]


class GmFit(C.Structure):
    """SvtHipGmFit (include/svt_hip.h)."""
    _fields_ = [("ret", C.c_int32), ("npoints", C.c_int32), ("num_inliers", C.c_int32), ("num_inliers_kept", C.c_int32), ("params", C.c_double * 8),
                ("wmmat", C.c_int32 * 8), ("wmtype", C.c_int32), ("reserved", C.c_int32)]


class GmModelRecord(C.Structure):
    """SvtHipGmModelRecord (include/svt_hip.h)."""
    _fields_ = [("num_inliers_kept", C.c_int32), ("fit_wmtype", C.c_int32), ("wmmat", C.c_int32 * 8), ("wmtype", C.c_int32), ("reserved", C.c_int32),
                ("best_error", C.c_int64)]


class GmEstimateOptions(C.Structure):
    """SvtHipGmEstimateOptions (include/svt_hip.h)."""
    _fields_ = [("rotzoom_model_only", C.c_int32), ("allow_high_precision_mv", C.c_int32), ("n_refinements", C.c_int32), ("max_points", C.c_int32)]


class GmEstimate(C.Structure):
    """SvtHipGmEstimate (include/svt_hip.h)."""
    _fields_ = [("wmmat", C.c_int32 * 8), ("wmtype", C.c_int32), ("num_correspondences", C.c_int32), ("n_models", C.c_int32), ("reserved", C.c_int32),
                ("ref_frame_error", C.c_int64), ("fits", GmFit * 2), ("models", GmModelRecord * 2)]


class PaletteJob(C.Structure):
    """SvtHipPaletteJob (include/svt_hip.h)."""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("bw", C.c_int32), ("bh", C.c_int32), ("cols", C.c_int32), ("rows", C.c_int32), ("n_cache", C.c_int32),
                ("dominant_step", C.c_int32), ("cache", C.c_uint16 * 16), ("map_off", C.c_int64)]


class PaletteResult(C.Structure):
    """SvtHipPaletteResult (include/svt_hip.h)."""
    _fields_ = [("colors", C.c_int32), ("n_cands", C.c_int32)]


class PaletteCand(C.Structure):
    """SvtHipPaletteCand (include/svt_hip.h)."""
    _fields_ = [("color_cost", C.c_int32), ("colors", C.c_uint16 * 8), ("raw", C.c_uint16 * 8), ("size", C.c_uint8), ("n", C.c_uint8), ("kind", C.c_uint8),
                ("reserved", C.c_uint8)]


PALETTE_MAX_CANDS = 14   # SVT_HIP_PALETTE_MAX_CANDS


def default_bd(pix_bytes, bd=None):
    """The bit depth of a call: `bd` when given, else 8 for one-byte samples and 10 for two-byte samples."""
    return bd if bd else (8 if pix_bytes == 1 else 10)


def _plane_args(plane):
    assert plane.ndim == 2 and plane.strides[1] == plane.itemsize and plane.strides[0] % plane.itemsize == 0
    return plane.itemsize, plane.ctypes.data_as(C.c_void_p), plane.strides[0] // plane.itemsize, plane.shape[1], plane.shape[0]


def palette_search_host(plane, jobs, results=None, cands=None, maps=None, bd=None):
    """svt_hip_palette_search_host: `plane` a 2-D uint8 / uint16 luma plane (may be an offset / strided view), `jobs` a ctypes array of PaletteJob.  `results`
    (PaletteResult * njobs), `cands` (PaletteCand * (14 njobs)) and `maps` (uint8 numpy array) are written in place when given, else made here, the maps zeroed
    and as long as the jobs' map_off need.  -> (results, cands, maps)."""
    n = len(jobs)
    pb, p, stride, _, _ = _plane_args(plane)
    results = results if results is not None else (PaletteResult * max(n, 1))()
    cands = cands if cands is not None else (PaletteCand * (PALETTE_MAX_CANDS * max(n, 1)))()
    if maps is None:
        maps = np.zeros(max([j.map_off + PALETTE_MAX_CANDS * j.bw * j.bh for j in jobs if 0 <= j.bw <= 64 and 0 <= j.bh <= 64 and j.map_off >= 0] + [4]), np.uint8)
    rc = lib().svt_hip_palette_search_host(pb, default_bd(pb, bd), p, stride, C.cast(jobs, C.c_void_p), n, C.cast(results, C.c_void_p), C.cast(cands, C.c_void_p),
                                           maps.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError(f"svt_hip_palette_search_host refused its arguments: status {rc}")
    return results, cands, maps


class IbcHashEntry(C.Structure):
    """SvtHipIbcHashEntry (include/svt_hip.h)."""
    _fields_ = [("x", C.c_int16), ("y", C.c_int16), ("hash_value2", C.c_uint32)]


class IbcSearchJob(C.Structure):
    """SvtHipIbcSearchJob (include/svt_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("x_pos", "y_pos", "block_size", "intra", "col_min", "col_max", "row_min", "row_max", "ref_mv_row", "ref_mv_col", "error_per_bit",
                                         "mi_row_start", "mi_row_end", "mi_col_start", "mi_col_end", "mib_size_log2")]


class IbcSearchResult(C.Structure):
    """SvtHipIbcSearchResult (include/svt_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("count", "n_matched", "n_valid", "found", "best_cost", "best_row", "best_col")]


class IbcFullSearchJob(C.Structure):
    """SvtHipIbcFullSearchJob (include/svt_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("x_pos", "y_pos", "block_w", "block_h", "intra", "col_min", "col_max", "row_min", "row_max", "ref_mv_row", "ref_mv_col", "mvp_row",
                                         "mvp_col", "step_param", "sad_per_bit", "error_per_bit", "exhaustive_allowed", "ibc_shift", "use_hash", "mi_row_start",
                                         "mi_row_end", "mi_col_start", "mi_col_end", "mib_size_log2")]


class IbcFullSearchResult(C.Structure):
    """SvtHipIbcFullSearchResult (include/svt_hip.h)."""
    _fields_ = ([(n, C.c_int32) for n in ("status", "dia_passes", "dia_refined", "dia_var", "dia_row", "dia_col", "mesh_ran", "mesh_passes", "mesh_var", "mesh_row",
                                          "mesh_col")] + [("hash", IbcSearchResult)] + [(n, C.c_int32) for n in ("source", "var", "best_row", "best_col", "dv_valid")])


IBC_HASH_BUCKETS = 1 << 19   # SVT_HIP_IBC_HASH_BUCKETS
IBC_MV_VALS = 32767          # SVT_HIP_IBC_MV_VALS
IBC_ENTRY_DTYPE = [("x", "<i2"), ("y", "<i2"), ("hash_value2", "<u4")]   # SvtHipIbcHashEntry as a numpy record


def ibc_hash_table_host(plane, capacity=None, bd=None):
    """svt_hip_ibc_hash_table_host: `plane` a 2-D uint8 / uint16 luma plane (may be a strided view).  capacity None: svt_hip_ibc_hash_max_entries.
    -> (bucket_start int32[2^19 + 1], entries record array [capacity], info int32[2])."""
    L = lib()
    pb, p, stride, w, h = _plane_args(plane)
    capacity = int(L.svt_hip_ibc_hash_max_entries(w, h)) if capacity is None else capacity
    start, entries, info = np.zeros(IBC_HASH_BUCKETS + 1, np.int32), np.zeros(max(capacity, 1), IBC_ENTRY_DTYPE), np.zeros(2, np.int32)
    nbytes = L.svt_hip_ibc_hash_scratch_bytes(w, h)
    scratch = np.zeros(max(nbytes, 1), np.uint8)
    rc = L.svt_hip_ibc_hash_table_host(pb, default_bd(pb, bd), p, stride, w, h, start.ctypes.data_as(C.c_void_p), entries.ctypes.data_as(C.c_void_p), capacity,
                                       info.ctypes.data_as(C.c_void_p), scratch.ctypes.data_as(C.c_void_p), nbytes)
    if rc != 0:
        raise RuntimeError(f"svt_hip_ibc_hash_table_host refused its arguments: status {rc}")
    return start, entries[:capacity], info


def ibc_cost_tables(joint_cost, comp_cost):
    j, c = np.ascontiguousarray(joint_cost, np.int32), np.ascontiguousarray(comp_cost, np.int32)
    assert j.shape == (4,) and c.shape == (2, IBC_MV_VALS)
    return j, c


def ibc_hash_search_host(plane, bucket_start, entries, joint_cost, comp_cost, jobs, bd=None):
    """svt_hip_ibc_hash_search_host: `jobs` a ctypes array of IbcSearchJob; the table as ibc_hash_table_host returns it.  -> IbcSearchResult * njobs."""
    pb, p, stride, w, h = _plane_args(plane)
    j, c = ibc_cost_tables(joint_cost, comp_cost)
    res = (IbcSearchResult * max(len(jobs), 1))()
    rc = lib().svt_hip_ibc_hash_search_host(pb, default_bd(pb, bd), p, stride, w, h, bucket_start.ctypes.data_as(C.c_void_p), entries.ctypes.data_as(C.c_void_p),
                                            j.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), C.cast(jobs, C.c_void_p), len(jobs), C.cast(res, C.c_void_p))
    if rc != 0:
        raise RuntimeError(f"svt_hip_ibc_hash_search_host refused its arguments: status {rc}")
    return res


def ibc_mesh_patterns(patterns):
    """[(range, interval), ...], at most four -> int32[8] as svt_hip_ibc_full_search_* take them; the patterns left out are (0, 0)"""
    p = np.zeros(8, np.int32)
    flat = np.asarray(patterns, np.int32).reshape(-1)
    assert flat.size <= 8 and flat.size % 2 == 0
    p[:flat.size] = flat
    return p


def ibc_full_search_host(plane, table, joint_cost, comp_cost, patterns, jobs, bd=None):
    """svt_hip_ibc_full_search_host: `jobs` a ctypes array of IbcFullSearchJob; `table` (bucket_start, entries) as ibc_hash_table_host returns them, or None;
    `patterns` [(range, interval), ...].  -> IbcFullSearchResult * njobs."""
    pb, p, stride, w, h = _plane_args(plane)
    j, c = ibc_cost_tables(joint_cost, comp_cost)
    pat = ibc_mesh_patterns(patterns)
    res = (IbcFullSearchResult * max(len(jobs), 1))()
    b, e = (table[0].ctypes.data_as(C.c_void_p), table[1].ctypes.data_as(C.c_void_p)) if table is not None else (None, None)
    rc = lib().svt_hip_ibc_full_search_host(pb, default_bd(pb, bd), p, stride, w, h, b, e, j.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                                            pat.ctypes.data_as(C.c_void_p), C.cast(jobs, C.c_void_p), len(jobs), C.cast(res, C.c_void_p))
    if rc != 0:
        raise RuntimeError(f"svt_hip_ibc_full_search_host refused its arguments: status {rc}")
    return res


def obmc_neighbours_host(above, left, mi_rows, mi_cols, mi_row, mi_col, bsize, job=None):
    """svt_hip_obmc_neighbours_host: `above` / `left` = (sb_type, overlappable) of the 4x4 units along the block's top / left edge, or None when there is no such
    neighbour.  Fills the segment lists of `job` (a fresh ObmcTargetJob when None) and returns it."""
    job = ObmcTargetJob(bsize=bsize) if job is None else job
    keep = [None if side is None else [np.ascontiguousarray(a, np.uint8) for a in side] for side in (above, left)]
    args = [None if a is None else a.ctypes.data_as(C.c_void_p) for side in keep for a in (side or (None, None))]
    rc = lib().svt_hip_obmc_neighbours_host(*args, mi_rows, mi_cols, mi_row, mi_col, bsize, C.byref(job))
    if rc != 0:
        raise RuntimeError(f"svt_hip_obmc_neighbours_host refused its arguments: status {rc}")
    return job


def obmc_target_host(plane, nbr, jobs, wm_samples):
    """svt_hip_obmc_target_host: `plane` the 2-D uint8 source luma plane, `nbr` the flat uint8 pool of neighbour predictions, `jobs` a ctypes array of
    ObmcTargetJob.  -> (wsrc, mask), int32[wm_samples] each, zero where no job writes."""
    _, p, stride, w, h = _plane_args(plane)
    nbr = np.ascontiguousarray(nbr, np.uint8)
    wsrc, mask = np.zeros(max(wm_samples, 1), np.int32), np.zeros(max(wm_samples, 1), np.int32)
    rc = lib().svt_hip_obmc_target_host(p, stride, w, h, nbr.ctypes.data_as(C.c_void_p), nbr.size, C.cast(jobs, C.c_void_p), len(jobs), wsrc.ctypes.data_as(C.c_void_p),
                                        mask.ctypes.data_as(C.c_void_p), wm_samples)
    if rc != 0:
        raise RuntimeError(f"svt_hip_obmc_target_host refused its arguments: status {rc}")
    return wsrc[:wm_samples], mask[:wm_samples]


def obmc_search_host(picture, pad_w, pad_h, mi_rows, mi_cols, wsrc, mask, joint_cost, comp_cost, jobs):
    """svt_hip_obmc_search_host: `picture` the 2-D uint8 view of the reference picture inside its padded plane (pad_w / pad_h samples of border around it), `wsrc` /
    `mask` int32 as obmc_target_host returns them, the cost tables as ibc_cost_tables takes them, `jobs` a ctypes array of ObmcSearchJob.  -> ObmcSearchResult * njobs."""
    _, p, stride, w, h = _plane_args(picture)
    j, c = ibc_cost_tables(joint_cost, comp_cost)
    wsrc, mask = np.ascontiguousarray(wsrc, np.int32), np.ascontiguousarray(mask, np.int32)
    assert wsrc.size == mask.size
    res = (ObmcSearchResult * max(len(jobs), 1))()
    rc = lib().svt_hip_obmc_search_host(p, stride, w, h, pad_w, pad_h, mi_rows, mi_cols, wsrc.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p), wsrc.size,
                                        j.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), C.cast(jobs, C.c_void_p), len(jobs), C.cast(res, C.c_void_p))
    if rc != 0:
        raise RuntimeError(f"svt_hip_obmc_search_host refused its arguments: status {rc}")
    return res


class CompSearchJob(C.Structure):
    """SvtHipCompSearchJob (include/svt_hip.h)."""
    _fields_ = [(n, C.c_uint32 if n == "full_lambda" else C.c_int32) for n in ("kind", "bsize", "x", "y", "pred0", "pred1", "quantizer", "full_lambda", "wedge_rate",
                                                                            "mode_rate")]


class CompSearchResult(C.Structure):
    """SvtHipCompSearchResult (include/svt_hip.h)."""
    _fields_ = ([(n, C.c_int32) for n in ("wedge_index", "wedge_sign", "mask_type", "interintra_mode", "interintra_wedge_index", "reserved")] +
                [("rd", C.c_int64), ("rd_wedge", C.c_int64)])


class CompSearchCand(C.Structure):
    """SvtHipCompSearchCand (include/svt_hip.h)."""
    _fields_ = [("sign", C.c_int32), ("rate", C.c_int32), ("sse", C.c_int64), ("dist", C.c_int64), ("rd", C.c_int64)]


COMP_SEARCH_MAX_CANDS = 20   # SVT_HIP_COMP_SEARCH_MAX_CANDS


def wedge_masks_host():
    """svt_hip_wedge_masks_host -> the contiguous wedge mask table, uint8[svt_hip_wedge_mask_table_bytes()]"""
    L = lib()
    out = np.zeros(L.svt_hip_wedge_mask_table_bytes(), np.uint8)
    rc = L.svt_hip_wedge_masks_host(out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError(f"svt_hip_wedge_masks_host failed: status {rc}")
    return out


def rd_curvfit_grids(grids):
    """(rate[4][65], dist[2][65], bsize_cat[22]) -> the three arrays as svt_hip_set_rd_curvfit_grids and svt_hip_compound_search_host take them"""
    rate, dist, cat = np.ascontiguousarray(grids[0], np.float64), np.ascontiguousarray(grids[1], np.float64), np.ascontiguousarray(grids[2], np.int32)
    assert rate.shape == (4, 65) and dist.shape == (2, 65) and cat.shape == (22,)
    return rate, dist, cat


def compound_search_host(grids, plane, pool, rates, jobs, bd=None, cands=True):
    """svt_hip_compound_search_host: `grids` (rate, dist, bsize_cat), `plane` the 2-D source luma plane (may be a strided view), `pool` the flat predictor pool of the
    same dtype, `rates` int32, `jobs` a ctypes array of CompSearchJob.  -> (CompSearchResult * njobs, CompSearchCand * (20 njobs) or None)."""
    pb, p, stride, w, h = _plane_args(plane)
    rate, dist, cat = rd_curvfit_grids(grids)
    pool, rates = np.ascontiguousarray(pool), np.ascontiguousarray(rates, np.int32)
    assert pool.dtype == plane.dtype
    n = len(jobs)
    res = (CompSearchResult * max(n, 1))()
    cand = (CompSearchCand * (COMP_SEARCH_MAX_CANDS * max(n, 1)))() if cands else None
    rc = lib().svt_hip_compound_search_host(rate.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p), cat.ctypes.data_as(C.c_void_p), pb, default_bd(pb, bd), p, stride,
                                            w, h, pool.ctypes.data_as(C.c_void_p), pool.size, rates.ctypes.data_as(C.c_void_p) if rates.size else None, rates.size,
                                            C.cast(jobs, C.c_void_p), n, C.cast(res, C.c_void_p), C.cast(cand, C.c_void_p) if cands else None)
    if rc != 0:
        raise RuntimeError(f"svt_hip_compound_search_host refused its arguments: status {rc}")
    return res, cand


class IfsJob(C.Structure):
    """SvtHipIfsJob (include/svt_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("bsize", "x", "y", "ref0_x", "ref0_y", "ref1_x", "ref1_y", "subpel0_x", "subpel0_y", "subpel1_x", "subpel1_y", "type", "fwd_offset",
                                         "bck_offset", "order", "dual", "quantizer")] + [("full_lambda", C.c_uint32), ("rate_tab", (C.c_int32 * 3) * 2), ("dst_x", C.c_int32),
                                                                                         ("dst_y", C.c_int32)]


class IfsResult(C.Structure):
    """SvtHipIfsResult (include/svt_hip.h)."""
    _fields_ = [("best", C.c_int32), ("interp_filters", C.c_uint32), ("switchable_rate", C.c_int32), ("regular_last", C.c_int32), ("rd", C.c_int64)]


class IfsCand(C.Structure):
    """SvtHipIfsCand (include/svt_hip.h)."""
    _fields_ = [("rate", C.c_int64), ("sse", C.c_int64), ("dist", C.c_int64), ("rd", C.c_int64)]


IFS_CANDS = 9   # SVT_HIP_IFS_CANDS


def ifs_search_host(src, ref0, ref1, jobs, dst=None, bd=None, cands=True):
    """svt_hip_ifs_search_host: `src` the 2-D source luma plane, `ref0` / `ref1` 2-D views whose sample (0, 0) is the reference picture's (the arrays behind them
    hold the border; ref1 may be None), `dst` None or the 2-D plane the winners' predictions are written into in place, all of one dtype; `jobs` a ctypes array of
    IfsJob.  -> (IfsResult * njobs, IfsCand * (9 njobs) or None)."""
    pb, p, stride, w, h = _plane_args(src)
    planes = [_plane_args(a) if a is not None else (pb, None, 0, 0, 0) for a in (ref0, ref1, dst)]
    assert all(a is None or a.dtype == src.dtype for a in (ref0, ref1, dst))
    n = len(jobs)
    res = (IfsResult * max(n, 1))()
    cand = (IfsCand * (IFS_CANDS * max(n, 1)))() if cands else None
    rc = lib().svt_hip_ifs_search_host(pb, default_bd(pb, bd), p, stride, w, h, planes[0][1], planes[0][2], planes[1][1], planes[1][2], planes[2][1], planes[2][2],
                                       C.cast(jobs, C.c_void_p), n, C.cast(res, C.c_void_p), C.cast(cand, C.c_void_p) if cands else None)
    if rc != 0:
        raise RuntimeError(f"svt_hip_ifs_search_host refused its arguments: status {rc}")
    return res, cand


class UpscalePlane(C.Structure):
    """SvtHipUpscalePlane (include/svt_hip.h)."""
    _fields_ = [("d_src", C.c_void_p), ("src_stride", C.c_int32), ("in_w", C.c_int32), ("d_dst", C.c_void_p), ("dst_stride", C.c_int32), ("out_w", C.c_int32),
                ("rows", C.c_int32)]


class ResizePlane(C.Structure):
    """SvtHipResizePlane (include/svt_hip.h)."""
    _fields_ = [("d_src", C.c_void_p), ("src_stride", C.c_int32), ("in_w", C.c_int32), ("in_h", C.c_int32), ("d_dst", C.c_void_p), ("dst_stride", C.c_int32),
                ("out_w", C.c_int32), ("out_h", C.c_int32)]


class ScaleFactors(C.Structure):
    """SvtHipScaleFactors (include/svt_hip.h)."""
    _fields_ = [("x_scale_fp", C.c_int32), ("y_scale_fp", C.c_int32), ("x_step_q4", C.c_int32), ("y_step_q4", C.c_int32)]


class ScaledBlk(C.Structure):
    """SvtHipScaledBlk (include/svt_hip.h)."""
    _fields_ = [("pos0_x", C.c_int32), ("pos0_y", C.c_int32), ("pos1_x", C.c_int32), ("pos1_y", C.c_int32), ("dst_x", C.c_int32), ("dst_y", C.c_int32),
                ("subpel0_x", C.c_uint16), ("subpel0_y", C.c_uint16), ("subpel1_x", C.c_uint16), ("subpel1_y", C.c_uint16),
                ("xs0", C.c_uint16), ("ys0", C.c_uint16), ("xs1", C.c_uint16), ("ys1", C.c_uint16), ("w", C.c_uint8), ("h", C.c_uint8),
                ("bank_x", C.c_uint8), ("bank_y", C.c_uint8), ("compound", C.c_uint8), ("fwd_offset", C.c_uint8), ("bck_offset", C.c_uint8),
                ("reserved", C.c_uint8)]


class ScaledRec(C.Structure):
    """SvtHipScaledRec (include/svt_hip.h)."""
    _fields_ = [("pre_x", C.c_int32), ("pre_y", C.c_int32), ("dst_x", C.c_int32), ("dst_y", C.c_int32), ("mv0_row", C.c_int16), ("mv0_col", C.c_int16),
                ("mv1_row", C.c_int16), ("mv1_col", C.c_int16), ("ss_x", C.c_uint8), ("ss_y", C.c_uint8), ("w", C.c_uint8), ("h", C.c_uint8),
                ("bank_x", C.c_uint8), ("bank_y", C.c_uint8), ("compound", C.c_uint8), ("fwd_offset", C.c_uint8), ("bck_offset", C.c_uint8),
                ("reserved", C.c_uint8 * 3)]


GM_MAX_REFS = 8    # SVT_HIP_GM_MAX_REFS
GM_FIT_MAX_JOBS = 64   # SVT_HIP_GM_FIT_MAX_JOBS
GM_MAX_CORNERS = 4096   # SVT_HIP_GM_MAX_CORNERS
TPL_MAX_REFS = 7   # MAX_PA_ME_MV: slots 0..3 list 0, 4..6 list 1
TPL_MAX_WINDOW = 60   # SVT_HIP_TPL_MAX_WINDOW (MAX_TPL_LA_SW)


def tpl_stats_grid(stats, is_720p_or_larger):
    """result_model_store's replication (EbRateControlProcess.c:148-161): the per-macroblock records `stats` ([mb_rows][mb_cols] structured array) spread over
    the picture's tpl_stats grid: one cell per 16x16 samples at 720p and above (the array as it is), one per 8x8 below (every record in a 2x2 square), i.e.
    [rows][aligned16_width >> shift] with shift = 3 + is_720p_or_larger."""
    rep = 1 if is_720p_or_larger else 2
    return np.repeat(np.repeat(stats, rep, axis=0), rep, axis=1)


def tpl_cell_log2(w, h):
    """The reference's is_720p_or_larger (EbPictureControlSet.c:1252): 16x16 cells when min(w, h) >= 720, else 8x8."""
    return 4 if min(w, h) >= 720 else 3


def tpl_ref_window(window_pocs, slot_pocs):
    """SvtHipTplWindowFrame.ref_window of one picture: `window_pocs` the picture_number of every window picture in window order, `slot_pocs` the POC of the
    picture's up to 7 reference slots (None = slot unused).  Entry rf_idx + 1 = the first window index with that POC (tpl_model_update's search,
    EbRateControlProcess.c:972-976), -1 when there is none; entry 0 serves rf_idx == -1, whose ref_frame_poc is the memset's 0 (:579)."""
    pocs = list(window_pocs)
    first = lambda poc: pocs.index(poc) if poc is not None and poc in pocs else -1
    slots = list(slot_pocs) + [None] * (TPL_MAX_REFS - len(slot_pocs))
    return [first(0)] + [first(p) for p in slots[:TPL_MAX_REFS]]


def tpl_synth_params(w, h, base_rdmult, r0_in=0.0, sb_size=64, cell_log2=None, rate=0):
    P = TplSynthParams()
    P.w, P.h, P.cell_log2, P.sb_size, P.base_rdmult, P.rate, P.r0_in = w, h, tpl_cell_log2(w, h) if cell_log2 is None else cell_log2, sb_size, base_rdmult, rate, r0_in
    return P


def tpl_window_frames(frames):
    """A ctypes array of TplWindowFrame from (stats pointer, grid pointer, on, ref_window) tuples; pointers are ints, c_void_p or None."""
    arr = (TplWindowFrame * len(frames))()
    for f, (d_stats, d_dep, on, ref_window) in zip(arr, frames):
        f.d_stats = getattr(d_stats, "value", d_stats)
        f.d_dep = getattr(d_dep, "value", d_dep)
        f.on = int(on)
        f.ref_window[:] = list(ref_window)
    return arr


def tpl_split_out(raw, params):
    """The bytes of d_out -> dict(r0, intra_cost_base, mc_dep_cost_base, factors [mb_rows][mb_cols], beta [sb_rows][sb_cols])."""
    mbw, mbh = (params.w + 15) // 16, (params.h + 15) // 16
    sbw, sbh = (params.w + params.sb_size - 1) // params.sb_size, (params.h + params.sb_size - 1) // params.sb_size
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    hd = TplR0BetaHeader.from_buffer_copy(raw[:C.sizeof(TplR0BetaHeader)].tobytes())
    body = raw[C.sizeof(TplR0BetaHeader):].view(np.float64)
    return dict(r0=hd.r0, intra_cost_base=hd.intra_cost_base, mc_dep_cost_base=hd.mc_dep_cost_base, factors=body[:mbw * mbh].reshape(mbh, mbw).copy(),
                beta=body[mbw * mbh:mbw * mbh + sbw * sbh].reshape(sbh, sbw).copy())


def tpl_window_host(params, stats, on, ref_windows):
    """svt_hip_tpl_window_host: `stats` one [mb_rows][mb_cols] structured array (TplMbStats fields) per window picture (None allowed for a picture that is
    off, except picture 0), `on` and `ref_windows` per picture.  Returns (the tpl_split_out dict, the grids as [n][rows][cols][2] int64)."""
    L = lib()
    s = 4 - params.cell_log2
    mbw, mbh = (params.w + 15) // 16, (params.h + 15) // 16
    n = len(stats)
    held = [None if a is None else np.ascontiguousarray(a, np.dtype(TplMbStats)) for a in stats]
    dep = np.full((n, mbh << s, mbw << s, 2), 0x5A5A5A5A5A5A5A5A, np.int64)
    out = np.zeros(max(L.svt_hip_tpl_r0beta_out_bytes(params.w, params.h, params.sb_size), 8) // 8, np.float64)
    frames = tpl_window_frames([(None if a is None else a.ctypes.data, dep[i].ctypes.data, on[i], ref_windows[i]) for i, a in enumerate(held)])
    rc = L.svt_hip_tpl_window_host(C.byref(params), frames, n, out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError(f"svt_hip_tpl_window_host refused its arguments: status {rc}")
    return tpl_split_out(out, params), dep


INTRA_EDGE_RECORD = 320   # samples of one edge record: 160 "above" + 160 "left", sample 0 at element 16 of each


def tx_desc(x, y, tx_type):
    return (x & 0x3FFF) | ((y & 0x3FFF) << 14) | (tx_type << 28)


vp, i32, sz, P = C.c_void_p, C.c_int, C.c_size_t, C.POINTER
P3, I3 = vp * 3, i32 * 3   # `void *const p[3]`, `const int v[3]`
_MEMCPY, _MEMCPY2D = [vp, vp, vp, sz], [vp, vp, sz, vp, sz, sz, sz]   # ctx, dst, src, bytes / ctx, dst, dst_pitch, src, src_pitch, width_bytes, rows
# the head the restoration plane calls share: ctx, pix_bytes, bd, d_dgd, stride, d_src or d_dst, its stride, pw, ph, unit_size, ss_y
_SGR = [vp, i32, i32, vp, i32, vp, i32, i32, i32, i32, i32]
# ... and the mode-decision tables: ctx, d_src, src_stride, pic_w, pic_h, sb_cols, n_sb, n_pus, pus, n_refs, refs, d_mv
_MD = [vp, vp, i32, i32, i32, i32, i32, i32, vp, i32, vp, vp]

# name -> (restype, argtypes) of every function include/svt_hip.h declares, in the header's order, and svt_hip_setup_rtcd of include/svt_hip_rtcd.h.
# tests/test_abi_binding.py compares each entry with the declaration (count, and pointer / integer width and sign / float per position).
PROTOTYPES = {
    # ---- context / memory
    "svt_hip_init": (i32, [i32, P(vp)]),
    "svt_hip_destroy": (None, [vp]),
    "svt_hip_last_error": (C.c_char_p, [vp]),
    "svt_hip_set_stream": (i32, [vp, vp]),
    "svt_hip_sync": (i32, [vp]),
    "svt_hip_malloc": (i32, [vp, P(vp), sz]),
    "svt_hip_free": (i32, [vp, vp]),
    "svt_hip_memcpy_h2d": (i32, _MEMCPY),
    "svt_hip_memcpy_d2h": (i32, _MEMCPY),
    "svt_hip_memcpy_d2d": (i32, _MEMCPY),
    "svt_hip_memcpy2d_h2d": (i32, _MEMCPY2D),
    "svt_hip_memcpy2d_d2h": (i32, _MEMCPY2D),
    "svt_hip_memcpy_h2d_async": (i32, _MEMCPY),
    "svt_hip_memcpy_d2h_async": (i32, _MEMCPY),
    "svt_hip_memcpy2d_h2d_async": (i32, _MEMCPY2D),
    "svt_hip_memcpy2d_d2h_async": (i32, _MEMCPY2D),
    "svt_hip_host_register": (i32, [vp, vp, sz]),
    "svt_hip_host_unregister": (i32, [vp, vp]),
    "svt_hip_host_alloc": (i32, [vp, P(vp), sz]),
    "svt_hip_host_free": (i32, [vp, vp]),
    "svt_hip_device_count": (i32, [P(i32)]),
    "svt_hip_warmup": (i32, [vp]),
    "svt_hip_timer_start": (i32, [vp]),
    "svt_hip_timer_stop_ms": (i32, [vp, P(C.c_float)]),
    # ---- open-loop ME
    "svt_hip_me_search_window": (SbSearch, [i32] * 8),
    "svt_hip_me_fullpel_frame_dev": (i32, [vp, vp, vp, i32, i32, i32, vp, i32, i32, vp, vp]),
    "svt_hip_me_fullpel_frame": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, vp, vp]),
    "svt_hip_me_set_big_windows": (i32, [vp, i32]),
    "svt_hip_me_get_big_windows": (i32, [vp, P(i32)]),
    "svt_hip_me_set_waves_per_sb": (i32, [vp, i32]),
    # ---- residual + transform + quantisation
    "svt_hip_fwd_txfm_quant_batch_dev": (i32, [vp, i32, i32, vp, i32, vp, i32, vp, i32, P(QuantParams), P(ScanTables), vp, vp, vp, vp, vp, vp]),
    "svt_hip_inv_txfm_add_batch_dev": (i32, [vp, i32, i32, i32, vp, vp, i32, vp, i32, vp, i32]),
    "svt_hip_iwht4x4_add_batch_dev": (i32, [vp, i32, i32, vp, vp, vp, i32, vp, i32, vp, i32]),
    "svt_hip_fwd_txfm_quant_multi_dev": (i32, [vp, i32, vp, i32]),
    "svt_hip_enc_txfm_multi_dev": (i32, [vp, i32, i32, P(EncTxJob), i32]),
    "svt_hip_inv_txfm_add_multi_dev": (i32, [vp, i32, i32, vp, i32]),
    # ---- deblocking loop filter
    "svt_hip_dlf_build_edges": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
    "svt_hip_dlf_filtered_units": (i32, [i32, i32, i32, i32]),
    "svt_hip_dlf_build_edges_crop": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
    "svt_hip_dlf_build_edges_picture_dev": (i32, [vp, vp, i32, i32, i32, i32, I3, I3, I3, I3, vp, P3, P3]),
    "svt_hip_deblock_plane_dev": (i32, [vp, vp, i32, i32, i32, vp, vp, i32, i32, i32]),
    "svt_hip_deblock_frame_dev": (i32, [vp, P3, i32, I3, i32, P3, P3, I3, I3, i32]),
    "svt_hip_deblock_frame_fused_dev": (i32, [vp, P3, P3, i32, I3, i32, I3, I3, P3, P3, I3, I3, i32]),
    "svt_hip_plane_sse_dev": (i32, [vp, i32, vp, i32, vp, i32, i32, i32, vp]),
    "svt_hip_dlf_search_level_dev": (i32, [vp, P(DlfSearch), vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, vp, i32, i32, vp, P(C.c_int), P(C.c_int64)]),
    "svt_hip_dlf_search_levels_picture_dev": (i32, [vp, i32, vp, i32, i32, vp, vp, vp]),
    # ---- CDEF
    "svt_hip_cdef_search_frame_dev": (i32, [vp, i32, P3, I3, P3, I3, i32, i32, vp, i32, i32, vp, vp, vp]),
    "svt_hip_cdef_apply_frame_dev": (i32, [vp, i32, P3, P3, I3, i32, i32, vp, vp, vp, i32, i32, vp, vp]),
    # ---- sub-pel prediction, block SAD / variance
    "svt_hip_subpel_predict_batch_dev": (i32, [vp, i32, i32, vp, i32, vp, i32, vp, i32]),
    "svt_hip_subpel_jobs_from_me_dev": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "svt_hip_block_sad_batch_dev": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, vp]),
    "svt_hip_block_variance_batch_dev": (i32, [vp, i32, i32, vp, i32, vp, i32, vp, i32, vp, vp]),
    "svt_hip_coeff_distortion_batch_dev": (i32, [vp, vp, vp, i32, i32, vp]),
    "svt_hip_block_sse_batch_dev": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, vp]),
    # ---- HME pyramids, variance pyramid, HME search
    "svt_hip_downsample_2d_dev": (i32, [vp, vp, i32, i32, i32, vp, i32, i32, i32]),
    "svt_hip_variance_pyramid_dev": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
    "svt_hip_sad_loop_batch_dev": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, vp]),
    "svt_hip_sad_loop16_batch_dev": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, vp]),
    # ---- self-guided restoration
    "svt_hip_sgr_filter_plane_dev": (i32, [vp, i32, i32, vp, i32, i32, i32, i32, vp, vp, i32]),
    "svt_hip_sgr_search_plane_dev": (i32, _SGR + [C.c_uint32, vp]),
    "svt_hip_sgr_apply_plane_dev": (i32, _SGR + [vp, i32, vp, vp]),
    "svt_hip_sgr_proj_error_plane_dev": (i32, _SGR + [C.c_uint32, i32, vp, vp]),
    "svt_hip_sgr_search_units_scratch_bytes": (sz, [i32, i32, i32]),
    "svt_hip_sgr_search_units_plane_dev": (i32, _SGR + [C.c_uint32, vp, vp, vp, vp, vp, sz]),
    "svt_hip_sgr_search_units_picture_dev": (i32, [vp, i32, i32, i32, P(SgrUnitsPlaneDev)]),
    "svt_hip_sgr_search_units_plane": (i32, _SGR + [C.c_uint32, vp, vp, vp, vp]),
    "svt_hip_sgr_search_units_picture": (i32, [vp, i32, i32, i32, P(SgrSearchPlane), vp]),
    "svt_hip_lr_apply_plane_dev": (i32, _SGR + [vp, i32, vp, vp, vp]),
    "svt_hip_lr_try_unit_dev": (i32, _SGR + [vp, i32, vp, vp, vp, vp, i32, i32, vp]),
    "svt_hip_lr_try_units_dev": (i32, _SGR + [vp, i32, vp, vp, vp, vp, i32, vp, i32, vp]),
    "svt_hip_wiener_walk_units_dev": (i32, [vp, i32, i32, vp, i32, i32, i32, i32, i32, vp, i32, vp, i32, vp, vp, i32, vp, vp]),
    "svt_hip_wiener_walk_units_picture_dev": (i32, [vp, i32, i32, i32, P(WienerWalkPlane)]),
    # ---- Wiener restoration search
    "svt_hip_wiener_stats_plane_dev": (i32, [vp, i32, i32, i32, vp, i32, vp, i32, i32, i32, i32, i32, vp, vp]),
    "svt_hip_wiener_init_units_dev": (i32, [vp, i32, i32, vp, vp, vp, vp, vp]),
    # ---- alt-ref temporal filtering
    "svt_hip_tf_filter_frame_dev": (i32, [vp, i32, i32, P3, I3, P3, I3, i32, i32, i32, i32, i32, P(TfRef), i32, P(C.c_double), i32, i32, vp]),
    "svt_hip_tf_estimate_noise_dev": (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "svt_hip_tf_noise_sigma": (C.c_double, [C.c_int64, C.c_int64]),
    "svt_hip_tf_subpel_frame_dev": (i32, [vp, i32, i32, P3, I3, P3, I3, P3, I3, i32, i32, C.c_uint64, i32, i32, vp, i32, vp]),
    # ---- compound inter prediction
    "svt_hip_compound_predict_batch_dev": (i32, [vp, i32, i32, vp, i32, vp, i32, vp, i32, vp, vp, i32]),
    "svt_hip_obmc_cost_batch_dev": (i32, [vp, vp, i32, vp, vp, vp, i32, vp]),
    "svt_hip_obmc_neighbours_host": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "svt_hip_obmc_target_batch_dev": (i32, [vp, vp, i32, i32, i32, vp, C.c_int64, vp, i32, vp, vp, C.c_int64]),
    "svt_hip_obmc_search_batch_dev": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, C.c_int64, vp, vp, vp, i32, vp]),
    "svt_hip_obmc_target_host": (i32, [vp, i32, i32, i32, vp, C.c_int64, vp, i32, vp, vp, C.c_int64]),
    "svt_hip_obmc_search_host": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, C.c_int64, vp, vp, vp, i32, vp]),
    "svt_hip_warp_predict_batch_dev": (i32, [vp, i32, i32, vp, i32, i32, i32, vp, i32, i32, i32, vp, i32]),
    "svt_hip_warp_compound_batch_dev": (i32, [vp, i32, i32, vp, i32, i32, i32, vp, i32, i32, i32, vp, vp, i32]),
    "svt_hip_blend_a64_batch_dev": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, i32]),
    # ---- picture formats around the high-bit-depth path
    "svt_hip_picture_format_dev": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, i32, i32]),
    "svt_hip_generate_padding_dev": (i32, [vp, vp, i32, i32, i32, i32, i32, i32]),
    # ---- super-resolution: normative upscale and the scaler
    "svt_hip_superres_scaled_dim": (i32, [i32, i32]),
    "svt_hip_superres_upscale_params": (i32, [i32, i32, P(C.c_int32), P(C.c_int32)]),
    "svt_hip_superres_upscale_planes_dev": (i32, [vp, i32, i32, P(UpscalePlane), i32]),
    "svt_hip_resize_scratch_bytes": (sz, [i32, P(ResizePlane), i32]),
    "svt_hip_resize_planes_dev": (i32, [vp, i32, i32, P(ResizePlane), i32, vp, sz]),
    # ---- inter prediction from a reference of another size
    "svt_hip_scale_factors": (i32, [i32, i32, i32, i32, P(ScaleFactors)]),
    "svt_hip_scaled_block_params": (None, [P(ScaleFactors), i32, i32, i32, i32, i32, i32, i32, i32] + [P(C.c_int32)] * 6),
    "svt_hip_scaled_jobs_dev": (i32, [vp, P(ScaleFactors), P(ScaleFactors), P(i32), P(i32), vp, vp, i32]),
    "svt_hip_scaled_predict_batch_dev": (i32, [vp, i32, i32, vp, i32, vp, i32, vp, i32, vp, i32]),
    # ---- per-call forms
    "svt_hip_quantize_batch_dev": (i32, [vp, vp, i32, i32, P(QuantParams), vp, vp, vp, vp]),
    "svt_hip_residual_dev": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, i32, i32]),
    "svt_hip_ext_all_sad_8x8_16x16_batch_dev": (i32, [vp, vp, i32, vp, i32, vp, i32, vp]),
    "svt_hip_ext_eight_sad_32x32_64x64_batch_dev": (i32, [vp, vp, i32, vp]),
    "svt_hip_interm_var_four8x8_batch_dev": (i32, [vp, vp, i32, vp, i32, vp, vp]),
    "svt_hip_handle_transform64_batch_dev": (i32, [vp, i32, vp, i32, vp]),
    "svt_hip_handle_transform64_n2n4_batch_dev": (i32, [vp, i32, vp, i32]),
    "svt_hip_upsampled_pred_batch_dev": (i32, [vp, vp, i32, vp, vp, i32]),
    "svt_hip_jnt_convolve_dev": (i32, [vp, i32, i32, i32, vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32]),
    "svt_hip_diffwtd_mask_dev": (i32, [vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32]),
    "svt_hip_blend_a64_d16_dev": (i32, [vp, i32, i32, vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32]),
    "svt_hip_block_mean_batch_dev": (i32, [vp, vp, i32, vp, i32, i32, i32, i32, vp]),
    "svt_hip_ext_sad_16x16_batch_dev": (i32, [vp, vp, i32, vp, i32, vp, i32, vp]),
    "svt_hip_ext_sad_32x32_64x64_batch_dev": (i32, [vp, vp, vp, i32]),
    "svt_hip_cdef_dist_dev": (i32, [vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, i32, vp]),
    "svt_hip_cdef_search_one_dual_dev": (i32, [vp, vp, vp, i32, vp, vp, i32, i32, i32, vp]),
    "svt_hip_cdef_joint_strength_search_dev": (i32, [vp, vp, vp, i32, vp, vp, i32, i32, i32, vp]),
    "svt_hip_set_cdef_select_form": (i32, [vp, i32]),
    "svt_hip_cdef_strength_select_dev": (i32, [vp, vp, vp, i32, i32, i32, vp, sz]),
    "svt_hip_cdef_strength_select_multi_dev": (i32, [vp, i32, P(vp), P(vp), i32, i32, i32, P(vp), sz]),
    "svt_hip_cdef_finish_dev": (i32, [vp, vp, vp, i32, vp, C.c_uint64, vp, vp, vp, vp, vp]),
    "svt_hip_sgr_flt_proj_dev": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
    "svt_hip_convolve8_dev": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32]),
    "svt_hip_wiener_convolve_add_src_dev": (i32, [vp, i32, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32]),
    "svt_hip_cdef_find_dir_batch_dev": (i32, [vp, vp, i32, vp, i32, i32, vp, vp]),
    "svt_hip_cdef_filter_block_batch_dev": (i32, [vp, vp, i32, vp, i32, vp, vp, i32]),
    "svt_hip_lpf_edges_batch_dev": (i32, [vp, i32, i32, vp, i32, vp, i32]),
    # ---- mode decision: picture-level precompute
    "svt_hip_md_fullpel_sad_picture_dev": (i32, _MD + [vp]),
    "svt_hip_md_fullpel_avg_sad_picture_dev": (i32, _MD + [i32, vp, vp]),
    "svt_hip_md_fullpel_sad_picture_hbd_dev": (i32, _MD + [vp]),
    "svt_hip_md_fullpel_avg_sad_picture_hbd_dev": (i32, _MD + [i32, vp, vp]),
    "svt_hip_md_subpel_grid_picture_dev": (i32, _MD + [i32, vp]),
    "svt_hip_md_halfpel_grid_picture_dev": (i32, _MD + [i32, vp]),
    # ---- intra prediction
    "svt_hip_intra_predict_batch_dev": (i32, [vp, i32, i32, vp, vp, i32, vp, i32]),
    "svt_hip_cfl_predict_batch_dev": (i32, [vp, i32, i32, vp, i32, vp, vp, i32, vp, vp, i32, vp]),
    "svt_hip_filter_intra_predict_batch_dev": (i32, [vp, i32, i32, vp, vp, i32, vp, i32]),
    "svt_hip_intra_ois_picture_dev": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
    # ---- palette luma search, screen-content detection
    "svt_hip_palette_search_batch_dev": (i32, [vp, i32, i32, vp, i32, vp, i32, vp, vp, vp]),
    "svt_hip_palette_search_host": (i32, [i32, i32, vp, i32, vp, i32, vp, vp, vp]),
    "svt_hip_screen_content_detect_dev": (i32, [vp, i32, i32, vp, i32, i32, i32, vp]),
    # ---- intra block copy: hash planes, hash table, hash search
    "svt_hip_ibc_hash_scratch_bytes": (sz, [i32, i32]),
    "svt_hip_ibc_hash_max_entries": (sz, [i32, i32]),
    "svt_hip_ibc_block_hashes_dev": (i32, [vp, i32, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, sz]),
    "svt_hip_ibc_hash_table_dev": (i32, [vp, i32, i32, vp, i32, i32, i32, vp, vp, C.c_int64, vp, vp, sz]),
    "svt_hip_ibc_hash_search_batch_dev": (i32, [vp, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]),
    "svt_hip_ibc_hash_table_host": (i32, [i32, i32, vp, i32, i32, i32, vp, vp, C.c_int64, vp, vp, sz]),
    "svt_hip_ibc_hash_search_host": (i32, [i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]),
    # ---- intra block copy: diamond, mesh and the final choice
    "svt_hip_wedge_mask_table_bytes": (sz, []),
    "svt_hip_wedge_mask_offset": (i32, [i32, i32, i32]),
    "svt_hip_wedge_masks_host": (i32, [vp]),
    "svt_hip_wedge_masks_dev": (i32, [vp, vp]),
    "svt_hip_set_rd_curvfit_grids": (i32, [vp, vp, vp, vp]),
    "svt_hip_compound_search_batch_dev": (i32, [vp, i32, i32, vp, i32, i32, i32, vp, C.c_int64, vp, i32, vp, i32, vp, vp]),
    "svt_hip_compound_search_host": (i32, [vp, vp, vp, i32, i32, vp, i32, i32, i32, vp, C.c_int64, vp, i32, vp, i32, vp, vp]),
    # ---- the dual interpolation filter search
    "svt_hip_ifs_search_batch_dev": (i32, [vp, i32, i32, vp, i32, i32, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp]),
    "svt_hip_ifs_search_host": (i32, [i32, i32, vp, i32, i32, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp]),
    "svt_hip_ibc_full_search_scratch_bytes": (sz, [i32]),
    "svt_hip_ibc_full_search_batch_dev": (i32, [vp, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, sz]),
    "svt_hip_ibc_full_search_host": (i32, [i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp]),
    # ---- TPL flow dispenser
    "svt_hip_tpl_dispenser_scratch_bytes": (sz, [i32, i32]),
    "svt_hip_tpl_dispenser_picture_dev": (i32, [vp, P(TplParams), vp, i32, P(TplRef), vp, vp, vp, vp, vp, i32, vp, vp]),
    "svt_hip_tpl_set_phases": (i32, [vp, i32]),
    # ---- TPL flow synthesizer, r0 / beta / lambda factors
    "svt_hip_tpl_dep_bytes": (sz, [i32, i32, i32]),
    "svt_hip_tpl_r0beta_out_bytes": (sz, [i32, i32, i32]),
    "svt_hip_tpl_r0beta_scratch_bytes": (sz, []),
    "svt_hip_tpl_synth_picture_dev": (i32, [vp, P(TplSynthParams), P(TplWindowFrame), i32, i32]),
    "svt_hip_tpl_r0beta_dev": (i32, [vp, P(TplSynthParams), vp, vp, vp, vp]),
    "svt_hip_tpl_window_dev": (i32, [vp, P(TplSynthParams), P(TplWindowFrame), i32, vp, vp]),
    "svt_hip_tpl_window_host": (i32, [P(TplSynthParams), P(TplWindowFrame), i32, vp]),
    # ---- global motion
    "svt_hip_gm_shear_params_batch_dev": (i32, [vp, vp, i32, vp]),
    "svt_hip_gm_warp_error_batch_dev": (i32, [vp, vp, i32, i32, i32, vp, i32, i32, i32, vp, i32, vp]),
    "svt_hip_gm_frame_error_batch_dev": (i32, [vp, vp, i32, i32, i32, P(GmRef), i32, vp]),
    "svt_hip_gm_refine_scratch_bytes": (sz, [i32]),
    "svt_hip_gm_refine_picture_dev": (i32, [vp, vp, i32, i32, i32, P(GmRef), i32, vp, i32, vp, vp, P(i32)]),
    "svt_hip_gm_error_table": (i32, [vp]),
    "svt_hip_gm_corners_scratch_bytes": (sz, [P(GmRef), i32]),
    "svt_hip_gm_corners_batch_dev": (i32, [vp, P(GmRef), i32, i32, vp, vp, vp, vp]),
    "svt_hip_gm_cross_correlation_batch_dev": (i32, [vp, vp, i32, vp, i32, i32, i32, vp, i32, vp]),
    "svt_hip_gm_correspondences_batch_dev": (i32, [vp, vp, i32, i32, i32, vp, vp, P(GmRef), i32, vp, vp, i32, vp, vp]),
    "svt_hip_gm_fit_scratch_bytes": (sz, [i32, i32]),
    "svt_hip_gm_fit_batch_dev": (i32, [vp, vp, vp, i32, i32, P(GmFitJob), i32, i32, i32, vp, vp, vp, vp]),
    "svt_hip_gm_params_cost_host": (i32, [P(C.c_int32), i32, i32]),
    "svt_hip_gm_decide_host": (i32, [P(GmModelRecord), C.c_int64, i32, i32, P(C.c_int32), P(C.c_int32)]),
    "svt_hip_gm_estimate_scratch_bytes": (sz, [i32, i32, i32, P(GmEstimateOptions)]),
    "svt_hip_gm_estimate_picture_dev": (i32, [vp, vp, i32, i32, i32, P(GmRef), i32, P(GmEstimateOptions), P(GmEstimate), vp]),
    # ---- include/svt_hip_rtcd.h
    "svt_hip_setup_rtcd": (i32, [vp, vp]),
}


def bind(L):
    """Attach PROTOTYPES to every function of them that the loaded library `L` exports (a test double may export only part of the ABI) -> L."""
    for name, (restype, argtypes) in PROTOTYPES.items():
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    return L


_lib = None


def lib():
    """Load libsvtav1_hip.so (once) and attach the prototypes. Raises if the library was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _lib = bind(C.CDLL(LIB_PATH))
    return _lib


Plane = collections.namedtuple("Plane", "d_root ptr stride root view")
Plane.__doc__ = """An uploaded 2-D plane: device pointer of the whole array, device pointer of the view's sample (0, 0), row stride in samples, the array, the view."""


class Scope:
    """The device memory of one call, `with ctx.scope() as s:`.  Whatever is allocated through `s` is freed when the block ends, normally or by an exception.
    Memory the caller owns is passed around as a pointer and never registered here; neither is a pointer derived by offset from a registered one."""

    def __init__(self, ctx):
        self.ctx, self.owned = ctx, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        owned, self.owned = self.owned, []
        self.ctx.free(*owned)

    def empty(self, nbytes):
        self.owned.append(self.ctx.empty(nbytes))
        return self.owned[-1]

    def upload(self, arr):
        """A numpy array (made contiguous) -> device pointer; max(nbytes, 4) are allocated and nothing is copied when nbytes == 0."""
        arr = np.ascontiguousarray(arr)
        return self.ctx._h2d(self.empty(arr.nbytes), arr.ctypes.data_as(C.c_void_p), arr.nbytes)

    def filled(self, shape, value, dtype):
        return self.upload(np.full(shape, value, dtype))

    def structs(self, arr):
        """A ctypes array -> device pointer, sized and copied as in upload."""
        return self.ctx._h2d(self.empty(C.sizeof(arr)), C.cast(arr, C.c_void_p), C.sizeof(arr))

    def plane(self, view):
        """A 2-D plane that may be an offset / strided view (unit stride along a row) of a C-contiguous array: that array is uploaded whole.  -> Plane"""
        root = view
        while isinstance(root.base, np.ndarray):
            root = root.base
        assert view.ndim == 2 and root.flags.c_contiguous and view.strides[1] == view.itemsize and view.strides[0] % view.itemsize == 0
        d = self.upload(root)
        return Plane(d, C.c_void_p(d.value + view.ctypes.data - root.ctypes.data), view.strides[0] // view.itemsize, root, view)

    def download(self, dptr, shape, dtype):
        return self.ctx.to_host(dptr, shape, dtype)

    def structs_back(self, dptr, kind):
        """A fresh ctypes array of type `kind` as the device holds it at dptr (a zero-size one is not copied)."""
        out = kind()
        if C.sizeof(out):
            self.ctx.call("memcpy_d2h", C.cast(out, C.c_void_p), dptr, C.sizeof(out), what="d2h")
        return out

    def plane_back(self, rec):
        """The view of `rec` as the device now holds it (a view of a fresh copy of the whole array: what lies around the view comes along)."""
        host = self.download(rec.d_root, rec.root.shape, rec.root.dtype)
        return np.ndarray(rec.view.shape, rec.view.dtype, host, rec.view.ctypes.data - rec.root.ctypes.data, rec.view.strides)


class Context:
    """RAII wrapper of SvtHipCtx."""

    def __init__(self, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        rc = self.L.svt_hip_init(device, C.byref(self.h))
        if rc != 0:
            raise RuntimeError(f"svt_hip_init failed with status {rc} (no gfx950 device?) — there is no CPU fallback")

    def check(self, rc, what=""):
        if rc != 0:
            raise RuntimeError(f"{what} failed: status {rc}: {self.L.svt_hip_last_error(self.h).decode()}")

    def call(self, name, *args, what=None):
        """svt_hip_<name>(ctx, *args), checked; a failure is reported as `what`, by default the name without its _dev suffix."""
        self.check(getattr(self.L, "svt_hip_" + name)(self.h, *args), what or name.removesuffix("_dev"))

    def sync(self):
        self.call("sync")

    def scope(self):
        return Scope(self)

    def timed(self, fn, window_ms, warm=2, reps=2, growth=1.2):
        """HIP-event time of back-to-back fn() calls: `warm` calls and a synchronisation, then windows of `reps` calls, `reps` growing until a window lasts
        window_ms; only that last window counts.  -> (ms per call, ms of the window, its reps)"""
        for _ in range(warm):
            fn()
        self.sync()
        ms = C.c_float()
        while True:
            self.L.svt_hip_timer_start(self.h)
            for _ in range(reps):
                fn()
            self.call("timer_stop_ms", C.byref(ms), what="timer")
            if ms.value >= window_ms:
                return ms.value / reps, ms.value, reps
            reps = int(reps * max(2.0, growth * window_ms / max(ms.value, 1e-3)))

    # ---- device memory through the C ABI (tests / tools; bench.py uses torch tensors instead)
    def _h2d(self, dptr, src, nbytes):
        if nbytes:
            self.call("memcpy_h2d", dptr, src, nbytes, what="h2d")
        return dptr

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return self._h2d(self.empty(arr.nbytes), arr.ctypes.data_as(C.c_void_p), arr.nbytes)

    def empty(self, nbytes):
        p = C.c_void_p()
        self.call("malloc", C.byref(p), max(nbytes, 4))
        return p

    def to_host(self, dptr, shape, dtype):
        out = np.empty(shape, dtype)
        if out.nbytes:
            self.call("memcpy_d2h", out.ctypes.data_as(C.c_void_p), dptr, out.nbytes, what="d2h")
        return out

    def free(self, *ptrs):
        for p in ptrs:
            self.L.svt_hip_free(self.h, p)

    # ---- intra prediction
    def intra_ois_picture(self, d_src, stride, w, h, mode_end=12):
        """svt_hip_intra_ois_picture_dev on a resident 8-bit luma plane -> (mode [mb_rows][mb_cols] uint8, cost [mb_rows][mb_cols] int32) on the host."""
        mbw, mbh = (w + 15) // 16, (h + 15) // 16
        with self.scope() as s:
            d_mode, d_cost = s.empty(mbw * mbh), s.empty(mbw * mbh * 4)
            self.call("intra_ois_picture_dev", d_src, stride, w, h, mode_end, d_mode, d_cost)
            self.sync()
            return s.download(d_mode, (mbh, mbw), np.uint8), s.download(d_cost, (mbh, mbw), np.int32)

    def intra_predict_batch(self, edges, jobs, dst, bd=None):
        """svt_hip_intra_predict_batch_dev: `edges` a uint8 / uint16 array of edge records, `jobs` a ctypes array of IntraJob, `dst` the 2-D destination plane
        (same dtype) the blocks are written into; `bd` defaults to the dtype's usual depth (8 for uint8, 10 for uint16; uint16 planes may also hold 8-bit samples: bd=8).
        Returns the plane after the launch."""
        pix_bytes = edges.dtype.itemsize
        assert dst.dtype == edges.dtype and dst.ndim == 2
        with self.scope() as s:
            d_e, d_j, d_d = s.upload(edges), s.structs(jobs), s.upload(dst)
            self.call("intra_predict_batch_dev", pix_bytes, default_bd(pix_bytes, bd), d_e, d_j, len(jobs), d_d, dst.shape[1])
            self.sync()
            return s.download(d_d, dst.shape, dst.dtype)

    def cfl_predict_batch(self, luma, edges, jobs, cb, cr, want_ac=False, bd=None):
        """svt_hip_cfl_predict_batch_dev: `luma` the 2-D luma plane, `edges` a flat array of edge records, `jobs` a ctypes array of CflJob, `cb` / `cr` the 2-D chroma
        planes (one of them may be None), all uint8 (bd 8) or all uint16 (bd 10 unless `bd` says 8); planes may be offset / strided views, the two chroma planes with one row stride.
        Returns (cb, cr) after the launch -- views like the ones given, None for a plane not given -- and with `want_ac` also the [njobs][32][32] int16 AC
        buffer; `want_ac` may be that buffer's initial content instead of True."""
        pix_bytes = luma.dtype.itemsize
        planes = [p for p in (cb, cr) if p is not None]
        assert planes and all(p.dtype == luma.dtype for p in planes) and edges.dtype == luma.dtype
        with self.scope() as s:
            y, d_e, d_j = s.plane(luma), s.upload(edges), s.structs(jobs)
            up = [s.plane(p) if p is not None else None for p in (cb, cr)]
            strides = {u.stride for u in up if u}
            assert len(strides) == 1, "the two chroma planes share one stride"
            d_ac = None
            if want_ac is not False:
                ac0 = np.zeros((len(jobs), 32, 32), np.int16) if want_ac is True else np.ascontiguousarray(want_ac, np.int16)
                assert ac0.shape == (len(jobs), 32, 32)
                d_ac = s.upload(ac0)
            self.call("cfl_predict_batch_dev", pix_bytes, default_bd(pix_bytes, bd), y.ptr, y.stride, d_e, d_j, len(jobs), up[0] and up[0].ptr, up[1] and up[1].ptr,
                      strides.pop(), d_ac)
            self.sync()
            out = tuple(s.plane_back(u) if u else None for u in up)
            if d_ac is not None:
                out += (s.download(d_ac, ac0.shape, np.int16),)
            return out

    def palette_search_batch(self, plane, jobs, results, cands, maps, bd=None):
        """svt_hip_palette_search_batch_dev: `plane` a 2-D uint8 / uint16 luma plane (may be an offset / strided view; bd 8 for uint8, 10 for uint16 unless `bd` says
        8), `jobs` a ctypes array of PaletteJob.  `results` (PaletteResult * njobs), `cands` (PaletteCand * (14 njobs)) and `maps` (uint8 numpy array) are the
        initial content of the three outputs.  -> (results, cands, maps) as the device left them, fresh objects of the same types."""
        with self.scope() as s:
            p, d_j, d_r, d_c, d_m = s.plane(plane), s.structs(jobs), s.structs(results), s.structs(cands), s.upload(maps)
            self.call("palette_search_batch_dev", plane.itemsize, default_bd(plane.itemsize, bd), p.ptr, p.stride, d_j, len(jobs), d_r, d_c, d_m)
            self.sync()
            return s.structs_back(d_r, type(results)), s.structs_back(d_c, type(cands)), s.download(d_m, maps.shape, np.uint8)

    def screen_content_detect(self, plane, bd=None, out=None):
        """svt_hip_screen_content_detect_dev: `plane` a 2-D uint8 (bd 8) or uint16 (bd 10) luma plane, may be an offset / strided view.  `out`, if given, is an int32
        array of at least four words, the initial content of the output buffer.  -> that buffer after the call: counts_1, counts_2, color_detection,
        sc_content_detected, then whatever followed."""
        out = np.zeros(4, np.int32) if out is None else np.ascontiguousarray(out, np.int32)
        with self.scope() as s:
            p, d_o = s.plane(plane), s.upload(out)
            self.call("screen_content_detect_dev", plane.itemsize, default_bd(plane.itemsize, bd), p.ptr, p.stride, plane.shape[1], plane.shape[0], d_o)
            self.sync()
            return s.download(d_o, out.shape, np.int32)

    def ibc_block_hashes(self, plane, block_size, bd=None, fill=0):
        """svt_hip_ibc_block_hashes_dev: `plane` a 2-D uint8 / uint16 luma plane (may be a strided view).  The outputs start filled with the byte `fill`.
        -> (hash1, hash2 uint32[h, w], same int8[3, h, w]); only x < w - block_size + 1, y < h - block_size + 1 is specified."""
        h, w = plane.shape
        with self.scope() as s:
            p = s.plane(plane)
            nbytes = self.L.svt_hip_ibc_hash_scratch_bytes(w, h)
            d_s = s.empty(max(nbytes, 256))
            d_1, d_2, d_m = s.filled(w * h * 4, fill, np.uint8), s.filled(w * h * 4, fill, np.uint8), s.filled(3 * w * h, fill, np.uint8)
            self.call("ibc_block_hashes_dev", plane.itemsize, default_bd(plane.itemsize, bd), p.ptr, p.stride, w, h, block_size, d_1, d_2, d_m, d_s, nbytes)
            self.sync()
            return s.download(d_1, (h, w), np.uint32), s.download(d_2, (h, w), np.uint32), s.download(d_m, (3, h, w), np.int8)

    def ibc_hash_table(self, plane, capacity=None, bd=None, guard=0, fill=0xC3):
        """svt_hip_ibc_hash_table_dev: `plane` a 2-D uint8 / uint16 luma plane.  capacity None: svt_hip_ibc_hash_max_entries.  `guard` bytes of `fill` lie before
        and behind d_bucket_start and d_entries, which start filled with it too.  -> (bucket_start int32[2^19 + 1], entries record array [capacity], info
        int32[2], the four guard areas as uint8 arrays)."""
        h, w = plane.shape
        capacity = int(self.L.svt_hip_ibc_hash_max_entries(w, h)) if capacity is None else capacity
        assert guard % 8 == 0
        nb_s, nb_e = (IBC_HASH_BUCKETS + 1) * 4, capacity * 8
        with self.scope() as s:
            p = s.plane(plane)
            nbytes = self.L.svt_hip_ibc_hash_scratch_bytes(w, h)
            d_s = s.empty(max(nbytes, 256))
            d_b, d_e = s.filled(nb_s + 2 * guard, fill, np.uint8), s.filled(nb_e + 2 * guard + 8, fill, np.uint8)
            d_i = s.filled(2, -1, np.int32)
            self.call("ibc_hash_table_dev", plane.itemsize, default_bd(plane.itemsize, bd), p.ptr, p.stride, w, h, d_b.value + guard, d_e.value + guard, capacity, d_i,
                      d_s, nbytes)
            self.sync()
            b, e = s.download(d_b, (nb_s + 2 * guard,), np.uint8), s.download(d_e, (nb_e + 2 * guard + 8,), np.uint8)
            guards = (b[:guard], b[guard + nb_s:], e[:guard], e[guard + nb_e:])
            return b[guard:guard + nb_s].view(np.int32).copy(), e[guard:guard + nb_e].view(IBC_ENTRY_DTYPE).copy(), s.download(d_i, (2,), np.int32), guards

    def ibc_hash_search_batch(self, plane, bucket_start, entries, joint_cost, comp_cost, jobs, bd=None, fill=0xC3):
        """svt_hip_ibc_hash_search_batch_dev: the table as ibc_hash_table returns it, `jobs` a ctypes array of IbcSearchJob.  -> IbcSearchResult * njobs as the
        device left them (started as the byte `fill`)."""
        h, w = plane.shape
        j, c = ibc_cost_tables(joint_cost, comp_cost)
        res = (IbcSearchResult * max(len(jobs), 1))()
        C.memset(res, fill, C.sizeof(res))
        with self.scope() as s:
            p = s.plane(plane)
            d_b, d_e = s.upload(np.ascontiguousarray(bucket_start, np.int32)), s.upload(np.frombuffer(entries.tobytes() + bytes(8), np.uint8))
            d_jc, d_cc = s.upload(j), s.upload(c)
            d_j, d_r = s.structs(jobs if len(jobs) else (IbcSearchJob * 1)()), s.structs(res)
            self.call("ibc_hash_search_batch_dev", plane.itemsize, default_bd(plane.itemsize, bd), p.ptr, p.stride, w, h, d_b, d_e, d_jc, d_cc, d_j, len(jobs), d_r)
            self.sync()
            return s.structs_back(d_r, type(res))

    def ibc_full_search_batch(self, plane, table, joint_cost, comp_cost, patterns, jobs, bd=None, guard=0, fill=0xC3):
        """svt_hip_ibc_full_search_batch_dev: `table` (bucket_start, entries) as ibc_hash_table returns them, or None; `patterns` [(range, interval), ...]; `jobs` a
        ctypes array of IbcFullSearchJob.  The results start as the byte `fill`; `guard` bytes (a multiple of 256) of it lie before and behind the results and the
        scratch.  -> (IbcFullSearchResult * njobs, the four guard areas as uint8 arrays)."""
        h, w = plane.shape
        j, c = ibc_cost_tables(joint_cost, comp_cost)
        pat = ibc_mesh_patterns(patterns)
        n = len(jobs)
        kind = IbcFullSearchResult * max(n, 1)
        nb_r, nb_s = C.sizeof(kind), self.L.svt_hip_ibc_full_search_scratch_bytes(n)
        assert guard % 256 == 0
        with self.scope() as s:
            p = s.plane(plane)
            d_b, d_e = (None, None) if table is None else (s.upload(np.ascontiguousarray(table[0], np.int32)), s.upload(np.frombuffer(table[1].tobytes() + bytes(8), np.uint8)))
            d_jc, d_cc = s.upload(j), s.upload(c)
            d_j = s.structs(jobs if n else (IbcFullSearchJob * 1)())
            d_r, d_s = s.filled(nb_r + 2 * guard, fill, np.uint8), s.filled(max(nb_s, 256) + 2 * guard, fill, np.uint8)
            self.call("ibc_full_search_batch_dev", plane.itemsize, default_bd(plane.itemsize, bd), p.ptr, p.stride, w, h, d_b, d_e, d_jc, d_cc,
                      pat.ctypes.data_as(C.c_void_p), d_j, n, d_r.value + guard, d_s.value + guard, nb_s)
            self.sync()
            r, sc = s.download(d_r, (nb_r + 2 * guard,), np.uint8), s.download(d_s, (max(nb_s, 256) + 2 * guard,), np.uint8)
            res = kind.from_buffer_copy(r[guard:guard + nb_r].tobytes())
            return res, (r[:guard], r[guard + nb_r:], sc[:guard], sc[guard + nb_s:])

    # ---- masked compound and inter-intra: choosing the mask
    def wedge_masks(self):
        """svt_hip_wedge_masks_dev -> the device pointer of the context's wedge mask table (owned by the context: not to be freed)"""
        p = C.c_void_p()
        self.call("wedge_masks_dev", C.byref(p))
        return p

    def set_rd_curvfit_grids(self, grids):
        """svt_hip_set_rd_curvfit_grids: `grids` (rate[4][65], dist[2][65], bsize_cat[22])"""
        rate, dist, cat = rd_curvfit_grids(grids)
        self.call("set_rd_curvfit_grids", rate.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p), cat.ctypes.data_as(C.c_void_p))

    def compound_search_batch(self, plane, pool, rates, jobs, bd=None, cands=True, fill=0xC3):
        """svt_hip_compound_search_batch_dev on the grids set before: `plane` the 2-D source luma plane (may be a strided view), `pool` the flat predictor pool of the
        same dtype, `rates` int32, `jobs` a ctypes array of CompSearchJob.  Results and candidate records start as the byte `fill`.
        -> (CompSearchResult * njobs, CompSearchCand * (20 njobs) or None)."""
        h, w = plane.shape
        pool, rates = np.ascontiguousarray(pool), np.ascontiguousarray(rates, np.int32)
        assert pool.dtype == plane.dtype
        n = len(jobs)
        rk, ck = CompSearchResult * max(n, 1), CompSearchCand * (COMP_SEARCH_MAX_CANDS * max(n, 1))
        with self.scope() as s:
            p, d_pool, d_rates = s.plane(plane), s.upload(pool), s.upload(rates)
            d_r = s.filled(C.sizeof(rk), fill, np.uint8)
            d_c = s.filled(C.sizeof(ck), fill, np.uint8) if cands else None
            self.call("compound_search_batch_dev", plane.itemsize, default_bd(plane.itemsize, bd), p.ptr, p.stride, w, h, d_pool, pool.size, d_rates if rates.size else None,
                      rates.size, C.cast(jobs, C.c_void_p), n, d_r, d_c)
            self.sync()
            return s.structs_back(d_r, rk), (s.structs_back(d_c, ck) if cands else None)

    # ---- the dual interpolation filter search
    def ifs_search_batch(self, src, ref0, ref1, jobs, dst=None, bd=None, cands=True, fill=0xC3, calls=1, lists=None):
        """svt_hip_ifs_search_batch_dev: `src` the 2-D source luma plane, `ref0` / `ref1` 2-D views whose sample (0, 0) is the reference picture's (the arrays behind
        them hold the border and are uploaded whole; ref1 may be None), `dst` None or the initial content of the destination plane, all of one dtype; `jobs` a ctypes
        array of IfsJob.  Results and candidate records start as the byte `fill`.  `calls` > 1 repeats the call back to back on the stream with no synchronisation in
        between; `lists` = [(first, count), ...] launches those parts of the list in that order instead of the whole, each writing its own part of the outputs.
        -> (IfsResult * njobs, IfsCand * (9 njobs) or None, dst after the calls or None)."""
        h, w = src.shape
        n = len(jobs)
        rk, ck = IfsResult * max(n, 1), IfsCand * (IFS_CANDS * max(n, 1))
        with self.scope() as s:
            p, r0 = s.plane(src), s.plane(ref0)
            r1 = s.plane(ref1) if ref1 is not None else None
            d = s.plane(dst) if dst is not None else None
            d_r = s.filled(C.sizeof(rk), fill, np.uint8)
            d_c = s.filled(C.sizeof(ck), fill, np.uint8) if cands else None
            for _ in range(calls):
                for first, count in (lists if lists is not None else [(0, n)]):
                    self.call("ifs_search_batch_dev", src.itemsize, default_bd(src.itemsize, bd), p.ptr, p.stride, w, h, r0.ptr, r0.stride, r1 and r1.ptr, r1.stride if r1 else 0,
                              d and d.ptr, d.stride if d else 0, C.cast(C.byref(jobs, first * C.sizeof(IfsJob)), C.c_void_p), count,
                              C.c_void_p(d_r.value + first * C.sizeof(IfsResult)), C.c_void_p(d_c.value + first * IFS_CANDS * C.sizeof(IfsCand)) if cands else None)
            self.sync()
            return s.structs_back(d_r, rk), (s.structs_back(d_c, ck) if cands else None), (s.plane_back(d) if d else None)

    # ---- OBMC in mode decision: the weighted target and the motion refinement
    def obmc_batch(self, plane=None, nbr=None, target_jobs=None, wm_samples=0, search=None, wsrc=None, mask=None, fill=0xC3):
        """svt_hip_obmc_target_batch_dev and / or svt_hip_obmc_search_batch_dev, back to back on the context's stream with no synchronisation between them.
        Target (when `target_jobs` is not None): `plane` the 2-D uint8 source luma plane, `nbr` the flat uint8 pool of neighbour predictions, `target_jobs` a ctypes
        array of ObmcTargetJob; wsrc / mask start as the byte `fill`.  Search (when `search` is not None): a dict of picture (the 2-D uint8 view of the reference
        picture inside its padded plane), pad_w, pad_h, mi_rows, mi_cols, joint_cost, comp_cost, jobs (a ctypes array of ObmcSearchJob); it reads the target
        stage's arrays, or `wsrc` / `mask` (int32) when there is no target stage; the results start as the byte `fill`.
        -> (wsrc, mask, ObmcSearchResult * njobs or None); wsrc / mask are None without a target stage."""
        with self.scope() as s:
            res = d_r = None
            if target_jobs is not None:
                h, w = plane.shape
                nbr = np.ascontiguousarray(nbr, np.uint8)
                p, d_n = s.plane(plane), s.upload(nbr)
                d_w, d_m = s.filled(max(wm_samples, 1) * 4, fill, np.uint8), s.filled(max(wm_samples, 1) * 4, fill, np.uint8)
                self.call("obmc_target_batch_dev", p.ptr, p.stride, w, h, d_n, nbr.size, C.cast(target_jobs, C.c_void_p), len(target_jobs), d_w, d_m, wm_samples)
            else:
                wsrc, mask = np.ascontiguousarray(wsrc, np.int32), np.ascontiguousarray(mask, np.int32)
                assert wsrc.size == mask.size
                d_w, d_m, wm_samples = s.upload(wsrc), s.upload(mask), wsrc.size
            if search is not None:
                pic = search["picture"]
                h, w = pic.shape
                j, c = ibc_cost_tables(search["joint_cost"], search["comp_cost"])
                r, d_jc, d_cc = s.plane(pic), s.upload(j), s.upload(c)
                n = len(search["jobs"])
                kind = ObmcSearchResult * max(n, 1)
                d_r = s.filled(C.sizeof(kind), fill, np.uint8)
                self.call("obmc_search_batch_dev", r.ptr, r.stride, w, h, search["pad_w"], search["pad_h"], search["mi_rows"], search["mi_cols"], d_w, d_m, wm_samples,
                          d_jc, d_cc, C.cast(search["jobs"], C.c_void_p), n, d_r)
            self.sync()
            if d_r is not None:
                res = s.structs_back(d_r, kind)
            if target_jobs is None:
                return None, None, res
            return s.download(d_w, (max(wm_samples, 1),), np.int32)[:wm_samples], s.download(d_m, (max(wm_samples, 1),), np.int32)[:wm_samples], res

    def filter_intra_predict_batch(self, edges, jobs, dst, bd=None):
        """svt_hip_filter_intra_predict_batch_dev: `edges` a flat uint8 / uint16 array of edge records, `jobs` a ctypes array of FilterIntraJob, `dst` the 2-D
        destination plane of the same dtype (may be an offset / strided view); bd 8 for uint8, 10 for uint16 unless `bd` says 8.  Returns the plane after the launch."""
        pix_bytes = edges.dtype.itemsize
        assert dst.dtype == edges.dtype
        with self.scope() as s:
            d_e, d_j, d = s.upload(edges), s.structs(jobs), s.plane(dst)
            self.call("filter_intra_predict_batch_dev", pix_bytes, default_bd(pix_bytes, bd), d_e, d_j, len(jobs), d.ptr, d.stride)
            self.sync()
            return s.plane_back(d)

    # ---- TPL flow dispenser
    def tpl_dispenser_picture(self, params, d_cur, cur_stride, refs, d_mv, d_ref_mask, d_ois_mode, d_ois_cost, d_recon, recon_stride):
        """svt_hip_tpl_dispenser_picture_dev on resident planes and tables: `params` a TplParams, `refs` a sequence of up to 7 TplRef (missing slots unused).
        The reconstruction (border included) stays on the device at d_recon; returns the statistics as a structured numpy array [mb_rows][mb_cols] whose
        fields are TplMbStats'."""
        mbw, mbh = (params.w + 15) // 16, (params.h + 15) // 16
        arr = (TplRef * TPL_MAX_REFS)()
        for i, r in enumerate(refs):
            arr[i] = r
        with self.scope() as s:
            d_stats = s.empty(mbw * mbh * C.sizeof(TplMbStats))
            d_scratch = s.empty(self.L.svt_hip_tpl_dispenser_scratch_bytes(params.w, params.h))
            self.call("tpl_dispenser_picture_dev", C.byref(params), d_cur, cur_stride, arr, d_mv, d_ref_mask, d_ois_mode, d_ois_cost, d_recon, recon_stride, d_stats,
                      d_scratch)
            self.sync()
            return s.download(d_stats, (mbh, mbw), np.dtype(TplMbStats))

    def tpl_recon_to_host(self, d_recon, recon_stride, w, h, pad):
        """The padded reconstruction tpl_dispenser_picture left at d_recon (sample (0, 0)): [h + 2 pad][w + 2 pad] uint8."""
        out = np.empty((h + 2 * pad, w + 2 * pad), np.uint8)
        top_left = C.c_void_p(d_recon.value - pad * recon_stride - pad)
        self.call("memcpy2d_d2h", out.ctypes.data_as(C.c_void_p), out.shape[1], top_left, recon_stride, out.shape[1], out.shape[0], what="d2h 2d")
        return out

    # ---- TPL flow synthesizer, r0 / beta / lambda factors
    def tpl_window(self, params, frames, d_out=None, d_scratch=None):
        """svt_hip_tpl_window_dev on resident records and grids: `frames` a TplWindowFrame array (tpl_window_frames) of device pointers.  Every grid stays on
        the device.  Returns the tpl_split_out dict; with the caller's d_out / d_scratch nothing is allocated here."""
        nbytes = self.L.svt_hip_tpl_r0beta_out_bytes(params.w, params.h, params.sb_size)
        with self.scope() as s:
            d_out = d_out if d_out is not None else s.empty(nbytes)
            d_scratch = d_scratch if d_scratch is not None else s.empty(self.L.svt_hip_tpl_r0beta_scratch_bytes())
            self.call("tpl_window_dev", C.byref(params), frames, len(frames), d_out, d_scratch)
            self.sync()
            return tpl_split_out(s.download(d_out, (nbytes,), np.uint8), params)

    def tpl_synth_picture(self, params, frames, frame_idx):
        """svt_hip_tpl_synth_picture_dev: the scatter of window picture frame_idx into the grids the descriptors name (nothing is zeroed)."""
        self.call("tpl_synth_picture_dev", C.byref(params), frames, len(frames), frame_idx)

    def tpl_r0beta(self, params, d_stats, d_dep):
        """svt_hip_tpl_r0beta_dev on one picture's resident records and grid -> the tpl_split_out dict."""
        nbytes = self.L.svt_hip_tpl_r0beta_out_bytes(params.w, params.h, params.sb_size)
        with self.scope() as s:
            d_out, d_scratch = s.empty(nbytes), s.empty(self.L.svt_hip_tpl_r0beta_scratch_bytes())
            self.call("tpl_r0beta_dev", C.byref(params), d_stats, d_dep, d_out, d_scratch)
            self.sync()
            return tpl_split_out(s.download(d_out, (nbytes,), np.uint8), params)

    def tpl_dep_to_host(self, params, d_dep):
        """One picture's grid: [rows][cols][2] int64 = {mc_dep_rate, mc_dep_dist} per cell."""
        s = 4 - params.cell_log2
        return self.to_host(d_dep, (((params.h + 15) // 16) << s, ((params.w + 15) // 16) << s, 2), np.int64)

    # ---- global motion
    def gm_shear_params_batch(self, wmmat):
        """svt_hip_gm_shear_params_batch_dev: `wmmat` [n][6] int32 -> a ctypes array of n GmModel."""
        wmmat = np.ascontiguousarray(wmmat, np.int32).reshape(-1, 6)
        n = len(wmmat)
        with self.scope() as s:
            d_in, d_out = s.upload(wmmat), s.empty(n * C.sizeof(GmModel))
            self.call("gm_shear_params_batch_dev", d_in, n, d_out)
            self.sync()
            return s.structs_back(d_out, GmModel * n)

    def gm_warp_error_batch(self, src, ref, models):
        """svt_hip_gm_warp_error_batch_dev: `src` / `ref` 2-D uint8 planes (offset / strided views allowed), `models` a ctypes array of GmModel -> int64 [n]."""
        with self.scope() as s:
            a, b, d_m = s.plane(src), s.plane(ref), s.structs(models)
            d_e = s.filled(max(len(models), 1), -7, np.int64)
            self.call("gm_warp_error_batch_dev", a.ptr, a.stride, src.shape[1], src.shape[0], b.ptr, ref.shape[1], ref.shape[0], b.stride, d_m, len(models), d_e)
            self.sync()
            return s.download(d_e, (len(models),), np.int64)

    def _gm_plane_table(self, s, planes, n_tab):
        tab = (GmRef * n_tab)()
        for i, r in enumerate(planes):
            p = s.plane(r)
            tab[i] = GmRef(p.ptr, r.shape[1], r.shape[0], p.stride, 0)
        return tab

    def gm_frame_error_batch(self, src, refs):
        """svt_hip_gm_frame_error_batch_dev: `src` and each of up to 8 `refs` a 2-D uint8 plane of one size -> int64 [len(refs)]."""
        with self.scope() as s:
            a, tab = s.plane(src), self._gm_plane_table(s, refs, GM_MAX_REFS)
            d_e = s.filled(max(len(refs), 1), -7, np.int64)
            self.call("gm_frame_error_batch_dev", a.ptr, a.stride, src.shape[1], src.shape[0], tab, len(refs), d_e)
            self.sync()
            return s.download(d_e, (len(refs),), np.int64)

    def gm_refine_picture(self, src, refs, jobs, repeat=1):
        """svt_hip_gm_refine_picture_dev: `src` a 2-D uint8 plane, `refs` up to 8 such planes (own sizes), `jobs` a ctypes array of GmJob.  `repeat` calls are issued
        back to back on the same scratch and results without a synchronisation of the caller's in between.  -> (ctypes array of GmResult, host polls of the last call)."""
        n = len(jobs)
        with self.scope() as s:
            a, tab = s.plane(src), self._gm_plane_table(s, refs, GM_MAX_REFS)
            d_j, d_o, d_x = s.structs(jobs), s.empty(n * C.sizeof(GmResult)), s.empty(self.L.svt_hip_gm_refine_scratch_bytes(n))
            polls = C.c_int(0)
            for _ in range(repeat):
                self.call("gm_refine_picture_dev", a.ptr, a.stride, src.shape[1], src.shape[0], tab, len(refs), d_j, n, d_o, d_x, C.byref(polls))
            self.sync()
            return s.structs_back(d_o, GmResult * n), polls.value

    def _gm_corners_dev(self, s, tab, n, max_points):
        """-> device pointers (points [n][max_points][2], counts [n], kept [n]) of svt_hip_gm_corners_batch_dev; nothing is synchronised."""
        d_p, d_c, d_k = s.filled((n, max_points, 2), -7, np.int32), s.filled(n, -7, np.int32), s.filled(n, -7, np.int32)
        d_x = s.empty(self.L.svt_hip_gm_corners_scratch_bytes(tab, n))
        self.call("gm_corners_batch_dev", tab, n, max_points, d_p, d_c, d_k, d_x)
        return d_p, d_c, d_k

    def gm_corners_batch(self, planes, max_points=GM_MAX_CORNERS):
        """svt_hip_gm_corners_batch_dev: up to 9 2-D uint8 `planes` (own sizes; offset / strided views allowed) -> (list of int32 [count][2] x, y per plane,
        counts int32 [n], kept-before-truncation int32 [n])."""
        n = len(planes)
        with self.scope() as s:
            d_p, d_c, d_k = self._gm_corners_dev(s, self._gm_plane_table(s, planes, 1 + GM_MAX_REFS), n, max_points)
            self.sync()
            pts, cnt, kept = s.download(d_p, (n, max_points, 2), np.int32), s.download(d_c, (n,), np.int32), s.download(d_k, (n,), np.int32)
            return [pts[i, :max(0, min(int(cnt[i]), max_points))].copy() for i in range(n)], cnt, kept

    def _scaled_planes(self, s, planes, shapes, dst):
        """Uploads 1 .. 3 source planes and their destinations (`dst[i]` a 2-D view to write into, or None / missing for a fresh zeroed plane of shapes[i]); views as
        in Scope.plane.  -> [(source Plane, destination Plane)]"""
        out = []
        for i, (src, shape) in enumerate(zip(planes, shapes)):
            d = dst[i] if dst is not None and dst[i] is not None else np.zeros(shape, src.dtype)
            assert d.shape == tuple(shape) and d.dtype == src.dtype == planes[0].dtype and src.dtype in (np.uint8, np.uint16)
            out.append((s.plane(src), s.plane(d)))
        return out

    def superres_upscale_planes(self, planes, out_widths, dst=None, bd=None):
        """svt_hip_superres_upscale_planes_dev: 1 .. 3 2-D `planes`, all uint8 (bd 8) or all uint16 (bd 10 unless `bd` says otherwise), each upscaled to its
        entry of `out_widths`; planes and the optional destinations `dst` may be offset / strided views.  -> the upscaled planes, each a view (like the one
        given) of a fresh copy of the whole destination array, so what lies around the plane can be checked through `.base`."""
        pix_bytes = planes[0].dtype.itemsize
        with self.scope() as s:
            recs = self._scaled_planes(s, planes, [(p.shape[0], w) for p, w in zip(planes, out_widths)], dst)
            tab = (UpscalePlane * len(recs))(*[UpscalePlane(a.ptr, a.stride, p.shape[1], b.ptr, b.stride, w, p.shape[0]) for (a, b), p, w in zip(recs, planes, out_widths)])
            self.call("superres_upscale_planes_dev", pix_bytes, default_bd(pix_bytes, bd), tab, len(recs))
            self.sync()
            return [s.plane_back(b) for _, b in recs]

    def resize_planes(self, planes, out_shapes, dst=None, bd=None, scratch=None):
        """svt_hip_resize_planes_dev: 1 .. 3 2-D `planes` (dtypes, views and `dst` as in superres_upscale_planes), each scaled to its (height, width) of
        `out_shapes`.  `scratch`, if given, is a uint8 array of at least svt_hip_resize_scratch_bytes that is used as the call's scratch and receives what
        the device left in it.  -> the scaled planes, as superres_upscale_planes returns them."""
        pix_bytes = planes[0].dtype.itemsize
        with self.scope() as s:
            recs = self._scaled_planes(s, planes, out_shapes, dst)
            tab = (ResizePlane * len(recs))(*[ResizePlane(a.ptr, a.stride, p.shape[1], p.shape[0], b.ptr, b.stride, o[1], o[0])
                                              for (a, b), p, o in zip(recs, planes, out_shapes)])
            need = self.L.svt_hip_resize_scratch_bytes(pix_bytes, tab, len(recs))
            d_x = s.upload(scratch) if scratch is not None else s.empty(need)
            self.call("resize_planes_dev", pix_bytes, default_bd(pix_bytes, bd), tab, len(recs), d_x, scratch.nbytes if scratch is not None else need)
            self.sync()
            if scratch is not None:
                scratch[...] = s.download(d_x, scratch.shape, np.uint8)
            return [s.plane_back(b) for _, b in recs]

    def scaled_jobs(self, sf0, sf1, frame_sizes, recs, fill=0xC3):
        """svt_hip_scaled_jobs_dev: `sf0` / `sf1` ScaleFactors of reference 0 / 1 (sf1 None: reference 1 is reference 0's twin), `frame_sizes` ((w0, h0), (w1, h1)),
        `recs` a ctypes array of ScaledRec.  -> ScaledBlk * n as the device left them (started as the byte `fill`)."""
        (w0, h0), (w1, h1) = frame_sizes
        with self.scope() as s:
            d_r, d_j = s.structs(recs), s.filled(len(recs) * C.sizeof(ScaledBlk), fill, np.uint8)
            self.call("scaled_jobs_dev", sf0, sf1, (i32 * 2)(w0, w1), (i32 * 2)(h0, h1), d_r, d_j, len(recs))
            self.sync()
            return s.structs_back(d_j, ScaledBlk * len(recs))

    def scaled_predict(self, ref0, ref1, dst, jobs, bd=None):
        """svt_hip_scaled_predict_batch_dev: `ref0`, `ref1` (None when no job is compound) and `dst` 2-D planes, all uint8 (bd 8) or all uint16 (bd 10 unless
        `bd` says otherwise); each may be an offset / strided view, and a job may read around its reference's view (a negative position) as far as the array
        the view lies in reaches.  `jobs` a ctypes array of ScaledBlk.  -> `dst` after the launch: a view like the one given of a fresh copy of the whole array."""
        pix_bytes = ref0.dtype.itemsize
        assert dst.dtype == ref0.dtype and (ref1 is None or ref1.dtype == ref0.dtype)
        with self.scope() as s:
            a, b, d, d_j = s.plane(ref0), s.plane(ref1) if ref1 is not None else None, s.plane(dst), s.structs(jobs)
            self.call("scaled_predict_batch_dev", pix_bytes, default_bd(pix_bytes, bd), a.ptr, a.stride, b and b.ptr, b.stride if b else 0, d.ptr, d.stride, d_j, len(jobs))
            self.sync()
            return s.plane_back(d)

    def gm_cross_correlation_batch(self, im1, im2, pairs):
        """svt_hip_gm_cross_correlation_batch_dev: `im1` / `im2` 2-D uint8 planes of one size, `pairs` [n][4] int32 x1, y1, x2, y2 -> float64 [n]."""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 4)
        assert im1.shape == im2.shape
        with self.scope() as s:
            a, b, d_q = s.plane(im1), s.plane(im2), s.upload(pairs)
            d_o = s.filled(max(len(pairs), 1), -7.0, np.float64)
            self.call("gm_cross_correlation_batch_dev", a.ptr, a.stride, b.ptr, b.stride, im1.shape[1], im1.shape[0], d_q, len(pairs), d_o)
            self.sync()
            return s.download(d_o, (len(pairs),), np.float64)

    def gm_correspondences_batch(self, src, refs, src_points=None, ref_points=None, max_points=GM_MAX_CORNERS):
        """svt_hip_gm_correspondences_batch_dev: `src` and up to 8 `refs` 2-D uint8 planes (the references are read at the source's size), `src_points` an int32
        [n][2] list and `ref_points` one such list per reference -> list of int32 [ncorr][4] x, y, rx, ry per reference.  With both lists None the corners come
        from svt_hip_gm_corners_batch_dev on the same stream and stay on the device in between."""
        h, w = src.shape
        n = len(refs)
        with self.scope() as s:
            if src_points is None and ref_points is None:
                tab = self._gm_plane_table(s, [src] + list(refs), 1 + GM_MAX_REFS)
                d_sp, d_sc, _ = self._gm_corners_dev(s, tab, n + 1, max_points)
                p_s, s_s = tab[0].d_plane, tab[0].stride
                rtab = (GmRef * GM_MAX_REFS)(*[tab[i + 1] for i in range(n)])
                d_rp, d_rc = C.c_void_p(d_sp.value + max_points * 8), C.c_void_p(d_sc.value + 4)   # the references' lists follow the source's
            else:
                a, rtab = s.plane(src), self._gm_plane_table(s, refs, GM_MAX_REFS)
                p_s, s_s = a.ptr, a.stride
                sp = np.ascontiguousarray(src_points, np.int32).reshape(-1, 2)
                assert len(sp) <= max_points and len(ref_points) == n
                rp = np.full((max(n, 1), max_points, 2), -7, np.int32)
                rc = np.zeros(max(n, 1), np.int32)
                for i, q in enumerate(ref_points):
                    q = np.ascontiguousarray(q, np.int32).reshape(-1, 2)
                    rp[i, :len(q)] = q; rc[i] = len(q)
                d_sp, d_sc, d_rp, d_rc = s.upload(sp), s.upload(np.array([len(sp)], np.int32)), s.upload(rp), s.upload(rc)
            d_o, d_n = s.filled((max(n, 1), max_points, 4), -7, np.int32), s.filled(max(n, 1), -7, np.int32)
            self.call("gm_correspondences_batch_dev", p_s, s_s, w, h, d_sp, d_sc, rtab, n, d_rp, d_rc, max_points, d_o, d_n)
            self.sync()
            out, cnt = s.download(d_o, (max(n, 1), max_points, 4), np.int32), s.download(d_n, (max(n, 1),), np.int32)
            assert all(0 <= int(c) <= max_points for c in cnt[:n])
            return [out[i, :int(cnt[i])].copy() for i in range(n)]

    def gm_fit_batch(self, corr, counts, jobs, n_refinements=5, want_inliers=True, want_jobs=True, repeat=1, refine=None, num_motions=1):
        """svt_hip_gm_fit_batch_dev: `corr` int32 [n_lists][max_points][4] and `counts` int32 [n_lists] as the correspondence call leaves them, `jobs` a list of
        (list index, model type).  `repeat` calls are issued back to back on the same scratch.  refine = (src, refs): svt_hip_gm_refine_picture_dev then runs on
        the jobs the fit wrote, without leaving the device.  -> (ctypes array of GmFit, int32 [njobs][max_points] inlier indices or None, ctypes array of GmJob or
        None, ctypes array of GmResult or None)."""
        corr = np.ascontiguousarray(corr, np.int32)
        counts = np.ascontiguousarray(counts, np.int32)
        n_lists, max_points = corr.shape[0], corr.shape[1]
        n = len(jobs)
        tab = (GmFitJob * max(n, 1))(*[GmFitJob(r, t) for r, t in jobs])
        with self.scope() as s:
            d_c, d_n = s.upload(corr), s.upload(counts)
            d_f = s.filled(max(n, 1) * C.sizeof(GmFit), 0xA5, np.uint8)
            d_i = s.filled((max(n, 1), max_points), -7, np.int32) if want_inliers else None
            d_j = s.filled(max(n, 1) * C.sizeof(GmJob), 0xA5, np.uint8) if want_jobs or refine else None
            d_x = s.empty(max(self.L.svt_hip_gm_fit_scratch_bytes(n, max_points), 8))
            for _ in range(repeat):
                self.call("gm_fit_batch_dev", d_c, d_n, n_lists, max_points, tab, n, num_motions, n_refinements, d_f, d_i, d_j, d_x)
            d_o = None
            if refine and n:
                src, refs = refine
                a, rtab = s.plane(src), self._gm_plane_table(s, refs, GM_MAX_REFS)
                d_o, d_y = s.empty(n * C.sizeof(GmResult)), s.empty(self.L.svt_hip_gm_refine_scratch_bytes(n))
                self.call("gm_refine_picture_dev", a.ptr, a.stride, src.shape[1], src.shape[0], rtab, len(refs), d_j, n, d_o, d_y, None)
            self.sync()
            fits = s.structs_back(d_f, GmFit * n)
            out_jobs = s.structs_back(d_j, GmJob * n) if d_j else None
            res = s.structs_back(d_o, GmResult * n) if d_o else None
            inl = s.download(d_i, (max(n, 1), max_points), np.int32)[:n] if d_i else None
            return fits, inl, out_jobs, res

    def gm_estimate_picture(self, src, refs, rotzoom_model_only=0, allow_high_precision_mv=0, n_refinements=5, max_points=GM_MAX_CORNERS, repeat=1):
        """svt_hip_gm_estimate_picture_dev: `src` a 2-D uint8 plane, `refs` up to 8 such planes at least as large (offset / strided views allowed); `repeat` calls
        on the same scratch -> ctypes array of GmEstimate, one per reference (of the last call)."""
        h, w = src.shape
        with self.scope() as s:
            a, rtab = s.plane(src), self._gm_plane_table(s, refs, GM_MAX_REFS)
            opt = GmEstimateOptions(rotzoom_model_only, allow_high_precision_mv, n_refinements, max_points)
            d_x = s.empty(max(self.L.svt_hip_gm_estimate_scratch_bytes(w, h, len(refs), C.byref(opt)), 256))
            out = (GmEstimate * max(len(refs), 1))()
            for _ in range(repeat):
                self.call("gm_estimate_picture_dev", a.ptr, a.stride, w, h, rtab, len(refs), C.byref(opt), out, d_x)
            return out

    def close(self):
        if self.h:
            self.L.svt_hip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

