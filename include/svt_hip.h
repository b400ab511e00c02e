/*
 * svt_hip.h — C ABI of libsvtav1_hip.so: the MI355X (gfx950) implementation of SVT-AV1's
 * per-superblock hot path (open-loop ME, transform/quant, in-loop filters) and of the look-ahead's source-side chain
 * (open-loop intra search, TPL flow dispenser, TPL flow synthesizer with r0 / beta / lambda factors, global motion).
 *
 * This is the drop-in boundary.  The reference binds kernels through global function pointers
 * (Source/Lib/Encoder/Codec/aom_dsp_rtcd.h, Source/Lib/Common/Codec/common_dsp_rtcd.h) that are
 * filled once in svt_av1_enc_init (Source/Lib/Encoder/Globals/EbEncHandle.c:1144-1145).  Two
 * families of entry points are exported:
 *
 *   (1) batched, frame-level calls (svt_hip_*_frame / *_batch): one call = one kernel launch over
 *       every 64x64 superblock of a picture.  They replace the per-SB loops of the reference's
 *       process kernels (EbMotionEstimationProcess.c:831-963, EbDlfProcess.c:175-216,
 *       EbCdefProcess.c:510-534 ...).  `_dev` variants take device pointers (inputs already
 *       resident in HBM); the plain variants take host pointers and move the data themselves.
 *   (2) per-call wrappers with the exact RTCD signatures (svt_*_hip), installable into the
 *       reference's dispatch tables by svt_hip_setup_rtcd().  They exist for
 *       parity testing against the reference's unit-test matrices; a per-block GPU round trip is
 *       never the fast path.
 *
 * Conventions: plain C types only; every function returns 0 on success and a nonzero
 * SvtHipStatus otherwise (the caller then keeps using the C pointer, mirroring the reference's
 * "kernels cannot fail" convention).  No CPU fallback exists inside this library:
 * if no gfx950 device is present svt_hip_init fails loudly.
 */
#ifndef SVT_HIP_H
#define SVT_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the functions declared in this header are exported */
#pragma GCC visibility push(default)

typedef enum {
    SVT_HIP_OK              = 0,
    SVT_HIP_ERR_NO_DEVICE   = 1, /* no HIP device / not gfx950 */
    SVT_HIP_ERR_BAD_ARG     = 2,
    SVT_HIP_ERR_RUNTIME     = 3, /* a HIP call failed; see svt_hip_last_error() */
    SVT_HIP_ERR_UNSUPPORTED = 4
} SvtHipStatus;

#define SVT_HIP_SQUARE_PU_COUNT 85              /* Encoder/Codec/EbMotionEstimationLcuResults.h:22 */
#define SVT_HIP_MAX_SAD_VALUE (128 * 128 * 255) /* Encoder/Codec/EbMotionEstimation.h:93 */

typedef struct SvtHipCtx SvtHipCtx; /* opaque: device, stream, scratch buffers */

/* ------------------------------------------------------------------ context / memory ---------- */
int         svt_hip_init(int device_id, SvtHipCtx **ctx);
void        svt_hip_destroy(SvtHipCtx *ctx);
const char *svt_hip_last_error(const SvtHipCtx *ctx);
/* Adopt an externally owned hipStream_t (e.g. the caller's); NULL restores the context's own. */
int  svt_hip_set_stream(SvtHipCtx *ctx, void *hip_stream);
int  svt_hip_sync(SvtHipCtx *ctx);
int  svt_hip_malloc(SvtHipCtx *ctx, void **dptr, size_t bytes);
int  svt_hip_free(SvtHipCtx *ctx, void *dptr);
int  svt_hip_memcpy_h2d(SvtHipCtx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int  svt_hip_memcpy_d2h(SvtHipCtx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int  svt_hip_memcpy_d2d(SvtHipCtx *ctx, void *dst_dev, const void *src_dev, size_t bytes); /* asynchronous, stream-ordered */
/* picture planes: `rows` rows of `width_bytes`, pitches in bytes (EbPictureBufferDesc planes keep their own strides) */
int  svt_hip_memcpy2d_h2d(SvtHipCtx *ctx, void *dst_dev, size_t dst_pitch, const void *src_host, size_t src_pitch, size_t width_bytes, size_t rows);
int  svt_hip_memcpy2d_d2h(SvtHipCtx *ctx, void *dst_host, size_t dst_pitch, const void *src_dev, size_t src_pitch, size_t width_bytes, size_t rows);
/* stream-ordered forms: return once the copy is queued; the host side must stay untouched (and, for the copy to really overlap, be page-locked:
 * svt_hip_host_register / svt_hip_host_alloc) until svt_hip_sync */
int  svt_hip_memcpy_h2d_async(SvtHipCtx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int  svt_hip_memcpy_d2h_async(SvtHipCtx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int  svt_hip_memcpy2d_h2d_async(SvtHipCtx *ctx, void *dst_dev, size_t dst_pitch, const void *src_host, size_t src_pitch, size_t width_bytes, size_t rows);
int  svt_hip_memcpy2d_d2h_async(SvtHipCtx *ctx, void *dst_host, size_t dst_pitch, const void *src_dev, size_t src_pitch, size_t width_bytes, size_t rows);
/* page-lock a buffer of the caller in place (the reference allocates its picture buffers once per encoder instance: EbPictureBufferDesc planes registered
 * once are copied by direct DMA afterwards); registering a registered range again is not an error.  svt_hip_host_alloc = page-locked staging memory. */
int  svt_hip_host_register(SvtHipCtx *ctx, void *host, size_t bytes);
int  svt_hip_host_unregister(SvtHipCtx *ctx, void *host);
int  svt_hip_host_alloc(SvtHipCtx *ctx, void **host, size_t bytes);
int  svt_hip_host_free(SvtHipCtx *ctx, void *host);
/* number of HIP devices visible to the process (0 and SVT_HIP_OK when there is none) */
int  svt_hip_device_count(int *count);
/* load the code object of every kernel translation unit for the context's device now (otherwise each is loaded at the first launch of one of its kernels,
 * which inside an encoder is the first pictures' clock) */
int  svt_hip_warmup(SvtHipCtx *ctx);
/* HIP-event stopwatch on the context's stream (used by bench.py for per-kernel device time). */
int  svt_hip_timer_start(SvtHipCtx *ctx);
int  svt_hip_timer_stop_ms(SvtHipCtx *ctx, float *elapsed_ms);

/* ------------------------------------------------------------------ open-loop ME --------------- */
/* Per-SB search descriptor = the window integer_search_sb derives for one (SB, reference)
 * (Encoder/Codec/EbMotionEstimation.c:1922-2066).  svt_hip_me_search_window() reproduces that
 * arithmetic on the host. */
typedef struct {
    int32_t sb_x, sb_y;                        /* SB origin in luma pixels */
    int16_t x_origin, y_origin, width, height; /* search area: origin relative to the SB, size */
} SvtHipSbSearch;

SvtHipSbSearch svt_hip_me_search_window(int sb_origin_x, int sb_origin_y, int x_center, int y_center,
                                        int sa_width, int sa_height, int pic_width, int pic_height);

/* Integer full search, all 85 square PUs, every SB of a frame, one reference.
 * Replaces open_loop_me_fullpel_search_sblock (EbMotionEstimation.c:814) and the kernels behind
 * svt_ext_all_sad_calculation_8x8_16x16 / svt_ext_eight_sad_calculation_32x32_64x64
 * (aom_dsp_rtcd.h:640-641) + single-candidate tails (:630,:636).
 *   src/ref : padded luma planes (u8), `stride` bytes per row (multiple of 4), pixel (0,0) at
 *             [org_y*stride + org_x]; the window of every SB must lie inside the padded plane.
 *   best_sad/best_mv : [n_sb][85] in EbMeTierZeroPu order (EbMotionEstimationContext.h:51-137);
 *             MV word = (y_mv << 16) | x_mv in quarter-pel int16 halves (EbDefinitions.h:2346).
 *   sub_sad : SUB_SAD_SEARCH (every other row, SAD doubled) vs FULL_SAD_SEARCH. */
int svt_hip_me_fullpel_frame_dev(SvtHipCtx *ctx, const uint8_t *d_src, const uint8_t *d_ref, int stride,
                                 int org_x, int org_y, const SvtHipSbSearch *d_sbs, int n_sb, int sub_sad,
                                 uint32_t *d_best_sad, uint32_t *d_best_mv);
int svt_hip_me_fullpel_frame(SvtHipCtx *ctx, const uint8_t *src, const uint8_t *ref, int stride, int plane_rows,
                             int org_x, int org_y, const SvtHipSbSearch *sbs, int n_sb, int sub_sad,
                             uint32_t *best_sad, uint32_t *best_mv);
/* Search areas above 65 536 candidates (the reference configures up to 750 x 750, EbMotionEstimationProcess.c:124-137) are searched by a second
 * launch of the same kernel that walks the window strip by strip; SBs with smaller windows leave it at once.  The _dev entry point cannot see the
 * descriptors, so that launch is always issued unless the caller declares that no window of this context exceeds 65 536 candidates (enable = 0;
 * an oversized window then yields SVT_HIP_MAX_SAD_VALUE for every PU of its SB).  The host-pointer entry point decides per call. */
int svt_hip_me_set_big_windows(SvtHipCtx *ctx, int enable);
/* the current setting (*enabled = 0 / 1): a caller that switches it for one call puts the context's own value back */
int svt_hip_me_get_big_windows(SvtHipCtx *ctx, int *enabled);
/* Tuning knob: low 4 bits = waves per SB workgroup (1, 2 or 4; default 4); bits 4.. = KiB of unused LDS added to each workgroup
 * (0 = off): with >= 56 only one ME workgroup fits a CU, which leaves half of every SIMD's registers to kernels running concurrently
 * on other streams (measured: ME alone 0.40 -> 0.63 ms, whole step unchanged -- see DESIGN.md 5). */
int svt_hip_me_set_waves_per_sb(SvtHipCtx *ctx, int waves);

/* ------------------------------------------------------- residual + transform + quantisation ---- */
/* One launch = a list of transform blocks of ONE size in one plane.  A block descriptor packs the
 * block position (pixels, relative to the plane pointers) and its TxType (enum order of the
 * reference, DCT_DCT = 0 .. H_FLIPADST = 15, Source/Lib/Common/Codec/EbDefinitions.h). */
#define SVT_HIP_TX_DESC(x, y, tx_type) ((uint32_t)(x) | ((uint32_t)(y) << 14) | ((uint32_t)(tx_type) << 28))

/* Quantizer of a launch = the {dc, ac} entries the reference takes from Quants/Dequants for one
 * (qindex, plane) (Encoder/Codec/EbFullLoop.c:1428-1489) plus the variant:
 *   0 svt_aom_quantize_b (8-bit, EbFullLoop.c:37)      1 svt_aom_highbd_quantize_b (:171)
 *   2 svt_av1_quantize_fp[_32x32|_64x64] (:379,557,580) 3 svt_av1_highbd_quantize_fp (:534)
 * For variants 2/3 pass round_fp_qtx / quant_fp_qtx in round / quant (as the facades :603-711 do).
 * log_scale = av1_get_tx_scale_tab[tx_size] (EbFullLoop.h:66).  Quant matrices are flat on this path.
 * coeff_shape = the EB_TRANS_COEFF_SHAPE argument of av1_estimate_transform (Encoder/Codec/EbTransforms.c:3613,
 * EbDefinitions.h:2610-2614): 0 DEFAULT_SHAPE, 1 N2_SHAPE (only the top-left W/2 x H/2 coefficients are produced, the
 * rest are zero), 2 N4_SHAPE (W/4 x H/4), 3 ONLY_DC_SHAPE (coefficient 0 only).  For shapes 1-3 the 64-point energy
 * is 0, as handle_transform*_N2_N4 (:2933-2964) returns it. */
typedef struct {
    int32_t zbin[2], round[2], quant[2], quant_shift[2], dequant[2];
    int32_t log_scale, variant;
    int32_t coeff_shape;
} SvtHipQuantParams;
/* Device pointers to the inverse scan (position of coefficient rc in scan order) of the launch's
 * tx_size for the three scan classes of av1_scan_orders (Common/Codec/EbCoefficients.h:2563):
 * [0] default zig-zag, [1] mrow, [2] mcol.  Classes 1/2 are only read for sizes <= 16x16. */
typedef struct {
    const int16_t *iscan[3];
} SvtHipScanTables;

/* residual (src - pred) -> forward 2-D transform -> [64-pt zero-out/re-pack + energy] -> quantize.
 * Replaces svt_residual_kernel8bit/16bit (common_dsp_rtcd.h:169), av1_estimate_transform
 * (EbTransforms.c:3613: svt_av1_fwd_txfm2d_WxH[_N2|_N4], aom_dsp_rtcd.h:129-135, 284-350;
 * svt_handle_transform64x*[_N2_N4], :230; qp->coeff_shape, default shape when qp is NULL) and the quantizers (:252-258) +
 * cul_level (EbFullLoop.c:1595-1608) for a whole list of blocks.
 *   pix_bytes 1: uint8_t planes, 2: uint16_t planes; strides in pixels.
 *   coeff / qcoeff+dqcoeff / eob / cul_level / energy may be NULL independently (qcoeff and dqcoeff
 *   go together); outputs are packed min(W,32) x min(H,32) int32 per block, block after block. */
int svt_hip_fwd_txfm_quant_batch_dev(SvtHipCtx *ctx, int tx_size, int pix_bytes, const void *d_src, int src_stride,
                                     const void *d_pred, int pred_stride, const uint32_t *d_descs, int nblk,
                                     const SvtHipQuantParams *qp, const SvtHipScanTables *scans, int32_t *d_coeff,
                                     int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob, int32_t *d_cul_level,
                                     uint64_t *d_energy);
/* dequantized coefficients -> inverse 2-D transform -> add to prediction -> clip -> recon.
 * Replaces svt_av1_inv_txfm2d_add_WxH (common_dsp_rtcd.h:117-153) / svt_av1_inv_txfm_add (:156).
 * recon may alias pred (in-place reconstruction). bd = 8 or 10 (bd 8 with pix_bytes 2 = the
 * 16-bit pipeline on 8-bit content). */
int svt_hip_inv_txfm_add_batch_dev(SvtHipCtx *ctx, int tx_size, int pix_bytes, int bd, const int32_t *d_dqcoeff,
                                   const void *d_pred, int pred_stride, void *d_recon, int recon_stride,
                                   const uint32_t *d_descs, int nblk);
/* The lossless 4x4 inverse (reversible Walsh-Hadamard) + add + clip for a list of blocks: svt_av1_highbd_iwht4x4_16_add_c /
 * svt_av1_highbd_iwht4x4_1_add_c (Common/Codec/EbInvTransforms.c:2771-2857), chosen per block by eob > 1 like highbd_iwht4x4_add (:2858-2864;
 * d_eob NULL = the 16-coefficient form for every block).  16 int32 per block, block after block; descs as above (tx_type ignored).
 * What svt_av1_highbd_inv_txfm_add_4x4 (:2870-2882) runs when TxfmParam.lossless is set -- the reference ENCODER never sets it
 * (Encoder/Codec/EbCodingLoop.c:1068-1243, EbFullLoop.c:1852-1863 pass 0), so this entry point serves the per-call pointer
 * svt_av1_inv_txfm_add only. */
int svt_hip_iwht4x4_add_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const int32_t *d_dqcoeff, const uint16_t *d_eob,
                                  const void *d_pred, int pred_stride, void *d_recon, int recon_stride,
                                  const uint32_t *d_descs, int nblk);

/* Mixed-size launches: the same two operations for up to any number of (transform size, plane) job lists in ONE launch per 16 jobs.
 * A frame's transform work is 15-20 short lists; launched one by one each leaves most of the 256 CUs idle.  Fields as in the
 * single-size entry points; jobs is a HOST array (copied into the kernel arguments), every pointer inside is a device pointer. */
typedef struct {
    int32_t tx_size, nblk;
    const void *d_src;  int32_t src_stride;
    const void *d_pred; int32_t pred_stride;
    const uint32_t *d_descs;
    SvtHipQuantParams qp;
    SvtHipScanTables scans;
    int32_t *d_coeff, *d_qcoeff, *d_dqcoeff;
    uint16_t *d_eob;
    int32_t *d_cul_level;
    uint64_t *d_energy;
} SvtHipFwdTxJob;
typedef struct {
    int32_t tx_size, nblk;
    const int32_t *d_dqcoeff;
    const void *d_pred; int32_t pred_stride;
    void *d_recon;      int32_t recon_stride;
    const uint32_t *d_descs;
} SvtHipInvTxJob;
int svt_hip_fwd_txfm_quant_multi_dev(SvtHipCtx *ctx, int pix_bytes, const SvtHipFwdTxJob *jobs, int njobs);
/* The encode loop's per-block chain in ONE launch (Encoder/Codec/EbCodingLoop.c:379-596: residual -> forward transform -> quantize -> inverse
 * quantize -> inverse transform -> reconstruction): the job lists of svt_hip_fwd_txfm_quant_multi_dev with the reconstruction plane of each job.
 * The dequantised coefficients go from the quantizer to the inverse transform in registers; fwd.d_qcoeff is required, fwd.d_dqcoeff may be NULL
 * (then they are never written).  d_recon may be the prediction plane itself (in-place reconstruction) when no two blocks of a job overlap. */
typedef struct {
    SvtHipFwdTxJob fwd;
    void *d_recon; int32_t recon_stride;
} SvtHipEncTxJob;
int svt_hip_enc_txfm_multi_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const SvtHipEncTxJob *jobs, int njobs);
int svt_hip_inv_txfm_add_multi_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const SvtHipInvTxJob *jobs, int njobs);

/* ------------------------------------------------------------------ deblocking loop filter ------ */
/* Per luma 4x4 unit summary of the reference's ModeInfo fields that set_lpf_parameters reads
 * (Encoder/Codec/EbDeblockingFilter.c:168-319): transform size actually used by the block in each
 * plane (get_transform_size, :134), prediction block size (sb_type), "skip && inter", and the filter
 * level already looked up in LoopFilterInfoN.lvl[plane][seg][dir][ref][mode] for the block. */
typedef struct {
    uint8_t tx_w_log2, tx_h_log2;       /* luma transform block, pixels, log2 (2..6) */
    uint8_t uv_tx_w_log2, uv_tx_h_log2; /* chroma transform block in chroma pixels, log2 */
    uint8_t bw_log2, bh_log2;           /* prediction block in luma pixels, log2 */
    uint8_t skip_inter;                 /* mbmi->skip && is_inter_block */
    uint8_t level[3][2];                /* [plane][0 = vertical edges, 1 = horizontal edges] */
} SvtHipDlfModeInfo;
/* Host: edge descriptors of one plane from the mode-info grid; restates set_lpf_parameters.
 * edges_v / edges_h: [units_h][units_w] uint16 = (level << 8) | filter_length(0,4,6,8,14) for the
 * edge on the left / top of each 4x4 unit of the plane; units = ceil(plane dim / 4). */
int svt_hip_dlf_build_edges(const SvtHipDlfModeInfo *mi, int mi_cols, int mi_rows, int plane, int ss_x, int ss_y,
                            int plane_w, int plane_h, uint16_t *edges_v, uint16_t *edges_h);
/* The same for a coded picture that contains padding (a source size that is not a multiple of 8 is coded padded): the reference's loops
 * (svt_av1_filter_block_plane_vert / _horz, EbDeblockingFilter.c:338-367, :479-508) stop at the unpadded extent in the last superblock row /
 * column, so units with x >= filt_units_w or y >= filt_units_h carry no edge.  svt_hip_dlf_filtered_units gives that extent along one axis:
 * coded_luma = the coded (padded) luma size, pad = scs->max_input_pad_right / _bottom, sb_size = 64 or 128, ss = the plane's subsampling;
 * -1 for arguments outside that domain. */
int svt_hip_dlf_filtered_units(int coded_luma, int pad, int sb_size, int ss);
int svt_hip_dlf_build_edges_crop(const SvtHipDlfModeInfo *mi, int mi_cols, int mi_rows, int plane, int ss_x, int ss_y, int plane_w,
                                 int plane_h, int filt_units_w, int filt_units_h, uint16_t *edges_v, uint16_t *edges_h);
/* svt_hip_dlf_build_edges_crop for the three planes of a picture (chroma sub-sampled by ss_x / ss_y) in one launch, from a mode-info grid in DEVICE memory:
 * a 3840 x 2160 picture has 777 600 units in two directions, which cost the host builder 2.5 ms per call on one thread and the edge planes a 3 MB upload.
 * level[plane][dir] >= 0 stands for the level of every record (frame-uniform levels, the case whenever the frame header carries no delta_lf and no
 * mode / reference deltas: svt_av1_loop_filter_frame_init, Common/Codec/EbDeblockingCommon.c:105-160) — one upload of the grid then serves the level
 * search and the filter itself; level == NULL or an entry < 0 reads the records' own levels.  A plane whose two output pointers are NULL is skipped.
 * filt_units_w / _h: see svt_hip_dlf_filtered_units; plane_w / plane_h in samples; the outputs are [ceil(plane_h / 4)][ceil(plane_w / 4)] as above. */
int svt_hip_dlf_build_edges_picture_dev(SvtHipCtx *ctx, const SvtHipDlfModeInfo *d_mi, int mi_cols, int mi_rows, int ss_x, int ss_y, const int plane_w[3],
                                        const int plane_h[3], const int filt_units_w[3], const int filt_units_h[3], const int (*level)[2],
                                        uint16_t *const d_edges_v[3], uint16_t *const d_edges_h[3]);
/* Deblock one plane in place: all vertical edges, then all horizontal edges (normative order;
 * replaces svt_av1_loop_filter_frame for that plane, EbDeblockingFilter.c:711, and the 16 edge
 * kernels svt_aom_[highbd_]lpf_{horizontal,vertical}_{4,6,8,14}, common_dsp_rtcd.h:1051-1081).
 * Either descriptor pointer may be NULL to run a single direction (filter-level search probes). */
int svt_hip_deblock_plane_dev(SvtHipCtx *ctx, void *d_plane, int pix_bytes, int stride, int bd, const uint16_t *d_edges_v,
                              const uint16_t *d_edges_h, int units_w, int units_h, int sharpness);
/* The same for all three planes of a picture in two launches (every vertical edge of every plane, then every horizontal edge):
 * svt_av1_loop_filter_frame(frame, pcs, 0, 3).  A NULL plane pointer skips that plane (frame filter level 0). */
int svt_hip_deblock_frame_dev(SvtHipCtx *ctx, void *const d_plane[3], int pix_bytes, const int stride[3], int bd,
                              const uint16_t *const d_edges_v[3], const uint16_t *const d_edges_h[3], const int units_w[3],
                              const int units_h[3], int sharpness);
/* svt_av1_loop_filter_frame(frame, pcs, 0, 3) in ONE launch, out of place: d_dst[p] receives the deblocked plane p (same stride as d_src[p], which is left
 * untouched; d_dst[p] != d_src[p]).  A workgroup stages a 128 x 64 tile with the 7 samples around it, filters the vertical edges of the staged region and then
 * the horizontal edges of the tile on chip (loop_filter_sb does both per superblock, EbDeblockingFilter.c:614): the picture is read 1.35 times and written once
 * instead of two read-modify-write passes.  plane_w / plane_h: extent of the plane in samples (the edge planes are (plane_w + 3) / 4 units wide at least).
 * A NULL d_src[p] skips the plane. */
int svt_hip_deblock_frame_fused_dev(SvtHipCtx *ctx, const void *const d_src[3], void *const d_dst[3], int pix_bytes, const int stride[3], int bd,
                                    const int plane_w[3], const int plane_h[3], const uint16_t *const d_edges_v[3], const uint16_t *const d_edges_h[3],
                                    const int units_w[3], const int units_h[3], int sharpness);
/* Sum of squared differences of two planes: svt_spatial_full_distortion_kernel (8-bit) /
 * svt_full_distortion_kernel16_bits (16-bit containers) as called by picture_sse_calculations
 * (Encoder/Codec/EbDeblockingFilter.c:830-961).  *d_sse (device) receives the sum (it is cleared by the call). */
int svt_hip_plane_sse_dev(SvtHipCtx *ctx, int pix_bytes, const void *d_a, int a_stride, const void *d_b, int b_stride, int w,
                          int h, uint64_t *d_sse);
/* svt_av1_pick_filter_level's search for one plane / direction: search_filter_level + try_filter_frame
 * (Encoder/Codec/EbDeblockingFilter.c:966-1187).  Every probe = copy of the unfiltered plane, whole-plane
 * deblock at the probed level, SSE against the source; the probe sequence and the integer bias rule are the
 * reference's.  As in the reference's search the level is frame-uniform (no segment / ref / mode deltas):
 * the edge descriptors only supply the geometry (any non-zero level in them is replaced by the probed one). */
typedef struct {
    int plane;             /* 0 Y, 1 U, 2 V */
    int dir;               /* luma: 0 = search filter_level[0] (vertical edges), 1 = filter_level[1]; ignored for chroma */
    int other_level;       /* luma: the frame header's level of the other direction (try_filter_frame :976-979) */
    int start_level;       /* last_frame_filter_level[dir | 2 | 3] */
    int loop_filter_mode;  /* pcs->parent_pcs_ptr->loop_filter_mode: <= 2 -> one +-2 refinement, else the full step search */
    int tx_mode_only_4x4;  /* frm_hdr->tx_mode == ONLY_4X4 (bias is not halved) */
    int sharpness;
} SvtHipDlfSearch;
/* d_recon: unfiltered plane (read only); d_tmp: scratch plane of the same geometry; best_err = ss_err[best_level]. */
int svt_hip_dlf_search_level_dev(SvtHipCtx *ctx, const SvtHipDlfSearch *p, const void *d_recon, void *d_tmp, int pix_bytes,
                                 int stride, int bd, int plane_w, int plane_h, const void *d_src, int src_stride,
                                 const uint16_t *d_edges_v, const uint16_t *d_edges_h, int units_w, int units_h,
                                 uint64_t *d_sse_scratch, int *best_level, int64_t *best_err);

/* The searches of several planes of one picture advanced in LOCKSTEP (svt_av1_pick_filter_level, Encoder/Codec/EbDeblockingFilter.c:1189-1300, runs search_filter_level
 * for luma, U and V one after the other; a plane's probes depend on nothing but that plane): every round measures, for every plane still searching, the one or two levels
 * its walk needs next (the low and the high neighbour of an iteration are both measured before either is compared) — all probes of a round are queued and waited for
 * once.  A 4:2:0 picture's three searches take 6-8 round trips instead of ~25.  d_tmp[0..1]: two scratch planes of the plane's geometry; d_sse_scratch: 2 * n_planes words. */
typedef struct {
    SvtHipDlfSearch q;
    const void     *d_recon;
    void           *d_tmp[2];
    int             stride, plane_w, plane_h;
    const void     *d_src;
    int             src_stride;
    const uint16_t *d_edges_v, *d_edges_h;
    int             units_w, units_h;
} SvtHipDlfSearchPlane;
int svt_hip_dlf_search_levels_picture_dev(SvtHipCtx *ctx, int n_planes, const SvtHipDlfSearchPlane *planes, int pix_bytes, int bd, uint64_t *d_sse_scratch,
                                          int *best_level, int64_t *best_err);

/* ------------------------------------------------------------------ CDEF ------------------------ */
/* Strength search of cdef_seg_search / cdef_seg_search16bit (Encoder/Codec/EbCdefProcess.c:80-475)
 * for every 64x64 filter block of a 4:2:0 frame in two launches (luma, then both chroma planes):
 *   d_rec[3]  deblocked reconstruction planes, d_src[3] source planes (pixel (0,0) pointers, strides in
 *             pixels); w x h = luma size (multiples of 8; a last filter block narrower than 16 luma
 *             pixels is not supported, see DESIGN.md "CDEF borders")
 *   d_skip8   [h/8][w/8], 1 = the 8x8 luma block is entirely skip (is_8x8_block_skip, EbEncCdef.c:239)
 *   d_mse     [2][nfb][64] uint64: distortion of plane 0 (Y) / 1 (U+V) for strength index
 *             gi = pri*4 + sec_idx of the full search (pcs->mse_seg, CDEF_FULL_SEARCH); the reduced
 *             pick methods are subsets of these 64 entries (get_cdef_filter_strengths,
 *             Common/Codec/EbDefinitions.h:1696).  Entries of all-skip filter blocks are not written.
 *   d_dir/d_var [nfb][64] scratch/outputs: direction and variance of every 8x8 block (svt_cdef_find_dir); 0 for a
 *             skipped block and outside the picture.
 * Replaces svt_cdef_find_dir, svt_cdef_filter_block, svt_copy_rect8_8bit_to_16bit,
 * svt_compute_cdef_dist_{8bit,16bit} (common_dsp_rtcd.h:1032-1037, aom_dsp_rtcd.c:97-98). */
int svt_hip_cdef_search_frame_dev(SvtHipCtx *ctx, int pix_bytes, const void *const d_rec[3], const int rec_stride[3],
                                  const void *const d_src[3], const int src_stride[3], int w, int h,
                                  const uint8_t *d_skip8, int pri_damping, int bd, uint64_t *d_mse, uint8_t *d_dir,
                                  int32_t *d_var);
/* Frame application of svt_av1_cdef_frame / av1_cdef_frame16bit (Encoder/Codec/EbEncCdef.c:292-1031).
 * d_in = pre-CDEF planes, d_out = destination planes (distinct from d_in); every sample of the picture is written — samples of skipped
 * blocks and of unfiltered filter blocks are passed through — so d_out needs no initial copy of d_in; y/uv_strength[nfb] = the frame
 * header strength value (pri*4 + sec_idx) selected for each filter block.  d_var == NULL: the directions are computed here and left in
 * d_dir; d_var != NULL: d_dir / d_var are the per-8x8 direction and variance svt_hip_cdef_search_frame_dev produced for the same
 * pre-CDEF picture (svt_cdef_find_dir is deterministic in the picture, so the reference recomputes the same values) and are reused. */
int svt_hip_cdef_apply_frame_dev(SvtHipCtx *ctx, int pix_bytes, const void *const d_in[3], void *const d_out[3],
                                 const int stride[3], int w, int h, const uint8_t *d_skip8, const uint8_t *d_y_strength,
                                 const uint8_t *d_uv_strength, int damping, int bd, uint8_t *d_dir, const int32_t *d_var);

/* ------------------------------------------------------- sub-pel prediction, block SAD / variance */
/* One block of a batched prediction launch.  mode 0 = AV1 single-reference convolve, i.e. what
 * convolve[subpel_x != 0][subpel_y != 0][0] dispatches to (svt_av1_[highbd_]convolve_{2d_copy,x,y,2d}_sr,
 * common_dsp_rtcd.h:197-219; round_0 = 3, round_1 = 11); mode 1 = svt_aom_upsampled_pred
 * (aom_dsp_rtcd.h:354; two convolve8 passes with an 8-bit intermediate; 8-bit planes only, pass
 * subpel_q3 << 1 as the phase).  Kernel banks: 0 EIGHTTAP_REGULAR, 1 EIGHTTAP_SMOOTH, 2 MULTITAP_SHARP,
 * 3 BILINEAR, 4 / 5 the 4-tap regular / smooth kernels AV1 uses for w <= 4
 * (av1_get_interp_filter_params_with_block_size, Common/Codec/EbInterPrediction.c:1254). */
typedef struct {
    int32_t src_x, src_y; /* integer position of the block's top-left sample in the reference plane */
    int32_t dst_x, dst_y;
    uint8_t w, h;         /* 4..128 */
    uint8_t bank_x, bank_y;
    uint8_t subpel_x, subpel_y; /* q4 phase 0..15 */
    uint8_t mode, reserved;
} SvtHipConvBlk;
/* The reference plane must be readable 3 samples left/above and 4 + 16-tile padding right/below of
 * every block (the reference's padded pictures are).  strides in pixels. */
int svt_hip_subpel_predict_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_ref, int ref_stride, void *d_dst,
                                     int dst_stride, const SvtHipConvBlk *d_blks, int nblk);
/* The job list of the sub-pel stage straight from the open-loop ME table, on the device: one mode-0 SvtHipConvBlk (EIGHTTAP_REGULAR both ways) per
 * whole 16x16 luma block of a w x h picture, in raster order -- (w / 16) * (h / 16) entries -- whose integer position is the block's position plus the
 * full-pel vector of its 16x16 PU in d_best_mv (the [n_sb][85] MV table of svt_hip_me_fullpel_frame_dev: EbMeTierZeroPu order, 16x16 PUs at 5 + the
 * z-order index inside the superblock), and whose q4 phases are d_frac_q4[2 * k], [2 * k + 1] (NULL: 0).  This is how md_subpel_search starts: the
 * sub-pel refinement of a block begins at its open-loop ME vector (EbProductCodingLoop.c:2063-2160). */
int svt_hip_subpel_jobs_from_me_dev(SvtHipCtx *ctx, const uint32_t *d_best_mv, int sb_cols, int w, int h, const uint8_t *d_frac_q4, SvtHipConvBlk *d_blks);

typedef struct {
    int32_t a_x, a_y, b_x, b_y;
    uint16_t w, h;
} SvtHipBlkPair;
/* svt_nxm_sad_kernel / svt_aom_sad{W}x{H} / sad_16b_kernel (aom_dsp_rtcd.h:334-336, :644, :651) for a list
 * of block pairs.  svt_aom_sad{W}x{H}x4d (:267-330) = four pairs that share the a block. */
int svt_hip_block_sad_batch_dev(SvtHipCtx *ctx, int pix_bytes, const void *d_a, int a_stride, const void *d_b, int b_stride,
                                const SvtHipBlkPair *d_pairs, int n, uint32_t *d_sad);
/* svt_aom_variance{W}x{H} (8-bit) / svt_aom_highbd_10_variance{W}x{H} (aom_dsp_rtcd.h:524, :568); pix_bytes 2 with bd = 16 selects the rule of
 * variance_highbd (aom_dsp_rtcd.h:653; EbComputeVariance_C.c:34: 32-bit sums, no bit-depth scaling).  svt_aom_mse16x16 (:248,
 * Encoder/Codec/EbPsnr.c:84) is the 16x16 case: return value = d_var, *sse = d_sse; svt_aom_highbd_8_mse16x16 (:263) is the plain
 * 16-bit SSE of svt_hip_block_sse_batch_dev. */
int svt_hip_block_variance_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_a, int a_stride, const void *d_b,
                                     int b_stride, const SvtHipBlkPair *d_pairs, int n, uint32_t *d_var, uint32_t *d_sse);

/* Coefficient-domain distortion of a list of transform blocks laid out like the outputs of svt_hip_fwd_txfm_quant_batch_dev
 * (n_per_block int32 per block, block after block):  d_out[blk][0] = sum (coeff - recon_coeff)^2, [1] = sum coeff^2, [2] = sum |coeff|.
 * Replaces svt_full_distortion_kernel32_bits (common_dsp_rtcd.h; Common/Codec/EbPictureOperators.c:156; [0] = DIST_CALC_RESIDUAL,
 * [1] = DIST_CALC_PREDICTION), svt_full_distortion_kernel_cbf_zero32_bits (:212; pass d_recon_coeff = NULL: [0] = [1]),
 * svt_av1_block_error (aom_dsp_rtcd.h, common_dsp_rtcd.c:56: returns [0], *ssz = [1]) and svt_aom_satd (:47: [2]). */
int svt_hip_coeff_distortion_batch_dev(SvtHipCtx *ctx, const int32_t *d_coeff, const int32_t *d_recon_coeff, int n_per_block,
                                       int nblk, uint64_t *d_out);
/* svt_aom_sse / svt_aom_highbd_sse (aom_dsp_rtcd.h:93-94) and svt_spatial_full_distortion_kernel / svt_full_distortion_kernel16_bits
 * (common_dsp_rtcd.h) for a list of block pairs: d_sse[n] = sum (a - b)^2. */
int svt_hip_block_sse_batch_dev(SvtHipCtx *ctx, int pix_bytes, const void *d_a, int a_stride, const void *d_b, int b_stride,
                                const SvtHipBlkPair *d_pairs, int n, uint64_t *d_sse);

/* ------------------------------------------------------- HME pyramids, variance pyramid, HME search */
/* decimation_2d / downsample_2d (Encoder/Codec/EbPictureAnalysisProcess.c:193,223): step 2 or 4,
 * filtered = 0 point-decimate, 1 = 2x2 box (a+b+c+d+2)>>2.  Output (w/step) x (h/step). */
int svt_hip_downsample_2d_dev(SvtHipCtx *ctx, const uint8_t *d_in, int in_stride, int w, int h, uint8_t *d_out, int out_stride,
                              int step, int filtered);
/* compute_block_mean_compute_variance (EbPictureAnalysisProcess.c:1005) for every 64x64 SB of a luma
 * plane whose (0,0) is 8-byte aligned with an 8-byte-multiple stride and at least 64 rows/cols of
 * padding past the last SB (the reference's padded input picture).  Replaces
 * svt_compute_interm_var_four8x8 / svt_compute_sub_mean_8x8 / svt_compute_mean_square_values_8x8
 * (aom_dsp_rtcd.h:650).  Outputs [n_sb][85]: [0] 64x64, [1..4] 32x32, [5..20] 16x16, [21..84] 8x8, each
 * level in raster order (pcs->y_mean / pcs->variance).  full_precision = BLOCK_MEAN_PREC_FULL. */
int svt_hip_variance_pyramid_dev(SvtHipCtx *ctx, const uint8_t *d_plane, int stride, int sb_cols, int n_sb,
                                 int full_precision, uint8_t *d_mean, uint16_t *d_var);
/* One exhaustive block search = one svt_sad_loop_kernel call (aom_dsp_rtcd.h:597) as issued by
 * hme_level_0/1/2 (Encoder/Codec/EbMotionEstimation.c:998,1146,1291).  row_step 2 reproduces the
 * "sub-SAD" calling convention (strides doubled, block height halved; the caller doubles the SAD). */
typedef struct {
    int32_t src_x, src_y; /* block position in the (decimated) source plane */
    int32_t ref_x, ref_y; /* position of the first candidate in the (decimated) reference plane */
    int16_t bw, bh;       /* block size, <= 64 x 64 */
    int16_t sa_w, sa_h;   /* search area */
    int16_t row_step, reserved;
} SvtHipSadLoop;
/* d_best_sad[n] (0xffffff when no candidate), d_best_xy[n][2] = (x_search_center, y_search_center);
 * first minimum in raster order, like the C kernel.  Entries are untouched when no candidate wins. */
int svt_hip_sad_loop_batch_dev(SvtHipCtx *ctx, const uint8_t *d_src, int src_stride, const uint8_t *d_ref, int ref_stride,
                               const SvtHipSadLoop *d_searches, int n, uint32_t *d_best_sad, int16_t *d_best_xy);
/* The same search on 16-bit planes (high-bit-depth path): sad_16b_kernel (aom_dsp_rtcd.h:651; Encoder/C_DEFAULT/EbComputeSAD_C.c:39) over the window,
 * candidate order / update rule of svt_sad_loop_kernel.  Block sizes up to 64 x 64; strides in samples. */
int svt_hip_sad_loop16_batch_dev(SvtHipCtx *ctx, const uint16_t *d_src, int src_stride, const uint16_t *d_ref, int ref_stride,
                                 const SvtHipSadLoop *d_searches, int n, uint32_t *d_best_sad, int16_t *d_best_xy);

/* ------------------------------------------------------------------ self-guided restoration ------ */
/* All three calls work on ONE plane that has been extended by >= 3 samples on every side
 * (svt_extend_frame, Common/Codec/EbRestoration.c:253); d_* pointers address sample (0,0); strides
 * in samples.  Restoration units are unit_size x unit_size (a multiple of 64) with the last row /
 * column of units absorbing the remainder, i.e. units_x = max((pw + unit_size/2) / unit_size, 1)
 * (av1 loop-restoration unit rule, EbRestoration.c:1413-1515); unit ROWS start RESTORATION_UNIT_OFFSET >> ss_y
 * (8 luma / 4 chroma rows) above their nominal position (foreach_rest_unit_in_tile, :1388-1391), so ss_y
 * (0 luma, 1 4:2:0 chroma) is part of every frame-level call.
 *
 * svt_hip_sgr_filter_plane_dev: svt_av1_selfguided_restoration (common_dsp_rtcd.h:191) for every
 *   processing unit of the plane and one parameter set `ep` (0..15): d_flt0 / d_flt1 int32 planes
 *   (flt_stride), written only for the radii the set uses.
 * svt_hip_sgr_search_plane_dev: the per-(unit, ep) sums svt_get_proj_subspace accumulates
 *   (Encoder/Codec/EbRestorationPick.c:448-496, units as search_selfguided_restoration :583 sees them)
 *   for every ep in ep_mask, without materialising flt0 / flt1: d_sums[unit][16][5] += {H00, H01, H11,
 *   C0, C1} (exact integers; zero the buffer first; divide by the unit's pixel count and solve the 2x2
 *   system on the host, :497-538).
 * svt_hip_sgr_apply_plane_dev: svt_av1_loop_restoration_filter_frame for the SGRPROJ units of a plane
 *   (EbRestoration.c:1293 -> svt_av1_loop_restoration_filter_unit :1162 -> sgrproj_filter_stripe :1086 ->
 *   svt_apply_selfguided_restoration, common_dsp_rtcd.h:187) with a per-unit parameter set
 *   d_unit_ep[unit] (255 = RESTORE_NONE: the unit is copied) and d_unit_xqd[unit][2].
 *   d_dbl != NULL gives the normative stripe handling: the 3 context rows above / below every
 *   (64 >> ss_y)-row stripe are taken from the DEBLOCKED (pre-CDEF) plane d_dbl exactly as
 *   svt_av1_loop_restoration_save_boundary_lines (:1843) + setup_processing_stripe_boundary (:353-453)
 *   arrange it (2 saved rows stretched to 3, edge-replicated); the GPU keeps that plane resident, so no
 *   line buffers are copied.  d_dbl == NULL filters the extended plane as is (the search's view). */
int svt_hip_sgr_filter_plane_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_plane, int stride, int pw, int ph, int ep,
                                 int32_t *d_flt0, int32_t *d_flt1, int flt_stride);
int svt_hip_sgr_search_plane_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_dgd, int stride, const void *d_src,
                                 int src_stride, int pw, int ph, int unit_size, int ss_y, uint32_t ep_mask, int64_t *d_sums);
int svt_hip_sgr_apply_plane_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_dgd, int stride, void *d_dst, int dst_stride,
                                int pw, int ph, int unit_size, int ss_y, const void *d_dbl, int dbl_stride,
                                const uint8_t *d_unit_ep, const int32_t *d_unit_xqd);
/* get_pixel_proj_error (Encoder/Codec/EbRestorationPick.c:317-351: svt_decode_xq + svt_av1_lowbd_pixel_proj_error /
 * svt_av1_highbd_pixel_proj_error, aom_dsp_rtcd.h) for every restoration unit of a plane, every parameter set in ep_mask and ncand
 * (1..SVT_HIP_SGR_MAX_CAND) xqd pairs (inside the tap range: xqd[0] in [-96, 31], xqd[1] in [-32, 95], EbRestoration.h:100-103) per (unit, set):
 * d_xqd[unit][16][ncand][2] -> d_err[unit][16][ncand] (cleared by the call;
 * entries of sets outside ep_mask stay 0; a candidate with xqd[0] == INT32_MIN ends the list of that (unit, set) early — as the first
 * candidate it skips the pair; the errors of the unused slots stay 0).
 * The filters are recomputed on chip, flt0 / flt1 never reach memory. */
#define SVT_HIP_SGR_MAX_CAND 24
int svt_hip_sgr_proj_error_plane_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_dgd, int stride, const void *d_src,
                                     int src_stride, int pw, int ph, int unit_size, int ss_y, uint32_t ep_mask, int ncand,
                                     const int32_t *d_xqd, int64_t *d_err);
/* search_selfguided_restoration (EbRestorationPick.c:583-671) for every restoration unit of a plane and every parameter set in
 * ep_mask (the reference's [start_ep, end_ep) window around the reference frames' sets, :596-607, is the caller's mask), ENTIRELY ON THE DEVICE:
 * the projection sums, svt_get_proj_subspace's 2x2 solve in IEEE double (:497-538), encode_xq (:539) and the coordinate descent of
 * finer_search_pixel_proj_error (:353-446, start step 2) — one workgroup per (unit, set) replays the reference's walk on exactly evaluated
 * errors (speculating ahead on the quadratic model of the five sums; a misprediction costs another pass over the unit, never exactness) — and the
 * unit's best set.  A fixed sequence of launches (sums + difference planes, then replay / evaluate rounds: walks that are done return at once), no host
 * synchronisation; stream-ordered like every _dev call.
 *   d_xqd [units][16][2], d_err [units][16] (entries of sets outside the mask are not written),
 *   d_best_ep [units] (may be NULL) = the first set with the smallest error, d_best_xqd [units][2] (may be NULL) = its xqd: exactly the
 *   d_unit_ep / d_unit_xqd arrays svt_hip_sgr_apply_plane_dev takes, so search -> trial filter -> SSE chains on the device.
 *   d_scratch: svt_hip_sgr_search_units_scratch_bytes(pw, ph, unit_size) bytes, 16-byte aligned, private to this call until it has completed
 *   (sums, per-walk state, 16 planes of (flt0 - u, flt1 - u) int16 pairs, one of dat - src).  Its first three uint32 receive diagnostics of the call:
 *   evaluation passes and evaluated points summed over all (unit, set) walks, and the number of walks that did not finish within the launched rounds (a
 *   failure: their error entry is -1; never observed). */
size_t svt_hip_sgr_search_units_scratch_bytes(int pw, int ph, int unit_size);
int svt_hip_sgr_search_units_plane_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_dgd, int stride, const void *d_src, int src_stride, int pw,
                                       int ph, int unit_size, int ss_y, uint32_t ep_mask, int32_t *d_xqd, int64_t *d_err, uint8_t *d_best_ep,
                                       int32_t *d_best_xqd, void *d_scratch, size_t scratch_bytes);
/* The same for all planes of a picture in one call: one sums / difference-plane launch per plane, then ONE walk launch over every
 * (plane, unit, set) — the long walks of one plane overlap the other planes' work instead of ending a launch each. */
typedef struct {
    const void *d_dgd; int32_t stride;      /* (0,0) of the 3-sample-extended CDEF output */
    const void *d_src; int32_t src_stride;
    int32_t pw, ph, unit_size, ss_y;
    uint32_t ep_mask;
    int32_t *d_xqd;       /* device [units][16][2] */
    int64_t *d_err;       /* device [units][16] */
    uint8_t *d_best_ep;   /* device [units] or NULL */
    int32_t *d_best_xqd;  /* device [units][2] or NULL */
    void *d_scratch; size_t scratch_bytes;   /* svt_hip_sgr_search_units_scratch_bytes(pw, ph, unit_size) */
} SvtHipSgrUnitsPlaneDev;
/* n_planes <= SVT_HIP_SGR_MAX_PLANES: the planes of up to FOUR pictures (same pixel type and bit depth) may share the two launches -- `planes` is then the
 * pictures' planes one after the other; every plane brings its own scratch and outputs, so the pictures stay independent. */
#define SVT_HIP_SGR_MAX_PLANES 12
int svt_hip_sgr_search_units_picture_dev(SvtHipCtx *ctx, int pix_bytes, int bd, int n_planes, const SvtHipSgrUnitsPlaneDev *planes);
/* HOST-output convenience form on library-owned device scratch: xqd_out[unit][16][2], err_out[unit][16] (sets outside the mask untouched),
 * best_ep[unit] (may be NULL); *rounds_out (may be NULL) is always 0 (kept from the host-driven search of earlier versions).  Synchronous: one
 * stream synchronisation at the end to hand the results over. */
int svt_hip_sgr_search_units_plane(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_dgd, int stride, const void *d_src, int src_stride,
                                   int pw, int ph, int unit_size, int ss_y, uint32_t ep_mask, int32_t *xqd_out, int64_t *err_out,
                                   uint8_t *best_ep, int *rounds_out);
/* The same for up to three planes of a picture (all launches first, then one hand-over per plane). */
typedef struct {
    const void *d_dgd; int32_t stride;      /* extended CDEF output plane, sample (0,0) */
    const void *d_src; int32_t src_stride;  /* source plane */
    int32_t pw, ph, unit_size, ss_y;
    uint32_t ep_mask;
    int32_t *xqd_out;   /* HOST [units][16][2] */
    int64_t *err_out;   /* HOST [units][16] */
    uint8_t *best_ep;   /* HOST [units] or NULL */
} SvtHipSgrSearchPlane;
int svt_hip_sgr_search_units_picture(SvtHipCtx *ctx, int pix_bytes, int bd, int n_planes, const SvtHipSgrSearchPlane *planes, int *rounds_out);
/* The same frame pass with Wiener units as well (svt_av1_loop_restoration_filter_frame for all three restoration types):
 * d_unit_ep[unit] = 254 selects RESTORE_WIENER with the taps d_unit_wiener[unit][0][8] (WienerInfo::vfilter) / [unit][1][8]
 * (hfilter); wiener_filter_stripe[_highbd] -> svt_av1_[highbd_]wiener_convolve_add_src (common_dsp_rtcd.h:179-185,
 * Common/Codec/convolve.c:105,207; round_0 = 3, round_1 = 11) with the same stripe-boundary rules as the self-guided units. */
int svt_hip_lr_apply_plane_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_dgd, int stride, void *d_dst, int dst_stride,
                               int pw, int ph, int unit_size, int ss_y, const void *d_dbl, int dbl_stride, const uint8_t *d_unit_ep,
                               const int32_t *d_unit_xqd, const int16_t *d_unit_wiener);
/* try_restoration_unit_seg (Encoder/Codec/EbRestorationPick.c:137-172): ONE restoration unit (index `unit` of the plane's unit grid) filtered with the
 * type / parameters its entries of d_unit_ep / d_unit_xqd / d_unit_wiener hold — same rules, stripe handling and arguments as
 * svt_hip_lr_apply_plane_dev, only the tiles of that unit are launched — and the unit's SSE against the source (sse_restoration_unit, :58) left in
 * *d_sse (device).  This is the probe of finer_tile_search_wiener_seg (:1092) and of search_sgrproj_seg's final check. */
int svt_hip_lr_try_unit_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_dgd, int stride, void *d_dst, int dst_stride, int pw, int ph,
                            int unit_size, int ss_y, const void *d_dbl, int dbl_stride, const uint8_t *d_unit_ep, const int32_t *d_unit_xqd,
                            const int16_t *d_unit_wiener, const void *d_src, int src_stride, int unit, uint64_t *d_sse);
/* The list form: the whole plane filtered with the per-unit entries (units that are not being probed hold 255 = RESTORE_NONE and are passed
 * through) and the SSE of every rectangle of d_rects (a = source plane coordinates, b = destination plane coordinates; normally one rectangle
 * per restoration unit) in d_sse[n_rects] — one round of a refinement that walks all units of a plane in lockstep
 * (finer_tile_search_wiener_seg, EbRestorationPick.c:1092, for every unit at once). */
int svt_hip_lr_try_units_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_dgd, int stride, void *d_dst, int dst_stride, int pw, int ph,
                             int unit_size, int ss_y, const void *d_dbl, int dbl_stride, const uint8_t *d_unit_ep, const int32_t *d_unit_xqd,
                             const int16_t *d_unit_wiener, const void *d_src, int src_stride, const SvtHipBlkPair *d_rects, int n_rects,
                             uint64_t *d_sse);
/* finer_tile_search_wiener_seg (Encoder/Codec/EbRestorationPick.c:1092-1200) of EVERY restoration unit of a plane in one launch: for each unit u with d_active[u] != 0 the
 * taps d_unit_wiener[u] (16 int16: vertical [0..7], horizontal [8..15], as svt_hip_lr_apply_plane_dev reads them) are refined by the reference's coordinate descent —
 * step sizes 4 / 2 / 1, horizontal then vertical taps, a downward then an upward probe per tap, a probe accepted iff its error is not larger — every probe being
 * try_restoration_unit_seg (:137): the unit filtered with the probed taps (stripe context rows from d_dbl, the deblocked picture) and its squared error against the
 * source.  The walk and every probe stay on the device; d_unit_wiener[u] receives the refined taps, d_err[u] their error, d_probes[u] (may be NULL) the number of
 * probes.  wiener_win: 7 / 5 / 3 (WIENER_WIN, _CHROMA, _3TAP: the outer taps of a shorter window are never probed).  Inactive units are left alone. */
int svt_hip_wiener_walk_units_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_dgd, int stride, int pw, int ph, int unit_size, int ss_y, const void *d_dbl, int dbl_stride,
                                  const void *d_src, int src_stride, int16_t *d_unit_wiener, const uint8_t *d_active, int wiener_win, int64_t *d_err, uint32_t *d_probes);
/* ... and of all planes of a picture in ONE launch (the fields are svt_hip_wiener_walk_units_dev's arguments): a unit's walk is a serial chain of ~30 probes on one
 * compute unit, so a launch takes as long as its longest walk whatever the number of units -- three planes side by side take a third of three launches
 * (search_wiener_seg's loop over the planes, EbRestProcess.c:527 -> EbRestorationPick.c:1552).  1 <= n_planes <= 3. */
typedef struct SvtHipWienerWalkPlane {
    const void *d_dgd; int stride, pw, ph, unit_size, ss_y;
    const void *d_dbl; int dbl_stride;
    const void *d_src; int src_stride;
    int16_t *d_unit_wiener; const uint8_t *d_active; int wiener_win;
    int64_t *d_err; uint32_t *d_probes;
} SvtHipWienerWalkPlane;
int svt_hip_wiener_walk_units_picture_dev(SvtHipCtx *ctx, int pix_bytes, int bd, int n_planes, const SvtHipWienerWalkPlane *planes);

/* ------------------------------------------------------------------ Wiener restoration search ---- */
/* svt_av1_compute_stats (aom_dsp_rtcd.h:99; Encoder/Codec/EbRestorationPick.c:704) for every restoration unit of a plane, as
 * search_wiener_seg (:1347) calls it: d_M[unit][win * win], d_H[unit][win^2 * win^2] (exact int64; feature index = (dx + win/2) * win
 * + (dy + win/2)).  win = 7 (luma), 5 (chroma) or 3.  The plane must be extended by 3 samples like for the self-guided calls.  The linear
 * solve / tap quantisation (wiener_decompose_sep_sym, finalize_sym_filter, compute_score: :800-1090): svt_hip_wiener_init_units_dev below, or the host.  8-bit planes, and
 * 16-bit planes (bd 8 / 10 / 12) = svt_av1_compute_stats_highbd (:741) incl. its bit_depth_divider; the 16-bit path keeps a library-owned
 * device scratch buffer inside the context (allocated on first use — growing it waits for the whole device —, freed by svt_hip_destroy): calls
 * of the 16-bit path through ONE context must not overlap on different streams (use one context per stream for that). */
int svt_hip_wiener_stats_plane_dev(SvtHipCtx *ctx, int pix_bytes, int bd, int win, const void *d_dgd, int stride, const void *d_src,
                                   int src_stride, int pw, int ph, int unit_size, int ss_y, int64_t *d_M, int64_t *d_H);

/* search_wiener_seg between the statistics and the tap refinement (EbRestorationPick.c:1388-1407), for every unit of a plane in one launch: wiener_decompose_sep_sym
 * (:946; its linear systems :800-944), finalize_sym_filter (:1022) and compute_score (:980) on d_M / d_H as svt_hip_wiener_stats_plane_dev left them — the statistics
 * never leave the device.  Per unit u: d_status[u] = 1 (the initial filter beats the identity filter by the model: refine it) or 2 (it does not: no Wiener filter for
 * the unit), d_active[u] = (status == 1), d_unit_wiener[16 u ..] = vfilter[8], hfilter[8] (InterpKernel layout) — the inputs of svt_hip_wiener_walk_units*_dev.
 * All 64-bit integer arithmetic: identical to the host code.  win = 7 / 5 / 3. */
int svt_hip_wiener_init_units_dev(SvtHipCtx *ctx, int win, int n_units, const int64_t *d_M, const int64_t *d_H, int16_t *d_unit_wiener, uint8_t *d_active,
                                  int8_t *d_status);

/* ------------------------------------------------------------------ alt-ref temporal filtering ---- */
#define SVT_HIP_TF_MAX_REFS 16
/* MeContext's TF fields of one 64x64 block after tf_32x32_sub_pel_search / tf_16x16_sub_pel_search / derive_tf_32x32_block_split_flag
 * (Encoder/Codec/EbMotionEstimationContext.h:447-454): tf_16x16_mv_x/y, tf_16x16_block_error, tf_32x32_mv_x/y, tf_32x32_block_error,
 * tf_32x32_block_split_flag. */
typedef struct SvtHipTfBlk64 {
    int16_t  mv16_x[16], mv16_y[16];
    uint64_t err16[16];
    int16_t  mv32_x[4], mv32_y[4];
    uint64_t err32[4];
    int32_t  split[4];
} SvtHipTfBlk64;
/* One frame of the filtering window: the motion-compensated predictor PICTURE (tf_inter_prediction's output, Encoder/Codec/
 * EbTemporalFiltering.c:2294; here a full picture instead of a 64x64 block buffer) and the TF fields of every 64x64 block
 * (raster, (w / 64) per row), all in device memory.  blocks == NULL marks the central picture (pred is ignored). */
typedef struct SvtHipTfRef {
    const void *pred[3];
    int pred_stride[3];
    const SvtHipTfBlk64 *blocks;
} SvtHipTfRef;
/* The pixel side of produce_temporally_filtered_pic (Encoder/Codec/EbTemporalFiltering.c:2136-2412) for a whole picture and the whole
 * window in one launch: apply_filtering_central (:557), svt_av1_apply_temporal_filter_planewise(_hbd) (aom_dsp_rtcd.h:616-629; :643,
 * :829) for every other frame and 32x32 block, get_final_filtered_pixels (:1943).  refs is a HOST array of n_refs <=
 * SVT_HIP_TF_MAX_REFS entries in window order; d_dst may alias d_src (the reference filters the central picture in place).
 * w / h = the multiple-of-64 extents the reference walks (blk_cols * 64, blk_rows * 64: the planes must be readable / writable there,
 * as the reference's padded pictures are).  noise_levels / decay_control / min_frame_size as in the reference call (:2313-2320,
 * MeContext::min_frame_size).  d_sse[0] / [1] receive filtered_sse / filtered_sse_uv.  4:2:0, 4:2:2 and 4:4:4. */
int svt_hip_tf_filter_frame_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *const d_src[3], const int src_stride[3],
                                void *const d_dst[3], const int dst_stride[3], int w, int h, int ss_x, int ss_y, int tf_chroma,
                                const SvtHipTfRef *refs, int n_refs, const double noise_levels[3], int decay_control,
                                int min_frame_size, uint64_t *d_sse);
/* estimate_noise / estimate_noise_highbd (Encoder/Codec/EbTemporalFiltering.c:2414, :2451): d_out[0] = sum of the rounded |Laplacian|
 * over the smooth pixels, d_out[1] = their number; sigma = out[0] / (6 * out[1]) * SQRT_PI_BY_2, or -1 when out[1] < 16 (host side,
 * svt_hip_tf_noise_sigma). */
int svt_hip_tf_estimate_noise_dev(SvtHipCtx *ctx, const void *d_src, int pix_bytes, int bd, int width, int height, int stride,
                                  int64_t *d_out);
double svt_hip_tf_noise_sigma(int64_t sum, int64_t num);

/* One (64x64 block, window frame) pair of the temporal filter's sub-pel stage. */
typedef struct SvtHipTfSubpelBlk {
    int32_t  x, y;          /* luma position of the block in the picture (sb_origin_x / sb_origin_y of the reference's calls) */
    int32_t  dst_x, dst_y;  /* luma position of the block in the central / predictor planes handed to the call */
    int32_t  blk_index;     /* its entry of d_blocks */
    uint32_t mv32[4];       /* MeContext::p_best_mv32x32[0..3] after motion_estimate_sb: (y << 16) | x, quarter-pel (integer vectors) */
    uint32_t mv16[16];      /* MeContext::p_best_mv16x16[0..15], z-order like the ME table */
} SvtHipTfSubpelBlk;
/* tf_32x32_sub_pel_search, tf_16x16_sub_pel_search, derive_tf_32x32_block_split_flag and tf_inter_prediction
 * (Encoder/Codec/EbTemporalFiltering.c:1469, :1133, :284, :1768; call sites :2272-2315) for every listed (block, frame) pair of ONE reference
 * picture, in one launch: per 32x32 block the half / quarter / (tf_hp) eighth-pel rounds of nine candidates each — EIGHTTAP_REGULAR prediction
 * through av1_inter_prediction's single-reference path (clamp_mv_to_umv_border_sb against the mi_cols x mi_rows picture, Encoder/Codec/
 * EbEncInterPrediction.c:24, :3593) scored with svt_aom_variance{32x32,16x16} (8-bit) / variance_highbd (16-bit planes) against the central
 * picture, first strictly smaller distortion wins —, the 16x16 rounds of the 32x32 blocks whose error reaches `th16`
 * (MeContext::tf_block_32x32_16x16_th), the split decision, and the MULTITAP_SHARP prediction of luma and (tf_chroma, 4:2:0) chroma with the
 * chosen vectors.  d_src: the central picture's planes, d_pred: the predictor planes (both addressed with dst_x / dst_y), d_ref: the
 * reference picture's planes with the pointer at picture sample (0, 0) (padded like the reference's pictures: the search reads up to
 * 4 + 32 + 4 samples outside the picture; only the rows the vectors reach have to be resident).  d_blocks[blk_index] receives the block's
 * SvtHipTfBlk64, which svt_hip_tf_filter_frame_dev then reads together with d_pred: the predictors never leave the device.
 * 16x16 fields of 32x32 blocks that skipped the 16x16 rounds are written as 0 (the reference leaves the previous block's values there and
 * never reads them: split is 0). */
int svt_hip_tf_subpel_frame_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *const d_src[3], const int src_stride[3],
                                const void *const d_ref[3], const int ref_stride[3], void *const d_pred[3], const int pred_stride[3],
                                int mi_cols, int mi_rows, uint64_t th16, int tf_hp, int tf_chroma, const SvtHipTfSubpelBlk *d_jobs, int n_jobs,
                                SvtHipTfBlk64 *d_blocks);

/* ------------------------------------------------------------------ compound inter prediction ---- */
/* One two-reference block.  Both references are predicted like svt_av1_[highbd_]jnt_convolve_{2d_copy,x,y,2d} (common_dsp_rtcd.h:221-243;
 * Common/Codec/EbInterPrediction.c:552-741, :944-1143; round_0 = 3 (5 at 12 bits), round_1 = COMPOUND_ROUND1_BITS) and combined by `type`:
 *   0 COMPOUND_AVERAGE   (the do_average branch, use_jnt_comp_avg = 0)
 *   1 COMPOUND_DISTANCE  (use_jnt_comp_avg = 1 with fwd_offset / bck_offset, sum 16)
 *   2 COMPOUND_DIFFWTD   svt_av1_build_compound_diffwtd_mask_d16 (common_dsp_rtcd.h:115; mask_type 0 = DIFFWTD_38, 1 = DIFFWTD_38_INV); the
 *                        w x h segmentation mask is also stored at d_masks + mask_off (stride w) unless mask_off < 0 — chroma reuses it
 *   3 mask supplied      (wedge tables or a stored segmentation mask) at d_masks + mask_off, stride mask_stride; mask_sub = 1: the mask is at
 *                        twice the block's resolution in both directions (4:2:0 chroma under a luma mask)
 *   2, 3 blend with svt_aom_{lowbd,highbd}_blend_a64_d16_mask (Common/Codec/EbBlend_a64_mask.c:34, :110) as build_masked_compound_no_round does.
 * Kernel banks as in SvtHipConvBlk; one filter pair for both references (AV1 signals one interp_filters per block). */
typedef struct {
    int32_t src0_x, src0_y, src1_x, src1_y; /* integer position of the block's top-left sample in reference plane 0 / 1 */
    int32_t dst_x, dst_y;
    uint8_t w, h;                           /* 4..128 */
    uint8_t bank_x, bank_y;
    uint8_t subpel0_x, subpel0_y, subpel1_x, subpel1_y; /* q4 phases */
    uint8_t type, fwd_offset, bck_offset, mask_type;
    uint8_t mask_sub, reserved[3];
    int32_t mask_off, mask_stride;
} SvtHipCompBlk;
int svt_hip_compound_predict_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_ref0, int ref0_stride, const void *d_ref1,
                                       int ref1_stride, void *d_dst, int dst_stride, uint8_t *d_masks, const SvtHipCompBlk *d_blks,
                                       int nblk);

/* OBMC motion-search costs of a list of blocks: svt_aom_obmc_sad{W}x{H} (aom_dsp_rtcd.h:356-398), svt_aom_obmc_variance{W}x{H} and
 * svt_aom_obmc_sub_pixel_variance{W}x{H} (:399-...; Encoder/C_DEFAULT/sad_av1.c:18, variance.c:270-318).  d_wsrc / d_mask: the int32 arrays of
 * calc_target_weighted_pred, block i at + wm_off with stride w.  d_out[i] = {sad, sse, variance at (xoffset, yoffset) eighths; 0, 0 = the
 * plain variance}.  The predictor plane must be readable one sample right / below of every block.  8-bit (the reference has no 16-bit twin). */
typedef struct {
    int32_t pre_x, pre_y;
    uint8_t w, h, xoffset, yoffset;
    int32_t wm_off;
} SvtHipObmcBlk;
int svt_hip_obmc_cost_batch_dev(SvtHipCtx *ctx, const uint8_t *d_pre, int pre_stride, const int32_t *d_wsrc, const int32_t *d_mask,
                                const SvtHipObmcBlk *d_blks, int nblk, uint32_t *d_out);

/* OBMC in mode decision, the two stages around those costs (csrc/obmc_search.h, obmc_search.hip; docs/kernels/obmc.md).  8-bit only, as in the reference: its
 * high-bit-depth mode decision unpacks the neighbour predictions to 8 bits and reads the 8-bit source (precompute_obmc_data,
 * Encoder/Codec/EbEncInterPrediction.c:2495-2522), and single_motion_search is "8bit path only" (Encoder/Codec/EbModeDecision.c:2958).
 *
 * 1. The weighted target: calc_target_weighted_pred (EbEncInterPrediction.c:2376-2437) with its visitors calc_target_weighted_pred_above (:2196-2224) and _left
 *    (:2226-2256), for a list of blocks in one launch.  wsrc = 0, mask = 64; over the above segments, rows 0 .. (min(bh, 64) >> 1) - 1: wsrc = m1 * above, mask = m0;
 *    both * 64; over the left segments, columns 0 .. (min(bw, 64) >> 1) - 1: wsrc = (wsrc >> 6) * m0 + (left << 6) * m1, mask = (mask >> 6) * m0; then
 *    wsrc = src * 4096 - wsrc.  m0 = obmc_mask_N[position] (Common/Codec/EbInterPrediction.c:2233-2260, svt_av1_get_obmc_mask; the specification's Obmc_Mask_N),
 *    m1 = 64 - m0.
 *      bsize                : the reference's BlockSize; the 17 sizes with min(bw, bh) >= 8 (is_motion_variation_allowed_bsize)
 *      x, y                 : the block's top-left sample in the source luma plane; the block lies inside the plane
 *      n_above, above_rel[], above_len[] : 0 .. 4 segments in 4-sample units, what foreach_overlappable_nb_above (:918-958) hands its visitor (rel_mi_col,
 *                             nb_mi_width); ascending, not overlapping, inside the block.  n_above = 0: !up_available, or no overlappable neighbour
 *      n_left, left_rel[], left_len[]    : likewise for foreach_overlappable_nb_left (:960-996)
 *      above_off, above_stride, left_off, left_stride : the neighbour predictions in the 8-bit pool d_nbr, addressed as the reference's `above` / `left`
 *                             pointers: the sample of block column c, row r is d_nbr[off + r * stride + c].  Strides >= 0; only samples the passes read are checked
 *      wm_off               : where the block's bw * bh wsrc and mask values go, as SvtHipObmcBlk::wm_off.  Ranges of two jobs must not overlap
 *    jobs is HOST memory, checked before anything is launched and copied to the device by the call (stream-ordered).  Refused with SVT_HIP_ERR_BAD_ARG before the
 *    device is touched: a NULL where a pointer is needed, njobs < 0 or above 2^24, a size outside the 17, a block outside the plane, a segment list that is not
 *    ascending inside the block, a neighbour sample outside d_nbr, a wm_off range outside the arrays.
 *    svt_hip_obmc_neighbours_host fills the segment lists of a job from the per-4x4 sb_type and is_neighbor_overlappable flag of the n4_w positions above and the
 *    n4_h positions left of the block (index 0 = the block's first column / row; NULL = !up_available / !left_available): the mi_step == 1 pairing rule (back to
 *    the even position, the flag of the odd one, step 2), the cap of a step at 16 units (BLOCK_64X64), nb_max = max_neighbor_obmc[log2 of the side in units] and the
 *    cut at the picture's last column / row (mi_cols, mi_rows).  No device.  The neighbour predictions are plain single-reference predictions (the prediction entry
 *    points above); the geometry of av1_setup_build_prediction_by_above_pred stays with the caller.
 *
 * 2. The motion refinement: single_motion_search (EbModeDecision.c:2951-3036) for a list of jobs in one launch.  mv_limits from mi_row, mi_col, the size, mi_rows,
 *    mi_cols and AOM_INTERP_EXTEND, narrowed by svt_av1_set_mv_search_range(ref_mv) for the full-pel stage.  Full-pel: svt_av1_obmc_full_pixel_search
 *    (Encoder/Codec/av1me.c:836-855): mv >> 3, clamp_mv, obmc_refining_search_sad (:791-834: neighbours {-1,0} {0,-1} {0,1} {1,0}, is_mv_in, `sad < best` then
 *    `sad + mvsad_err_cost < best`, at most search_range = 8 steps), get_obmc_mvpred_var (:776-790).  Sub-pel: svt_av1_find_best_obmc_sub_pixel_tree_up (:1069-1254)
 *    with forced_stop 0, iters_per_step 2, USE_8_TAPS, round 3 (2 when !allow_hp), on the limits as they were before the narrowing: set_subpel_mv_search_range,
 *    upsampled_setup_obmc_center_error, per round the four axis probes, the diagonal chosen by cost_array[0] <= [1] / [2] <= [3], SECOND_LEVEL_CHECKS_BEST(1); the
 *    unsigned / int mix of besterr, cost_array and INT_MAX, the slots of probes outside the range, the strict < and distortion / sse1 following the winner are the
 *    reference's.  A probe is upsampled_obmc_pref_error (:973-1035) = svt_aom_upsampled_pred_c (Encoder/C_DEFAULT/variance.c:212-269, EIGHTTAP_REGULAR) +
 *    svt_aom_obmc_variance{W}x{H}_c (:270-299).  rate_mv = svt_av1_mv_bit_cost with MV_COST_WEIGHT (108).
 *      d_ref, ref_stride, width, height, pad_w, pad_h : the 8-bit reference luma plane; d_ref points at picture sample (0, 0), pad_w columns / pad_h rows of border
 *                             lie around the picture (svt_hip_generate_padding_dev makes them).  The block of a job is at (4 mi_col, 4 mi_row) (svt_av1_setup_pred_block)
 *      d_wsrc, d_mask, wm_samples : the arrays of stage 1; a mask value is 0 .. 4096
 *      d_mv_joint_cost, d_mv_comp_cost : as svt_hip_ibc_full_search_batch_dev takes them
 *      mv_*, ref_mv_*       : the candidate's vector and ref_mv in 1/8 sample, each inside -32768 .. 32767 (the reference's MV is two int16): with that, no
 *                             difference the walks cost leaves the tables (the limits keep a probe within 1023 samples of ref_mv)
 *    Result: status 0 = searched; full_row / full_col, refining, steps (moves of the refinement, 0 .. 8), bestsme of the full-pel stage; row / col (1/8 sample),
 *    besterr, distortion, sse, rate_mv of the sub-pel stage.  status 1 = the narrowed limits are empty (the reference's clamp_mv has no meaning there): every
 *    vector, steps, distortion, sse and rate_mv are 0 and refining, bestsme and besterr are INT32_MAX.
 *    jobs is HOST memory, as in stage 1.  Refused with SVT_HIP_ERR_BAD_ARG before the device is touched: a NULL where a pointer is needed, njobs < 0 or above 2^24, a
 *    size outside the 17, mi_row / mi_col outside the picture, a wm_off range outside the arrays, a vector component outside int16, negative sad_per_bit /
 *    error_per_bit, allow_hp outside 0 / 1, and a plane whose border does not cover every sample the walk COULD read under its limits: the limits themselves, one
 *    more whole sample, and the 8-tap filter's -3 .. +4 around the block.
 * Not covered: force_integer_mv, scaled references (use_scaled_rec_refs_if_needed), choose_best_av1_mv_pred after the search, the chroma side of the final OBMC
 * prediction, and a hook in the reference encoder.  Stream-ordered and asynchronous apart from the job upload. */
typedef struct {
    int32_t bsize, x, y;
    int32_t n_above, above_rel[4], above_len[4];
    int32_t n_left, left_rel[4], left_len[4];
    int32_t above_off, above_stride, left_off, left_stride;
    int32_t wm_off;
} SvtHipObmcTargetJob;
typedef struct {
    int32_t bsize, mi_row, mi_col, wm_off;
    int32_t mv_row, mv_col, ref_mv_row, ref_mv_col;
    int32_t sad_per_bit, error_per_bit, allow_hp;
} SvtHipObmcSearchJob;
typedef struct {
    int32_t  status;
    int32_t  full_row, full_col, refining, steps, bestsme;
    int32_t  row, col;
    uint32_t besterr;
    int32_t  distortion;
    uint32_t sse;
    int32_t  rate_mv;
} SvtHipObmcSearchResult;
int svt_hip_obmc_neighbours_host(const uint8_t *above_sb_type, const uint8_t *above_overlappable, const uint8_t *left_sb_type, const uint8_t *left_overlappable,
                                 int mi_rows, int mi_cols, int mi_row, int mi_col, int bsize, SvtHipObmcTargetJob *job);
int svt_hip_obmc_target_batch_dev(SvtHipCtx *ctx, const uint8_t *d_src, int src_stride, int width, int height, const uint8_t *d_nbr, int64_t nbr_samples,
                                  const SvtHipObmcTargetJob *jobs, int njobs, int32_t *d_wsrc, int32_t *d_mask, int64_t wm_samples);
int svt_hip_obmc_search_batch_dev(SvtHipCtx *ctx, const uint8_t *d_ref, int ref_stride, int width, int height, int pad_w, int pad_h, int mi_rows, int mi_cols,
                                  const int32_t *d_wsrc, const int32_t *d_mask, int64_t wm_samples, const int32_t *d_mv_joint_cost, const int32_t *d_mv_comp_cost,
                                  const SvtHipObmcSearchJob *jobs, int njobs, SvtHipObmcSearchResult *d_results);
/* the same two contracts on host pointers, serially, from csrc/obmc_search.h: no context */
int svt_hip_obmc_target_host(const uint8_t *src, int src_stride, int width, int height, const uint8_t *nbr, int64_t nbr_samples, const SvtHipObmcTargetJob *jobs,
                             int njobs, int32_t *wsrc, int32_t *mask, int64_t wm_samples);
int svt_hip_obmc_search_host(const uint8_t *ref, int ref_stride, int width, int height, int pad_w, int pad_h, int mi_rows, int mi_cols, const int32_t *wsrc,
                             const int32_t *mask, int64_t wm_samples, const int32_t *mv_joint_cost, const int32_t *mv_comp_cost, const SvtHipObmcSearchJob *jobs,
                             int njobs, SvtHipObmcSearchResult *results);

/* Warped (affine) prediction of a list of blocks of one plane: svt_av1_warp_affine / svt_av1_highbd_warp_affine (Common/Codec/EbWarpedMotion.c:577, :733),
 * the non-compound path of svt_warp_plane / svt_highbd_warp_plane.  mat = EbWarpedMotionParams::wmmat[0..5], alpha .. delta = its shear
 * parameters (svt_get_shear_params, :921, stays on the host); (p_col, p_row, p_width, p_height) = the block in the destination plane, any size
 * from 4 x 4 to 128 x 128: the block is predicted in 8 x 8 cells and the last cell of a row or column is cut to what the block leaves of it
 * (the reference's AOMMIN(4, p_col + p_width - j - 4)), which is how the 4-wide chroma block of an 8 x 8 luma block is predicted; width /
 * height / stride describe the reference plane, of any size from 1 x 1 (samples outside are clamped to its edges, as in the reference;
 * ss_x and ss_y are independent: 4:2:2 is ss_x = 1, ss_y = 0). */
typedef struct {
    int32_t mat[6];
    int16_t alpha, beta, gamma, delta;
    int32_t p_col, p_row;
    uint8_t p_width, p_height, reserved[2];
} SvtHipWarpBlk;
int svt_hip_warp_predict_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_ref, int width, int height, int stride, void *d_dst,
                                   int dst_stride, int ss_x, int ss_y, const SvtHipWarpBlk *d_blks, int nblk);
/* The is_compound branches of the same two functions (EbWarpedMotion.c:660-683, :812-835): do_average = 0 — the block's prediction from the FIRST
 * reference goes to the 16-bit compound buffer (ConvolveParams::dst) at cb_off with stride cb_stride, d_dst is not touched; do_average = 1 —
 * the prediction from the SECOND reference is averaged with the buffer ((a + b) >> 1, or (a * fwd_offset + b * bck_offset) >> 4 when
 * use_jnt_comp_avg) and written to d_dst as pixels.  round_0 / round_1 are the values av1 uses for compound prediction (3 or 5 at 12 bits / 7). */
typedef struct {
    SvtHipWarpBlk blk;
    int32_t cb_off, cb_stride;
    uint8_t do_average, use_jnt_comp_avg, fwd_offset, bck_offset;
} SvtHipWarpCompBlk;
int svt_hip_warp_compound_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_ref, int width, int height, int stride, void *d_dst,
                                    int dst_stride, int ss_x, int ss_y, uint16_t *d_convbuf, const SvtHipWarpCompBlk *d_blks, int nblk);

/* Pixel-domain mask blends of a list of blocks: svt_aom_[highbd_]blend_a64_mask (mode 0: 2-D mask at d_masks + mask_off with mask_stride, subw / subh = the
 * mask is at twice the block's resolution in that direction), _hmask (mode 1: one mask value per column) and _vmask (mode 2: per row)
 * (common_dsp_rtcd.h:75-90; Common/Codec/EbBlend_a64_mask.c:214-434) — the blends of OBMC (av1_build_obmc_inter_prediction with the
 * av1_get_obmc_mask tables), inter-intra and pixel-domain masked compound.  d_dst may alias d_src0 (same stride), like the reference. */
typedef struct {
    int32_t src0_x, src0_y, src1_x, src1_y, dst_x, dst_y;
    uint8_t w, h, mode, subw, subh, reserved[3];
    int32_t mask_off, mask_stride;
} SvtHipBlendBlk;
int svt_hip_blend_a64_batch_dev(SvtHipCtx *ctx, int pix_bytes, const void *d_src0, int src0_stride, const void *d_src1, int src1_stride, void *d_dst,
                                int dst_stride, const uint8_t *d_masks, const SvtHipBlendBlk *d_blks, int nblk);

/* ------------------------------------------------------------------ masked compound and inter-intra: choosing the mask ---- */
/* The wedge mask set of the AV1 specification (7.11.3.11 "Wedge mask process", Wedge_Codebook), generated by the library: what svt_av1_init_wedge_masks builds
 * (Common/Codec/EbInterPrediction.c:1550-1615 the codebooks and wedge_params_lookup, :1672-1734 the primary masks, :1737-1767 the sign flips, :1770-1809 the
 * contiguous copies) and av1_get_contiguous_soft_mask returns.  Nine block sizes have wedges (BlockSize 3 .. 9 = 8x8, 8x16, 16x8, 16x16, 16x32, 32x16, 32x32; 18 = 8x32;
 * 19 = 32x8), 16 indices x 2 signs of bw * bh bytes (stride bw) each, 100 352 bytes in all: for each size in BlockSize order, for each index, sign 0 then sign 1.
 *   svt_hip_wedge_mask_table_bytes : 100352
 *   svt_hip_wedge_mask_offset      : byte offset of a mask in the table; -1 for a size without wedges, a sign outside 0 / 1, an index outside 0 .. 15
 *   svt_hip_wedge_masks_host       : fills dst[100352]; no device
 *   svt_hip_wedge_masks_dev        : the context's device copy, built and uploaded by the first call that needs it and kept until svt_hip_destroy.  The pointer is
 *                                    valid as d_masks of svt_hip_compound_predict_batch_dev (type 3: mask_off = the offset, mask_stride = bw; that call only reads the
 *                                    table for type 3, so its non-const parameter may be given this pointer) and of svt_hip_blend_a64_batch_dev. */
size_t svt_hip_wedge_mask_table_bytes(void);
int svt_hip_wedge_mask_offset(int bsize, int sign, int index);
int svt_hip_wedge_masks_host(uint8_t *dst);
int svt_hip_wedge_masks_dev(SvtHipCtx *ctx, const uint8_t **d_masks);
/* The tables of model_rd_with_curvfit / av1_model_rd_curvfit (Encoder/Codec/EbEncInterPrediction.c:432-503): rate = interp_rgrid_curv[4][65], dist =
 * interp_dgrid_curv[2][65], bsize_cat = bsize_curvfit_model_cat_lookup[22] (each 0 .. 3).  They are the caller's data: the library holds no copy of its own.  Copied
 * to the context (host and device) before the call returns; may be set again.  A search call made before is refused. */
int svt_hip_set_rd_curvfit_grids(SvtHipCtx *ctx, const double *rate, const double *dist, const int32_t *bsize_cat);
/* The mask decisions of compound mode decision for a list of blocks, one launch: search_compound_diff_wedge -> pick_interinter_mask -> pick_wedge /
 * pick_interinter_seg (Encoder/Codec/EbEncInterPrediction.c:562-631, :700-756, with the residual1 / diff10 set-up of calc_pred_masked_compound, :6120-6162) and the
 * decision part of inter_intra_search (Encoder/Codec/EbModeDecision.c:387-475) with pick_interintra_wedge (:214-242) -> pick_wedge_fixed_sign
 * (EbEncInterPrediction.c:635-675).  The leaves are the C forms: svt_av1_wedge_compute_delta_squares_c (:517-521, saturating to int16),
 * svt_av1_wedge_sign_from_residuals_c (:554-560), svt_av1_wedge_sse_from_residuals_c (Common/Codec/EbInterPrediction.c:2141-2151, each term clamped to int16),
 * aom_sum_squares_i16, svt_av1_build_compound_diffwtd_mask[_highbd] (:78-175), combine_interintra[_highbd] over build_smooth_interintra_mask (:1823-1875),
 * svt_aom_[highbd_]sse, model_rd_for_sb_with_curvfit (EbEncInterPrediction.c:819-869, luma), model_rd_with_curvfit (:432-503) and RDCOST
 * (Encoder/Codec/EbRateDistortionCost.h:106).  svt_log2f(0) (log2f_32, Common/Codec/EbUtility.c:251), undefined in the reference's C, is 0 as its C build gives it (csrc/comp_search.h).
 *   kind 0  inter-inter wedge: p0 at pred0, p1 at pred1.  Decides wedge_index, wedge_sign, rd.  Candidates 0 .. 15 = the wedge indices.  The nine wedge sizes.
 *   kind 1  inter-inter diff-weighted: decides mask_type (0 DIFFWTD_38, 1 DIFFWTD_38_INV), rd.  Candidates 0, 1.  Every size with min(bw, bh) >= 8.
 *   kind 2  inter-intra: the intra predictions II_DC, II_V, II_H, II_SMOOTH back to back (bw * bh samples each) at pred0, the inter prediction at pred1.  Decides
 *           interintra_mode with rd (RDCOST of rate + inter_intra_mode_fac_bits), then interintra_wedge_index with rd_wedge on the winner's intra prediction, sign
 *           0, wedge_idx_fac_bits added to the rate.  Candidates 0 .. 3 = the modes, 4 .. 19 = the wedge indices.  The nine wedge sizes.
 * A strict `<` from INT64_MAX keeps the first minimum.  Fields a kind does not decide are -1 (indices, sign, type, mode) and 0 (rd values, reserved).
 *   d_src, src_stride, width, height : the source luma plane (pix_bytes 1 with bd 8; pix_bytes 2 with bd 8 or 10); every block lies inside it
 *   d_pred, pred_samples : the predictor pool, blocks stored with stride bw as the reference's pred0 / pred1 / intrapred_buf; offsets are in samples
 *   d_rates, nrates      : int32 rate tables; kind 2 reads 16 values at wedge_rate (wedge_idx_fac_bits[bsize]) and 4 at mode_rate
 *                          (inter_intra_mode_fac_bits[size_group]); may be NULL when nrates is 0
 *   jobs                 : HOST memory, checked before anything is launched and copied to the device by the call (stream-ordered)
 *   d_results            : njobs results
 *   d_cand               : NULL, or njobs * SVT_HIP_COMP_SEARCH_MAX_CANDS records, one per candidate evaluated; slots a kind does not use are {-1, 0, 0, 0, 0}
 * Refused with SVT_HIP_ERR_BAD_ARG before anything touches the device: a NULL where a pointer is needed, njobs < 0 or above 2^24, a sample format other than the three,
 * an unknown kind, a size the kind does not allow, a block outside the plane, a predictor or rate offset outside its array, quantizer outside 1 .. 32767, grids not
 * set.  Stream-ordered and asynchronous apart from the job upload. */
#define SVT_HIP_COMP_SEARCH_WEDGE 0
#define SVT_HIP_COMP_SEARCH_DIFFWTD 1
#define SVT_HIP_COMP_SEARCH_INTERINTRA 2
#define SVT_HIP_COMP_SEARCH_MAX_CANDS 20
typedef struct {
    int32_t  kind, bsize;          /* bsize: the reference's BlockSize (0 = 4x4 .. 21 = 64x16) */
    int32_t  x, y;                 /* the block's top-left sample in the source plane */
    int32_t  pred0, pred1;         /* sample offsets into d_pred */
    int32_t  quantizer;            /* y_dequant_q3[base_q_idx][1] of the depth in use */
    uint32_t full_lambda;          /* full_lambda_md of the depth in use */
    int32_t  wedge_rate, mode_rate; /* kind 2: offsets into d_rates */
} SvtHipCompSearchJob;
typedef struct {
    int32_t wedge_index, wedge_sign, mask_type, interintra_mode, interintra_wedge_index, reserved;
    int64_t rd, rd_wedge;
} SvtHipCompSearchResult;
typedef struct {
    int32_t sign, rate;            /* rate: as it enters RDCOST, the caller's rate included */
    int64_t sse, dist, rd;
} SvtHipCompSearchCand;
int svt_hip_compound_search_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_src, int src_stride, int width, int height, const void *d_pred,
                                      int64_t pred_samples, const int32_t *d_rates, int nrates, const SvtHipCompSearchJob *jobs, int njobs,
                                      SvtHipCompSearchResult *d_results, SvtHipCompSearchCand *d_cand);
/* the same on host pointers, serially, from csrc/comp_search.h: no context, the three tables of svt_hip_set_rd_curvfit_grids first */
int svt_hip_compound_search_host(const double *rate, const double *dist, const int32_t *bsize_cat, int pix_bytes, int bd, const void *src, int src_stride, int width,
                                 int height, const void *pred, int64_t pred_samples, const int32_t *rates, int nrates, const SvtHipCompSearchJob *jobs, int njobs,
                                 SvtHipCompSearchResult *results, SvtHipCompSearchCand *cand);

/* ------------------------------------------------------------------ the dual interpolation filter search of mode decision ---- */
/* interpolation_filter_search (Encoder/Codec/EbEncInterPrediction.c:3047-3297) for a list of blocks, one launch (csrc/ifs_search.h, ifs_search.hip;
 * docs/kernels/ifs.md).  The nine candidates are filter_sets[i] = {y filter, x filter} (:3034-3045; 0 EIGHTTAP_REGULAR, 1 EIGHTTAP_SMOOTH, 2 MULTITAP_SHARP), with
 * interp_filters = y | x << 16 (av1_make_interp_filters, Common/Codec/filter.h:59-67).  Per candidate, luma only as the reference (use_uv = EB_FALSE):
 *   prediction  type -1, one reference: what convolve[subpel_x != 0][subpel_y != 0][0] dispatches to, svt_av1_[highbd_]convolve_{2d_copy,x,y,2d}_sr
 *               (Common/Codec/EbInterPrediction.c:349-469, :744-866), i.e. svt_hip_subpel_predict_batch_dev mode 0 with the candidate's banks; type 0 COMPOUND_AVERAGE
 *               and 1 COMPOUND_DISTANCE, two references: the svt_av1_[highbd_]jnt_convolve_{2d_copy,x,y,2d} pair (:552-741, :944-1143) and the combination of
 *               svt_hip_compound_predict_batch_dev, one filter pair for both references.  A direction whose phase is 0 does not see its filter.
 *   sse         svt_spatial_full_distortion_kernel / svt_full_distortion_kernel16_bits against the source block (model_rd_for_sb, :2903-2996)
 *   rate, dist  model_rd_from_sse (:2877-2901) -> svt_av1_model_rd_from_var_lapndz (:2855-2875) -> model_rd_norm (:2795-2853) on
 *               ROUND_POWER_OF_TWO(sse, 2 * (bd - 8)), quantizer >> (bd - 5) and num_pels_log2_lookup[bsize]; dist <<= 4; rate += rate_tab[0][y] + rate_tab[1][x],
 *               the caller's six values of svt_av1_get_switchable_rate (:2760-2789: switchable_interp_fac_bitss[ctx of dir 0][y] and [ctx of dir 1][x])
 *   rd          RDCOST(full_lambda, rate, dist) as that file defines it (:2792-2793)
 * The decision: order 0, the interpolation_search_level && enable_dual_filter branch, ascending over all nine with a strict `<` (the first minimum wins; its second
 * loop cannot change the result, csrc/ifs_search.h); order 1, the else branch, descending from 8 to 0 with a strict `<` (among equals the highest index wins), with
 * dual = 0 over the pairs with equal filters only; it also gives ifs_is_regular_last (regular_last; -1 under order 0, which does not touch it).
 *   d_src, src_stride, width, height : the source luma plane (pix_bytes 1 with bd 8; pix_bytes 2 with bd 8 or 10); every block lies inside it
 *   d_ref0 / d_ref1 : the reference planes; ref*_x / ref*_y are the caller's integer positions, already clamped, as for the prediction calls.  EVERY reference block
 *                     is readable exactly 3 samples left and above and 4 samples right and below of it, whatever its phases; nothing further is read.  d_ref1
 *                     may be NULL when no job has two references
 *   d_dst           : NULL, or a plane that receives the winner's luma prediction of every job at (dst_x, dst_y): what svt_hip_subpel_predict_batch_dev /
 *                     svt_hip_compound_predict_batch_dev write with the winner's banks
 *                     The destination rectangle is NOT validated: (dst_x, dst_y) and dst_stride are the caller's, like the reference positions and strides, as for
 *                     the prediction calls; rectangles of one call must not overlap
 *   jobs            : HOST memory, checked before anything is launched and copied to the device by the call (stream-ordered)
 *   d_results       : njobs results
 *   d_cand          : NULL, or njobs * SVT_HIP_IFS_CANDS records; a pair that was not evaluated is {-1, 0, 0, 0}
 * Refused with SVT_HIP_ERR_BAD_ARG before anything touches the device: a NULL where a pointer is needed, a two-reference job without d_ref1, a size with a dimension
 * below 8 (17 sizes remain: the caller's cap is 4, so the 4-tap kernels are never reached), a block outside the source plane, a phase above 15, an unknown type or
 * order, offsets that do not sum to 16 for type 1, quantizer outside 1 .. 32767, a sample format other than the three, njobs < 0 or above 2^24.  Stream-ordered
 * and asynchronous apart from the job upload. */
#define SVT_HIP_IFS_CANDS 9
typedef struct {
    int32_t  bsize;                    /* the reference's BlockSize (3 = 8x8 .. 15 = 128x128, 18 .. 21) */
    int32_t  x, y;                     /* the block's top-left sample in the source plane */
    int32_t  ref0_x, ref0_y, ref1_x, ref1_y; /* integer position of the block's top-left sample in reference plane 0 / 1 */
    int32_t  subpel0_x, subpel0_y, subpel1_x, subpel1_y; /* q4 phases 0 .. 15 */
    int32_t  type;                     /* -1 one reference, 0 COMPOUND_AVERAGE, 1 COMPOUND_DISTANCE */
    int32_t  fwd_offset, bck_offset;   /* type 1: a row of quant_dist_lookup_table, sum 16 */
    int32_t  order, dual;              /* the branch of the decision; dual = enable_dual_filter (read under order 1) */
    int32_t  quantizer;                /* y_dequant_q3[base_q_idx][1] of the depth in use */
    uint32_t full_lambda;              /* full_lambda_md of the depth in use, >> 2 * (bd - 8) as the reference divides it */
    int32_t  rate_tab[2][3];           /* [0][y filter], [1][x filter] */
    int32_t  dst_x, dst_y;             /* where the winner's prediction goes in d_dst */
} SvtHipIfsJob;
typedef struct {
    int32_t  best;                     /* 0 .. 8 */
    uint32_t interp_filters;
    int32_t  switchable_rate;          /* what the reference adds to fast_luma_rate */
    int32_t  regular_last;
    int64_t  rd;
} SvtHipIfsResult;
typedef struct {
    int64_t rate, sse, dist, rd;       /* rate: as it enters RDCOST, the two filter symbols included; sse: before the depth rounding */
} SvtHipIfsCand;
int svt_hip_ifs_search_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_src, int src_stride, int width, int height, const void *d_ref0, int ref0_stride,
                                 const void *d_ref1, int ref1_stride, void *d_dst, int dst_stride, const SvtHipIfsJob *jobs, int njobs, SvtHipIfsResult *d_results,
                                 SvtHipIfsCand *d_cand);
/* the same on host pointers, serially, from csrc/ifs_search.h: no context */
int svt_hip_ifs_search_host(int pix_bytes, int bd, const void *src, int src_stride, int width, int height, const void *ref0, int ref0_stride, const void *ref1,
                            int ref1_stride, void *dst, int dst_stride, const SvtHipIfsJob *jobs, int njobs, SvtHipIfsResult *results, SvtHipIfsCand *cand);

/* ------------------------------------------------------------------ picture formats around the high-bit-depth path ---- */
/* The reference keeps 10-bit pictures as an 8-bit plane + a 2-bit plane; these are its conversions to / from the 16-bit samples the
 * kernels above take (Common/C_DEFAULT/EbPackUnPack_C.c):
 *   mode 0 svt_enc_msb_pack2_d        in0 = 8-bit plane, in1 = 2-bit plane (one byte per sample, bits on top)  -> out0 16-bit
 *   mode 1 svt_compressed_packmsb     in1 = 2-bit plane packed 4 samples per byte (stride in bytes), w % 4 == 0 -> out0 16-bit
 *   mode 2 svt_enc_msb_un_pack2_d     in0 16-bit -> out0 8-bit, out1 2-bit plane (may be NULL)
 *   mode 3 svt_convert_8bit_to_16bit, mode 4 svt_convert_16bit_to_8bit
 *   mode 5 svt_c_pack                 in0 = unpacked 2-bit plane -> out0 packed (stride in bytes), w % 4 == 0
 *   mode 6 svt_unpack_avg             in0, in1 16-bit -> out0 = rounded average of their 8-bit MSBs
 * Strides in samples of the respective plane. */
int svt_hip_picture_format_dev(SvtHipCtx *ctx, int mode, const void *d_in0, int in0_stride, const void *d_in1, int in1_stride, void *d_out0,
                               int out0_stride, void *d_out1, int out1_stride, int w, int h);

/* generate_padding / generate_padding16_bit (Common/Codec/EbMcp.c:112, :166) for a plane that is resident on the device: the border of pad_w columns /
 * pad_h rows around the w x h picture is filled with the nearest picture sample (what the motion search and the sub-pel kernels expect of a
 * reference picture, and svt_extend_frame's 3-sample border of the restoration input).  d_plane points at picture sample (0, 0). */
int svt_hip_generate_padding_dev(SvtHipCtx *ctx, void *d_plane, int pix_bytes, int stride, int w, int h, int pad_w, int pad_h);

/* ------------------------------------------------------------------ super-resolution: normative upscale and the scaler ---- */
/* A picture coded with super-resolution is encoded at width * 8 / denom (denom 9 .. 16) and brought back to full width between CDEF and the
 * restoration by the normative, horizontal-only 8-tap upscale (svt_av1_superres_upscale_frame, Encoder/Codec/EbRestProcess.c:397-452 ->
 * svt_av1_upscale_normative_rows, Common/Codec/EbSuperRes.c:40-294); the same upscale makes the restoration's stripe context rows from the deblocked
 * picture (save_deblock_boundary_lines, Common/Codec/EbRestoration.c:1645-1702: rows = 1 or 2).  On the source side the input picture and every
 * reference are scaled to the coded size by av1_resize_plane / av1_highbd_resize_plane (Encoder/Codec/EbResize.c:186-765).
 * Samples: pix_bytes 1 (bd 8) or 2 (bd 8 .. 12, a value).  Strides in samples, >= the plane's width.  Everything is out of place: d_src is only read.
 *
 * svt_hip_superres_scaled_dim = calculate_scaled_size_helper (8 <= denom <= 16, 8 returns dim; 1 <= dim <= 65535); 0 for anything else.
 * svt_hip_superres_upscale_params: the step and the first position, in 1/16384 sample, of an in_w -> out_w upscale (1 <= in_w <= out_w <= 16384):
 * output x is the 8 taps of phase ((x0_qn + x * x_step_qn) & 0x3fff) >> 8 over the source samples ((x0_qn + x * x_step_qn) >> 14) - 4 + k, k = 0 .. 7. */
int svt_hip_superres_scaled_dim(int dim, int denom);
int svt_hip_superres_upscale_params(int in_w, int out_w, int32_t *x_step_qn, int32_t *x0_qn);
/* One plane of an upscale: `rows` rows (1 .. 16384) of in_w samples -> out_w samples each. */
typedef struct {
    const void *d_src;
    int         src_stride, in_w;
    void       *d_dst;
    int         dst_stride, out_w;
    int         rows;
} SvtHipUpscalePlane;
/* 1 .. 3 planes in one launch.  Source positions outside [0, in_w) read the nearest sample of the row (the reference writes 5 replicated columns
 * either side of its input for the time of the call; this does not touch the source), and the result does not depend on the tile columns: no tile
 * information is taken (docs/kernels/superres.md).  Refused: out_w < in_w, in_w < 1, out_w > 16384, d_src == d_dst, a stride below the width. */
int svt_hip_superres_upscale_planes_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const SvtHipUpscalePlane *planes, int n_planes);
/* One plane of the general scaler: in_w x in_h -> out_w x out_h, any sizes 1 .. 16384 per axis, enlarging included; equal sizes copy. */
typedef struct {
    const void *d_src;
    int         src_stride, in_w, in_h;
    void       *d_dst;
    int         dst_stride, out_w, out_h;
} SvtHipResizePlane;
/* av1_resize_plane for 1 .. 3 planes: rows first, then columns, the plane in between clipped to samples.  d_scratch holds
 * svt_hip_resize_scratch_bytes(pix_bytes, planes, n_planes) bytes (0 when no plane changes its height; also 0 for what the call would refuse) and
 * may be NULL when that is 0. */
size_t svt_hip_resize_scratch_bytes(int pix_bytes, const SvtHipResizePlane *planes, int n_planes);
int svt_hip_resize_planes_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const SvtHipResizePlane *planes, int n_planes, void *d_scratch, size_t scratch_bytes);

/* ------------------------------------------------------------------ inter prediction from a reference of another size ---- */
/* Once a picture and one of its references differ in size (super-resolution, reference scaling) every inter block that predicts from that reference
 * goes through svt_av1_convolve_2d_scale / svt_av1_highbd_convolve_2d_scale (Common/Codec/EbInterPrediction.c:471-550, :867-946, called by
 * svt_inter_predictor / svt_highbd_inter_predictor, :1368-1500): the filter phase changes per output column and row, x_qn = subpel_x + x * xs in 1/1024
 * sample.  Positions and phases come from the scaled branch of compute_subpel_params (Encoder/Codec/EbEncInterPrediction.c:3591-3661), the scale factors
 * from svt_av1_setup_scale_factors_for_frame (EbInterPrediction.c:178-241).  The arithmetic is csrc/scaled_pred.h, the kernels csrc/scaled_pred.hip
 * (docs/kernels/scaled_pred.md). */
typedef struct {
    int32_t x_scale_fp, y_scale_fp; /* reference size / picture size in 1/16384; -1, -1 = not a valid pair (REF_INVALID_SCALE) */
    int32_t x_step_q4, y_step_q4;   /* the same in 1/1024: 64 .. 2048, 1024 = not scaled */
} SvtHipScaleFactors;
/* Host only.  other_* = the reference's size, this_* = the picture's.  Returns SVT_HIP_OK, or SVT_HIP_ERR_BAD_ARG with out->x_scale_fp = y_scale_fp = -1
 * (steps 0) for a pair valid_ref_frame_size refuses: 2 * this >= other and this <= 16 * other per axis (and every size 1 .. 65535). */
int svt_hip_scale_factors(int other_w, int other_h, int this_w, int this_h, SvtHipScaleFactors *out);
/* Host only: the scaled branch of compute_subpel_params for one plane of one block.  pre_x / pre_y = the block's position in that plane, mv_row / mv_col
 * in 1/8 luma sample, ss_x / ss_y the plane's sub-sampling, frame_w / frame_h the luma size the reference is clamped against.  Out: the integer position
 * in the reference plane (may be negative: the border), the phases 0 .. 1023 and the steps.  The branch is applied whatever the factors are; with both
 * 16384 it gives the position and the filter index of the unscaled branch for a vector clamp_mv_to_umv_border_sb leaves alone (phase = 64 * q4 + 32). */
void svt_hip_scaled_block_params(const SvtHipScaleFactors *sf, int pre_x, int pre_y, int mv_row, int mv_col, int ss_x, int ss_y, int frame_w, int frame_h,
                                 int32_t *pos_x, int32_t *pos_y, int32_t *subpel_x, int32_t *subpel_y, int32_t *xs, int32_t *ys);
/* One job of svt_hip_scaled_predict_batch_dev: position, phase and step per reference, raw.  compound 0 = one reference (reference 0; the *1 members are
 * not read), pixels as convolve_2d_scale writes them with is_compound = 0; 1 = the two references averaged (do_average, round_1 =
 * COMPOUND_ROUND1_BITS); 2 = distance-weighted ((d0 * fwd_offset + d1 * bck_offset) >> DIST_PRECISION_BITS, offsets of quant_dist_lookup_table).  The two
 * references of a pair may have different sizes, so each has its own steps; a reference with both steps 1024 is legal and gives what the reference's
 * unscaled dispatch (jnt_convolve_{2d,x,y,2d_copy}) gives at phase subpel >> 6.  Kernel banks as in SvtHipConvBlk.  A job with a step outside 1 .. 2048,
 * a phase above 1023 or a size outside 1 .. 128 writes nothing. */
typedef struct {
    int32_t pos0_x, pos0_y, pos1_x, pos1_y;                 /* integer position of the block's top-left sample in reference plane 0 / 1 */
    int32_t dst_x, dst_y;
    uint16_t subpel0_x, subpel0_y, subpel1_x, subpel1_y;    /* 0 .. 1023 */
    uint16_t xs0, ys0, xs1, ys1;                            /* 1/1024 sample per output sample */
    uint8_t w, h;                                           /* 4 .. 128 */
    uint8_t bank_x, bank_y;
    uint8_t compound, fwd_offset, bck_offset, reserved;
} SvtHipScaledBlk;
/* One block as the encoder holds it, for svt_hip_scaled_jobs_dev: everything of SvtHipScaledBlk that does not depend on the scale factors, and the
 * vectors (1/8 luma sample; mv1_* read when compound != 0). */
typedef struct {
    int32_t pre_x, pre_y; /* the block's position in the plane being predicted */
    int32_t dst_x, dst_y;
    int16_t mv0_row, mv0_col, mv1_row, mv1_col;
    uint8_t ss_x, ss_y;   /* the plane's sub-sampling, 0 / 1 */
    uint8_t w, h;
    uint8_t bank_x, bank_y;
    uint8_t compound, fwd_offset, bck_offset, reserved[3];
} SvtHipScaledRec;
/* d_jobs[i] = d_recs[i] through svt_hip_scaled_block_params, on the device: vectors that live there never visit the host.  sf0 / sf1 (host pointers) and
 * frame_w / frame_h [2] belong to reference 0 / 1; sf1 == NULL: reference 1 is reference 0's twin (same factors, same size).  Both must be valid. */
int svt_hip_scaled_jobs_dev(SvtHipCtx *ctx, const SvtHipScaleFactors *sf0, const SvtHipScaleFactors *sf1, const int frame_w[2], const int frame_h[2],
                            const SvtHipScaledRec *d_recs, SvtHipScaledBlk *d_jobs, int n);
/* The prediction of n jobs in one launch; (pix_bytes, bd) = (1, 8), (2, 8), (2, 10) or (2, 12).  d_ref1 may be NULL when no job is compound: the jobs are
 * device memory the host cannot see, so a compound job with d_ref1 == NULL is the caller's error and is not caught.  What the caller owes, for every job
 * and each reference it uses: the plane is readable from pos_x - 3 to pos_x + (((w - 1) * xs + subpel_x) >> 10) + 4 in x, and from pos_y - 3 to
 * pos_y + (((h - 1) * ys + subpel_y) >> 10) + 4 in y (the reference's 288-sample border guarantees it after the clamp of svt_hip_scaled_block_params), and
 * the destinations of a launch are disjoint.  Nothing outside a job's w x h destination is written.  strides in samples. */
int svt_hip_scaled_predict_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_ref0, int ref0_stride, const void *d_ref1, int ref1_stride,
                                     void *d_dst, int dst_stride, const SvtHipScaledBlk *d_jobs, int n);

/* ------------------------------------------------------------------ per-call forms ------------- */
/* Operations that the frame entry points above run fused inside larger kernels, exposed on their own for a list of units, so that every
 * pointer of the reference's dispatch table on this path has a device form (include/svt_hip_rtcd.h launches these with a list of one).
 * All pointers are device pointers; lists are device arrays. */

/* The quantizer stage alone: nblk blocks of n_coeffs coefficients each (packed, block after block), quantizer variants and parameters as in
 * SvtHipQuantParams (flat quant matrix), d_iscan = inverse scan of the transform size (eob = 1 + last scan position with a non-zero level).
 * Replaces svt_aom_quantize_b / svt_aom_highbd_quantize_b / svt_av1_quantize_fp[_32x32|_64x64] / svt_av1_highbd_quantize_fp
 * (aom_dsp_rtcd.h:250-262). */
int svt_hip_quantize_batch_dev(SvtHipCtx *ctx, const int32_t *d_coeff, int n_coeffs, int nblk, const SvtHipQuantParams *qp,
                               const int16_t *d_iscan, int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob);
/* residual = src - pred over a w x h area: svt_residual_kernel8bit / 16bit (common_dsp_rtcd.h:168, :180).  Strides in samples. */
int svt_hip_residual_dev(SvtHipCtx *ctx, int pix_bytes, const void *d_src, int src_stride, const void *d_pred, int pred_stride,
                         int16_t *d_residual, int residual_stride, int w, int h);
/* svt_ext_all_sad_calculation_8x8_16x16 (aom_dsp_rtcd.h:640; EbMotionEstimation.c:356): for each job the 64 8x8 and 16 16x16 SADs of a 64x64
 * source block against 8 horizontally consecutive candidates, and the running bests updated in candidate order.
 * d_state: 800 uint32 per job = best_sad8x8[64] best_sad16x16[16] best_mv8x8[64] best_mv16x16[16] (in/out) eight_sad16x16[16][8]
 * eight_sad8x8[64][8] (out), block indices in the reference's z-order. */
typedef struct { int32_t src_off, ref_off; uint32_t mv; int32_t sub_sad; } SvtHipExtSadJob;
int svt_hip_ext_all_sad_8x8_16x16_batch_dev(SvtHipCtx *ctx, const uint8_t *d_src, int src_stride, const uint8_t *d_ref, int ref_stride,
                                            const SvtHipExtSadJob *d_jobs, int n, uint32_t *d_state);
/* svt_ext_eight_sad_calculation_32x32_64x64 (aom_dsp_rtcd.h:641; EbMotionEstimation.c:394).  d_state: 170 uint32 per job =
 * sad16x16[16][8] (in) best_sad32x32[4] best_sad64x64 best_mv32x32[4] best_mv64x64 (in/out) sad32x32[4][8] (out); d_mv[n]. */
int svt_hip_ext_eight_sad_32x32_64x64_batch_dev(SvtHipCtx *ctx, const uint32_t *d_mv, int n, uint32_t *d_state);
/* svt_compute_interm_var_four8x8 (aom_dsp_rtcd.h:650; EbPictureAnalysisProcess.c:352): for each offset (top-left sample of four
 * horizontally adjacent 8x8 blocks) 4 means and 4 means of squares with the reference's fixed-point scaling. */
int svt_hip_interm_var_four8x8_batch_dev(SvtHipCtx *ctx, const uint8_t *d_plane, int stride, const int32_t *d_offs, int n,
                                         uint64_t *d_mean, uint64_t *d_mean_sq);
/* svt_handle_transform64x64 / 64x32 / 32x64 / 64x16 / 16x64 (aom_dsp_rtcd.h:221-230) in place on nblk blocks of W*H coefficients:
 * energy of the coefficients outside the top-left 32x32, zero them, pack the kept rows to stride min(W,32). tx_size = TxSize (4, 12, 11, 18, 17). */
int svt_hip_handle_transform64_batch_dev(SvtHipCtx *ctx, int tx_size, int32_t *d_coeff, int nblk, uint64_t *d_energy);
/* handle_transform64x64_N2_N4 / 64x32 / 32x64 / 64x16 / 16x64 (aom_dsp_rtcd.h:237-245; EbTransforms.c:2933-2969), the re-pack that follows the
 * N2 / N4 forward transforms: the kept rows move from stride 64 to stride 32 in place (nothing is zeroed, the energy is 0); blocks of W*H coefficients. */
int svt_hip_handle_transform64_n2n4_batch_dev(SvtHipCtx *ctx, int tx_size, int32_t *d_coeff, int nblk);
/* svt_aom_upsampled_pred (aom_dsp_rtcd.h:353; C_DEFAULT/variance.c:212): sub-pel prediction of the OBMC / sub-pel refinement searches, two
 * 8-tap passes with an 8-bit clip after each.  bank = filter family as in SvtHipConvBlk (3 bilinear = USE_2_TAPS, 4 = USE_4_TAPS, 0 = USE_8_TAPS).
 * Output is packed (stride = w) at dst_off. */
typedef struct { int32_t ref_off, dst_off; uint8_t w, h, subpel_x_q3, subpel_y_q3, bank, reserved[3]; } SvtHipUpsampledBlk;
int svt_hip_upsampled_pred_batch_dev(SvtHipCtx *ctx, const uint8_t *d_ref, int ref_stride, uint8_t *d_dst, const SvtHipUpsampledBlk *d_blks, int n);
/* ONE reference of a compound prediction, the form the reference's pointers have: svt_av1_[highbd_]jnt_convolve_{2d, x, y, 2d_copy} (variant 0..3;
 * common_dsp_rtcd.h:211-243; Common/Codec/EbInterPrediction.c:552-741, :868-1143).  do_average = 0: the 16-bit result goes to d_convbuf
 * (ConvolveParams::dst), d_dst is not touched; do_average = 1: it is combined with d_convbuf (plain average, or fwd_offset / bck_offset when
 * use_jnt_comp_avg) and written to d_dst as pixels.  d_taps[16] = the horizontal and the vertical 8-tap kernel of the block's phases; d_src needs 3
 * samples of context before and 4 after in the filtered directions.  (svt_hip_compound_predict_batch_dev is the fused two-reference form.) */
int svt_hip_jnt_convolve_dev(SvtHipCtx *ctx, int pix_bytes, int bd, int variant, const void *d_src, int src_stride, void *d_dst, int dst_stride,
                             uint16_t *d_convbuf, int convbuf_stride, const int16_t *d_taps, int w, int h, int round_0, int round_1, int do_average,
                             int use_jnt_comp_avg, int fwd_offset, int bck_offset);
/* svt_av1_build_compound_diffwtd_mask (elem_bytes 1: 8-bit pixels), _highbd (elem_bytes 2, shift = bd - 8) and _d16 (elem_bytes 2 on the compound
 * buffers, round = 14 - round_0 - round_1 + bd - 8) — common_dsp_rtcd.h:113-117; EbInterPrediction.c:78-175, C_DEFAULT/EbInterPrediction_c.c:15-45:
 * d_mask[h][w] (packed) = 38 + |a - b| / 16 after the rounding / shift, clamped to [0, 64]; inverse = DIFFWTD_38_INV. */
int svt_hip_diffwtd_mask_dev(SvtHipCtx *ctx, int elem_bytes, uint8_t *d_mask, const void *d_src0, int src0_stride, const void *d_src1, int src1_stride, int w,
                             int h, int inverse, int round, int shift);
/* svt_aom_lowbd_blend_a64_d16_mask / svt_aom_highbd_blend_a64_d16_mask (common_dsp_rtcd.h; EbBlend_a64_mask.c:34, :116): the two compound buffers
 * blended under a mask (at the block's resolution, or twice it in the directions subw / subh say) into pixels. */
int svt_hip_blend_a64_d16_dev(SvtHipCtx *ctx, int pix_bytes, int bd, void *d_dst, int dst_stride, const uint16_t *d_src0, int src0_stride,
                              const uint16_t *d_src1, int src1_stride, const uint8_t *d_mask, int mask_stride, int w, int h, int subw, int subh,
                              int round_0, int round_1);
/* svt_compute_mean_square_values_8x8 (aom_dsp_rtcd.h; EbPictureAnalysisProcess.c:287: mode 0, (sum of squares << 16) / (w * h) over a w x h
 * area) and svt_compute_sub_mean_8x8 (:310: mode 1, rows 0 / 2 / 4 / 6 of an 8x8 block, sum << 3) for a list of block offsets. */
int svt_hip_block_mean_batch_dev(SvtHipCtx *ctx, const uint8_t *d_plane, int stride, const int32_t *d_offs, int n, int mode, int w, int h,
                                 uint64_t *d_out);
/* svt_ext_sad_calculation_8x8_16x16 (aom_dsp_rtcd.h:630; EbMotionEstimation.c:122): one candidate of one 16x16 block per job.  d_state: 15 uint32
 * per job = best_sad8x8[4] best_sad16x16 best_mv8x8[4] best_mv16x16 (in/out) sad16x16 sad8x8[4] (out). */
int svt_hip_ext_sad_16x16_batch_dev(SvtHipCtx *ctx, const uint8_t *d_src, int src_stride, const uint8_t *d_ref, int ref_stride,
                                    const SvtHipExtSadJob *d_jobs, int n, uint32_t *d_state);
/* svt_ext_sad_calculation_32x32_64x64 (aom_dsp_rtcd.h:636; EbMotionEstimation.c:189).  d_state: 30 uint32 per job = sad16x16[16] (in)
 * best_sad32x32[4] best_sad64x64 best_mv32x32[4] best_mv64x64 (in/out) sad32x32[4] (out); d_mv[n]. */
int svt_hip_ext_sad_32x32_64x64_batch_dev(SvtHipCtx *ctx, uint32_t *d_state, const uint32_t *d_mv, int n);
/* svt_compute_cdef_dist_8bit / _16bit (aom_dsp_rtcd.c:97-98; EbEncCdef.c:134, :178) of one filter block: d_dst = the source plane at the filter
 * block's origin (the reference's argument name), d_src = the n filtered blocks packed one after the other, d_list[n][3] = (by, bx, skip) in units of
 * the block size (the reference's CdefList, EbDefinitions.h:77-81), block = (1 << bw_log2) x (1 << bh_log2); 8x8 luma (pli 0) uses the perceptual metric in FP64.  d_out[0] = the sum. */
int svt_hip_cdef_dist_dev(SvtHipCtx *ctx, int pix_bytes, const void *d_dst, int dstride, const void *d_src, const uint8_t *d_list, int n, int bw_log2,
                          int bh_log2, int coeff_shift, int pli, uint64_t *d_out);
/* svt_search_one_dual (aom_dsp_rtcd.c:363; EbEncCdef.c:1070): one greedy step of joint_strength_search_dual over d_mse0 / d_mse1[sb_count][64]:
 * the (luma, chroma) strength pair in [start_gi, end_gi)^2 that, added to the nb_strengths pairs already in d_lev0 / d_lev1, minimises the total;
 * written to d_lev0 / d_lev1[nb_strengths], total to d_work[0].  d_work: 4097 + sb_count uint64 of scratch. */
int svt_hip_cdef_search_one_dual_dev(SvtHipCtx *ctx, const uint64_t *d_mse0, const uint64_t *d_mse1, int sb_count, int *d_lev0, int *d_lev1,
                                     int nb_strengths, int start_gi, int end_gi, uint64_t *d_work);
/* joint_strength_search_dual (EbEncCdef.c:1140-1164), the strength-pair selection of finish_cdef_search for one count nb_strengths (1, 2, 4, 8): the
 * greedy steps and the 4 * nb_strengths refinement steps of svt_search_one_dual queued back to back, no host round trip in between.  d_lev0 / d_lev1
 * [8] receive the selected pairs, d_work[0] the total; d_work: 4097 + sb_count uint64 of scratch. */
int svt_hip_cdef_joint_strength_search_dev(SvtHipCtx *ctx, const uint64_t *d_mse0, const uint64_t *d_mse1, int sb_count, int *d_lev0, int *d_lev1,
                                           int nb_strengths, int start_gi, int end_gi, uint64_t *d_work);
/* The four joint_strength_search_dual calls of finish_cdef_search (nb_strengths = 1, 2, 4, 8; EbEncCdef.c:1258) at once; the chains are independent.  Two forms
 * (svt_hip_set_cdef_select_form, or SVT_HIP_CDEF_SELECT=steps|resident in the environment; the default is steps):
 *  - steps: one pair of launches per step index advances all chains that are still running (80 launches instead of 225: slices of the filter blocks into
 *    per-slice totals, then the sum over slices and the first minimum -- no atomics on the totals).  0.64 - 0.77 ms for 2040 filter blocks on MI355X, nearly
 *    all of it dependent-launch latency: the selections of several pictures issued on their own streams overlap almost freely.
 *  - resident: ONE launch for the 40 step indices (pictures of up to 2048 filter blocks): 256 workgroups each own a 4 x 4 tile of strength pairs, keep the tile's
 *    table columns in LDS and exchange one 8-byte word per chain and step.  0.37 ms when every distortion is below 2^26, 0.58 ms below 2^32, 0.89 ms above
 *    (same data: 0.64 / 0.77 / 0.77 ms in steps) -- the form for ONE picture in flight.  Its workgroups wait for each other, so all resident selections of a
 *    device are issued on one library-owned stream (ordered against the context's stream with events; inside a stream capture they are chained with events
 *    instead) and other work in flight delays it: with four frames in flight bench.py's step takes 12.1 ms against 8.7 ms in steps.
 * Both forms end a chain as soon as its list is a fixed point (nb refinement steps in a row that put back the pair they dropped; the list is then rotated by the
 * remaining steps mod nb, which is what those steps would leave): 16 - 21 dependent steps instead of 40 on coded pictures -- 0.44 ms in steps, 0.23 ms resident.
 * d_state: SVT_HIP_CDEF_SELECT_STATE_BYTES of device memory, cleared by the call; afterwards it starts with SvtHipCdefSelectResult (the selected pairs of each
 * count and the totals).  status[0] != 0 afterwards: the resident form gave up waiting for a workgroup (bounded spin; nothing else should be able to cause
 * it) -- the result is not valid, svt_hip_cdef_finish_dev reports cdef_bits = -1 for it; run the selection again in the steps form. */
typedef struct {
    int32_t  lev0[4][8], lev1[4][8]; /* [log2 nb_strengths][pair]: cdef_y_strength / cdef_uv_strength indices */
    uint32_t status[4];              /* all zero after a complete selection */
    uint64_t tot_mse[4];
} SvtHipCdefSelectResult;
#define SVT_HIP_CDEF_SELECT_STATE_BYTES (sizeof(SvtHipCdefSelectResult) + (size_t)8192 + (size_t)4 * 128 * 4096 * 8)   /* + exchange slots, per-slice totals / transposed tables */
#define SVT_HIP_CDEF_SELECT_DEFAULT  (-1) /* SVT_HIP_CDEF_SELECT from the environment, else steps */
#define SVT_HIP_CDEF_SELECT_STEPS    0
#define SVT_HIP_CDEF_SELECT_RESIDENT 1
int svt_hip_set_cdef_select_form(SvtHipCtx *ctx, int form);
int svt_hip_cdef_strength_select_dev(SvtHipCtx *ctx, const uint64_t *d_mse0, const uint64_t *d_mse1, int sb_count, int start_gi, int end_gi, void *d_state,
                                     size_t state_bytes);
/* The same for n_pictures pictures of equal size (d_mse0 / d_mse1 / d_states: HOST arrays of n_pictures device pointers).  steps form: ONE set of launches for
 * all of them (blockIdx.y = picture); measured on MI355X this does not beat issuing each picture's selection on its own stream (bench.py, four frames: 9.9 ms
 * against 9.5 ms per step -- the join it needs idles the other streams for the length of the chain).  resident form: one picture after the other. */
int svt_hip_cdef_strength_select_multi_dev(SvtHipCtx *ctx, int n_pictures, const uint64_t *const *d_mse0, const uint64_t *const *d_mse1, int sb_count, int start_gi,
                                           int end_gi, void *const *d_states, size_t state_bytes);
/* finish_cdef_search after its four searches (EbEncCdef.c:1258-1298): the number of signalled strength pairs by rate-distortion cost
 * (RDCOST(lambda, av1_cost_literal(sb_count * bits + nb * CDEF_STRENGTH_BITS * 2), tot_mse * 16), the first minimum over bits = 0..3), then every filter
 * block's pair (first minimum of mse0[i][y[gi]] + mse1[i][uv[gi]]).  d_state = what svt_hip_cdef_strength_select_dev left; d_sel_gi[sb_count] = the
 * index the reference stores in mbmi.cdef_strength; d_fb_y / d_fb_uv (may be NULL) receive the strength values per filter block in the layout
 * svt_hip_cdef_apply_frame_dev reads, at d_sb_fb[i] (NULL: i) -- the distortion tables only list the filter blocks that are not all-skip.  The
 * strength values are positions in the caller's strength list: the reduced lists of the fast pick methods are mapped by the caller
 * (get_cdef_filter_strengths), as finish_cdef_search does after this point. */
typedef struct {
    int32_t  cdef_bits, nb_strengths;
    int32_t  y_strength[8], uv_strength[8];
    uint64_t best_cost;
} SvtHipCdefFinish;
int svt_hip_cdef_finish_dev(SvtHipCtx *ctx, const uint64_t *d_mse0, const uint64_t *d_mse1, int sb_count, const void *d_state, uint64_t lambda,
                            const int32_t *d_sb_fb, SvtHipCdefFinish *d_out, int32_t *d_sel_gi, uint8_t *d_fb_y, uint8_t *d_fb_uv);
/* The self-guided projection on MATERIALISED filter planes (the form the reference's pointers have; the frame kernels never write flt0 / flt1):
 * mode 0 = svt_get_proj_subspace (common_dsp_rtcd.h; EbRestorationPick.c:448): d_acc[5] = {H00, H01, H11, C0, C1} as exact integers, d_xq[2] = the
 * solved pair; mode 1 = svt_av1_lowbd_pixel_proj_error / svt_av1_highbd_pixel_proj_error (:174, :244): d_acc[0] = the squared error of the
 * projection with xq[2] (host array).  r0 / r1 = the radii of the parameter set (0 = filter absent). */
int svt_hip_sgr_flt_proj_dev(SvtHipCtx *ctx, int pix_bytes, const void *d_src, int src_stride, const void *d_dat, int dat_stride, const int32_t *d_flt0,
                             int flt0_stride, const int32_t *d_flt1, int flt1_stride, int w, int h, int r0, int r1, int mode, const int32_t *xq,
                             int64_t *d_acc, int32_t *d_xq);
/* svt_aom_convolve8_horiz / _vert (common_dsp_rtcd.h:231; Common/Codec/convolve.c:286, :298): d_filters = the 16 x 8 kernel table the reference
 * derives from its filter pointer (get_filter_base), q0 = the first phase (get_filter_offset), step_q4 = phase advance per output sample
 * (16 = unscaled).  d_src addresses the first output sample's position (taps reach 3 samples before, 4 + scaling after). */
int svt_hip_convolve8_dev(SvtHipCtx *ctx, int vert, const uint8_t *d_src, int src_stride, uint8_t *d_dst, int dst_stride, const int16_t *d_filters, int q0,
                          int step_q4, int w, int h);
/* svt_av1_wiener_convolve_add_src / svt_av1_highbd_wiener_convolve_add_src (common_dsp_rtcd.h; Common/Codec/convolve.c:105, :205) of one w x h
 * processing unit: d_taps[16] = the horizontal and the vertical 8-tap kernel, round_0 / round_1 = ConvolveParams; d_src needs 3 samples of
 * context on every side (4 after). */
int svt_hip_wiener_convolve_add_src_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_src, int src_stride, void *d_dst, int dst_stride,
                                        const int16_t *d_taps, int w, int h, int round_0, int round_1);
/* svt_cdef_find_dir (common_dsp_rtcd.h:1031) for a list of 8x8 blocks of a 16-bit image (offsets in samples). */
int svt_hip_cdef_find_dir_batch_dev(SvtHipCtx *ctx, const uint16_t *d_img, int stride, const int32_t *d_offs, int n, int coeff_shift,
                                    int32_t *d_dir, int32_t *d_var);
/* svt_cdef_filter_block (common_dsp_rtcd.h:1033) for a list of blocks of the 16-bit staging image (CDEF_VERY_LARGE outside the picture);
 * strengths as the reference passes them (already scaled by coeff_shift), block 4 or 8 samples wide / high (log2 2 or 3).
 * Exactly one of d_dst8 / d_dst16 is non-NULL. */
typedef struct { int32_t in_off, dst_off, pri_strength, sec_strength, dir, pri_damping, sec_damping, bw_log2, bh_log2, coeff_shift; } SvtHipCdefBlk;
int svt_hip_cdef_filter_block_batch_dev(SvtHipCtx *ctx, const uint16_t *d_in, int in_stride, const SvtHipCdefBlk *d_blks, int n,
                                        uint8_t *d_dst8, uint16_t *d_dst16, int dst_stride);
/* svt_aom_[highbd_]lpf_{vertical,horizontal}_{4,6,8,14} (common_dsp_rtcd.h:1044-1075) for a list of 4-sample edge segments with explicit
 * thresholds.  off = sample index of the first q0 sample; dir 0 = vertical edge (filter taps run along x, the 4 samples along y), 1 =
 * horizontal edge.  The segments of one call must not touch each other's samples (they are filtered concurrently). */
typedef struct { int32_t off; uint8_t dir, len, blimit, limit, thresh, reserved[3]; } SvtHipLpfEdge;
int svt_hip_lpf_edges_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, void *d_plane, int stride, const SvtHipLpfEdge *d_edges, int n);

/* ------------------------------------------------------------------ mode decision: picture-level precompute ----------
 * md_stage_0 -> fast_loop_core (Encoder/Codec/EbProductCodingLoop.c:1461, :907) predicts a candidate and measures its luma distortion against the source,
 * one block and one candidate at a time.  For a FULL-PEL single-reference translation candidate the prediction is a copy of the reference block
 * (inter_pu_prediction_av1, EbEncInterPrediction.c:6178 -> av1_inter_prediction :4040 -> svt_av1_convolve_2d_copy_sr) and the distortion is
 * svt_nxm_sad_kernel_sub_sampled (:953; aom_dsp_rtcd.c:372 — the plain SAD of all rows), and in the first partitioning pass (PD_PASS_0) at presets above M4
 * the open-loop ME vectors enter stage 0 unrefined (EbEncDecProcess.c:3050-3093).  One launch per picture computes that distortion for every
 * (superblock, PU of `pus`, reference picture):
 *   d_src  : sample (0, 0) of the source luma plane, pic_w x pic_h samples exist from there (PUs that leave them are skipped).  Any address and stride: the kernels read
 *            a row's samples as whole aligned dwords, so up to 4 bytes past the last sample of a PU row are read (8- and 16-bit planes alike) and the caller's plane
 *            must be readable there — after the last row of the picture too.  The bridge's padded pictures are.
 *   pus    : the PUs of a 64x64 superblock, positions relative to it (host array; the 85 square PUs of the open-loop ME in its order, or any other list)
 *   refs   : the reference pictures' luma planes (host array of n_refs <= SVT_HIP_MD_MAX_REFS descriptors; d_plane = device address of sample (0, 0),
 *            [x_min, x_max) x [y_min, y_max) = the sample coordinates its allocation holds, padding included)
 *   d_mv   : [n_sb][n_pus][n_refs] vectors in whole samples, x | y << 16 (two int16); x = SVT_HIP_MD_NO_MV = no candidate
 *   d_sad  : [n_sb][n_pus][n_refs] SAD of the PU against the reference block at its vector; 0xffffffff = not computed (no vector, PU outside the picture,
 *            reference block outside the allocation) */
#define SVT_HIP_MD_MAX_REFS 7     /* MAX_PA_ME_MV, Encoder/Codec/EbMotionEstimationLcuResults.h:23 */
#define SVT_HIP_MD_MAX_PUS 128
#define SVT_HIP_MD_NO_MV (-32768)
typedef struct { uint8_t x, y, w, h; } SvtHipMdPu;   /* w a multiple of 4, at most 64 (every such width, not only the powers of two); h 1 .. 64 */
typedef struct { const uint8_t *d_plane; int32_t stride, x_min, y_min, x_max, y_max; } SvtHipMdRefPlane;
int svt_hip_md_fullpel_sad_picture_dev(SvtHipCtx *ctx, const uint8_t *d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus,
                                       const SvtHipMdPu *pus, int n_refs, const SvtHipMdRefPlane *refs, const uint32_t *d_mv, uint32_t *d_sad);
/* The same table for the COMPOUND-AVERAGE candidates mode decision builds from two ME vectors (NEW_NEWMV of the open-loop ME's bi-directional candidates,
 * Encoder/Codec/EbModeDecision.c:3408-3540 with MD_COMP_AVG: interinter_comp.type COMPOUND_AVERAGE, compound_idx 1).  Both predictions are full-pel copies in the compound
 * domain (svt_av1_jnt_convolve_2d_copy, Common/Codec/convolve.c) and the second averages: the luma prediction is (a + b + 1) >> 1 sample by sample.
 *   pairs : n_pairs <= SVT_HIP_MD_MAX_PAIRS pairs of columns (c0, c1) of the vector table: the first / second reference of the candidate; its vectors are d_mv's entries
 *           of those two columns for the same PU
 *   d_sad : [n_sb][n_pus][n_pairs] SAD of the PU against the averaged prediction; 0xffffffff = not computed (a missing vector, PU or block outside) */
#define SVT_HIP_MD_MAX_PAIRS 16
int svt_hip_md_fullpel_avg_sad_picture_dev(SvtHipCtx *ctx, const uint8_t *d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus,
                                           const SvtHipMdPu *pus, int n_refs, const SvtHipMdRefPlane *refs, const uint32_t *d_mv, int n_pairs,
                                           const uint8_t (*pairs)[2], uint32_t *d_sad);
/* Both tables for the 16-bit planes a 10-bit encode's mode decision decides on (hbd_mode_decision 1 / 2: fast_loop_core predicts from reference_picture16bit and measures with
 * sad_16b_kernel, Encoder/C_DEFAULT/EbComputeSAD_C.c:39; the compound copy is svt_av1_highbd_jnt_convolve_2d_copy, which rounds to (a + b + 1) >> 1 as well).  d_src and every
 * refs[i].d_plane point at 16-bit samples; strides and the reference boxes are in samples. */
int svt_hip_md_fullpel_sad_picture_hbd_dev(SvtHipCtx *ctx, const uint16_t *d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus,
                                           const SvtHipMdPu *pus, int n_refs, const SvtHipMdRefPlane *refs, const uint32_t *d_mv, uint32_t *d_sad);
int svt_hip_md_fullpel_avg_sad_picture_hbd_dev(SvtHipCtx *ctx, const uint16_t *d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus,
                                               const SvtHipMdPu *pus, int n_refs, const SvtHipMdRefPlane *refs, const uint32_t *d_mv, int n_pairs,
                                               const uint8_t (*pairs)[2], uint32_t *d_sad);
/* The probes of mode decision's sub-pel refinement (md_subpel_search, Encoder/Codec/EbProductCodingLoop.c:2063 -> svt_av1_find_best_sub_pixel_tree, mcomp.c:350): every probe
 * is svt_upsampled_pref_error (mcomp.c:102) = svt_aom_upsampled_pred (Encoder/C_DEFAULT/variance.c:212-269) + svt_aom_variance{W}x{W} against the source.  The tree starts at
 * the block's full-pel vector and its half-pel and quarter-pel rounds stay inside the 7 x 7 quarter-pel grid around it, so one launch per picture computes, for every
 * (superblock, square PU of `pus`, reference picture), all 49 grid positions:
 *   d_out : [n_sb][n_pus][n_refs][49][2] = (variance, sse) of grid position 7 * row + col, offsets (2 col - 6, 2 row - 6) eighth-samples from the full-pel vector in d_mv;
 *           0xffffffff pairs = not computed (no vector, PU outside the picture or not 8 / 16 / 32 / 64 square, window outside the reference's allocation)
 *   bank  : the interpolation kernels, 0 .. 5 as in SvtHipUpsampledBlk, all accepted (1 = EIGHTTAP_SMOOTH, 2 = MULTITAP_SHARP, 5 = 4-tap smooth); the encoder's
 *           subpel_search_type uses three of them: 0 = USE_8_TAPS, 4 = USE_4_TAPS, 3 = USE_2_TAPS
 * The other arguments are svt_hip_md_fullpel_sad_picture_dev's. */
#define SVT_HIP_MD_GRID 49
int svt_hip_md_subpel_grid_picture_dev(SvtHipCtx *ctx, const uint8_t *d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const SvtHipMdPu *pus,
                                       int n_refs, const SvtHipMdRefPlane *refs, const uint32_t *d_mv, int bank, uint32_t *d_out);
/* The half-pel round alone (svt_first_level_check, Encoder/Codec/mcomp.c:188: the eight half-sample neighbours of the full-pel vector, and the centre):
 *   d_out : [n_sb][n_pus][n_refs][9][2] = (variance, sse) of position 3 * row + col, offsets (4 col - 4, 4 row - 4) eighth-samples — the same values as positions
 *           (1, 3, 5) x (1, 3, 5) of the 7 x 7 table.  One workgroup per (superblock, PU, reference) stages the window once for all nine. */
#define SVT_HIP_MD_HALFPEL_GRID 9
int svt_hip_md_halfpel_grid_picture_dev(SvtHipCtx *ctx, const uint8_t *d_src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const SvtHipMdPu *pus,
                                        int n_refs, const SvtHipMdRefPlane *refs, const uint32_t *d_mv, int bank, uint32_t *d_out);

/* ------------------------------------------------------------------ intra prediction --------------------------------------------------------
 * The AV1 luma intra predictors for a list of blocks in one launch: svt_aom_[highbd_]{dc,dc_left,dc_top,dc_128,v,h,smooth,smooth_v,smooth_h,paeth}_predictor_WxH_c
 * (Common/Codec/EbIntraPrediction.c:863-968 and the size wrappers after them), dr_predictor / highbd_dr_predictor (:2260, :2374: zones 1 / 2 / 3, :246-345) and
 * the edge conditioning build_intra_predictors / filter_intra_edge (:2545) do before them: filter_intra_edge_corner[_high] (:2288, :2427),
 * svt_av1_filter_intra_edge[_high]_c (:88, :2403) and svt_av1_upsample_intra_edge[_high]_c (Common/C_DEFAULT/EbIntraPrediction_c.c:14-55).
 *   d_edges : edge records, samples of pix_bytes each.  One record is what the reference keeps on its stack: 160 samples of "above" followed by 160 of "left"
 *             (MAX_TX_SIZE * 2 + 32 each); element 16 of each is sample 0, element 15 the corner (sample -1).  A job names its record by the index of the record's
 *             first sample (edge_off).  Records are read only: a job conditions a private copy, in the reference's order -- corner filter, edge filter of
 *             "above", of "left", then up-sampling of "above", of "left" -- and predicts from that copy.
 *   d_jobs  : device array.  Strengths and sample counts are the caller's (intra_edge_filter_strength / use_intra_edge_upsample and the n_px arithmetic of
 *             build_intra_predictors are three-line functions of the block's position).  The filtered run of an edge is npx samples starting at sample -1
 *             (start_m1 = 1, the corner itself passes through unfiltered as in the reference) or at sample 0; npx is clamped to 129, up_npx to 16.
 *             A job whose tx_size (> 18), mode (> 12) or angle_delta (outside -3 .. 3) is out of range is skipped: nothing is written for it.
 *   d_dst   : destination plane (pix_bytes per sample, stride in samples); a job writes its W x H block at (dst_x, dst_y).  Jobs must not overlap.
 * pix_bytes 1 with bd 8, or pix_bytes 2 with bd 8 / 10.  Chroma-from-luma and filter-intra have entry points of their own below; palette and intra block copy are
 * not covered. */
typedef struct {
    uint32_t edge_off;            /* first sample of this job's edge record in d_edges */
    int32_t  dst_x, dst_y;        /* top-left sample of the block in the destination plane */
    uint8_t  tx_size;             /* TxSize 0..18: the block shape */
    uint8_t  mode;                /* PredictionMode 0..12 (DC, V, H, D45, D135, D113, D157, D203, D67, SMOOTH, SMOOTH_V, SMOOTH_H, PAETH) */
    int8_t   angle_delta;         /* -3..3 (x 3 degrees), directional modes only */
    uint8_t  dc_have;             /* DC_PRED: bit 0 = left available, bit 1 = above available (dc_pred[left][above]) */
    uint8_t  corner_filter;       /* 1: filter_intra_edge_corner before the edge filters */
    uint8_t  strength_above, strength_left;   /* 0 = no edge filter, else 1..3 */
    uint8_t  npx_above, npx_left; /* samples the edge filter is given (its sz), at most 129 */
    uint8_t  start_m1;            /* 1: the filtered runs start at sample -1, else at sample 0 */
    uint8_t  upsample_above, upsample_left;
    uint8_t  up_npx_above, up_npx_left;       /* samples svt_av1_upsample_intra_edge is given (its sz), at most 16 */
} SvtHipIntraJob;
int svt_hip_intra_predict_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_edges, const SvtHipIntraJob *d_jobs, int njobs, void *d_dst,
                                    int dst_stride);
/* Chroma-from-luma (UV_CFL_PRED) for a list of 4:2:0 chroma blocks in one launch: svt_cfl_luma_subsampling_420_{lbd,hbd} -> svt_subtract_average ->
 * svt_cfl_predict_{lbd,hbd} (Common/Codec/EbIntraPrediction.c:349-402, Common/C_DEFAULT/cfl_c.c), as cfl_prediction / av1_cost_calc_cfl compose them
 * (Encoder/Codec/EbProductCodingLoop.c:2723-3230).  Per job: the 2W x 2H luma area at (luma_x, luma_y) is read, (a + b + c + d) << 1 per chroma sample, the block
 * average (sum + W H / 2) >> log2(W H) subtracted, and for each selected plane clip(pred + ROUND_POWER_OF_TWO_SIGNED(alpha_q3 * ac, 6), bd) written at
 * (dst_x, dst_y).  pred is the sample already in the chroma plane at that position (the in-place form: the reference passes pred == dst), or, with dc_from_edges,
 * the DC predictor of the plane's edge record -- the dc_pred[left][above] selection of mode 0 of svt_hip_intra_predict_batch_dev -- so that a CfL block is one launch.
 *   d_luma  : the luma plane the areas are read from (pix_bytes per sample, stride in samples); areas of different jobs may overlap
 *   d_edges : edge records in the layout of svt_hip_intra_predict_batch_dev; read only by jobs with dc_from_edges (edge_off[0] Cb, edge_off[1] Cr)
 *   d_cb / d_cr : the two chroma planes, one stride.  One of them may be NULL: that plane is then written by no job, whatever plane_mask says.
 *   d_ac    : NULL, or [njobs][32][32] int16: job i's pred_buf_q3 after the average subtraction, its W x H corner at row stride 32 (CFL_BUF_LINE); nothing else
 *             of the slot is written
 * 4:2:0 only.  A job whose tx_size is not one of the 14 shapes with both sides <= 32 (CFL_SUB_AVG_FN), or with an |alpha_q3| above 16, writes nothing.  Jobs must
 * not overlap in the chroma planes.  pix_bytes 1 with bd 8, or pix_bytes 2 with bd 8 / 10.  Stream-ordered and asynchronous: no host synchronisation, no
 * allocation, no read-back. */
typedef struct {
    int32_t  luma_x, luma_y;      /* top-left sample of the 2W x 2H luma area (rounded by the caller the way cfl_prediction does) */
    int32_t  dst_x, dst_y;        /* top-left sample of the block in both chroma planes */
    uint32_t edge_off[2];         /* dc_from_edges: first sample of the Cb / Cr edge record in d_edges */
    int8_t   alpha_q3[2];         /* -16..16 for Cb / Cr (cfl_idx_to_alpha); 0 is legal */
    uint8_t  tx_size;             /* TxSize of the chroma block, both sides <= 32 */
    uint8_t  plane_mask;          /* bit 0 = Cb, bit 1 = Cr */
    uint8_t  dc_from_edges;       /* 0: pred is what the chroma plane holds; 1: pred is the DC predictor of the edge record */
    uint8_t  dc_have;             /* dc_from_edges: bit 0 = left available, bit 1 = above available */
    uint8_t  reserved[2];
} SvtHipCflJob;
int svt_hip_cfl_predict_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_luma, int luma_stride, const void *d_edges, const SvtHipCflJob *d_jobs,
                                  int njobs, void *d_cb, void *d_cr, int chroma_stride, int16_t *d_ac);
/* Filter-intra (use_filter_intra: the five recursive 4x2-patch predictors FILTER_DC, FILTER_V, FILTER_H, FILTER_D157, FILTER_PAETH) for a list of blocks in one
 * launch: svt_av1_filter_intra_predictor_c (Common/C_DEFAULT/filterintra_c.c) / highbd_filter_intra_predictor (Common/Codec/EbIntraPrediction.c:2492).  The edge
 * record is the one of svt_hip_intra_predict_batch_dev; a job reads above[-1 .. W - 1] and left[0 .. H - 1] of it, unconditioned, and writes its W x H block at
 * (dst_x, dst_y) of d_dst.  A job with mode > 4, tx_size > 18 or a 64-sample side writes nothing.  Jobs must not overlap.  pix_bytes 1 with bd 8, or pix_bytes 2
 * with bd 8 / 10.  Stream-ordered and asynchronous. */
typedef struct {
    uint32_t edge_off;            /* first sample of this job's edge record in d_edges */
    int32_t  dst_x, dst_y;        /* top-left sample of the block in the destination plane */
    uint8_t  tx_size;             /* TxSize, both sides <= 32 */
    uint8_t  mode;                /* FilterIntraMode 0..4 */
    uint8_t  reserved[2];
} SvtHipFilterIntraJob;
int svt_hip_filter_intra_predict_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_edges, const SvtHipFilterIntraJob *d_jobs, int njobs, void *d_dst,
                                           int dst_stride);
/* The palette luma search for a list of blocks of one luma plane in one launch: search_palette_luma (Encoder/Codec/palette.c:320-496) -- svt_av1_count_colors[_highbd]
 * (Encoder/Codec/EbPictureAnalysisProcess.c:3364-3399), the dominant colours, svt_av1_k_means_dim1 (Encoder/Codec/k_means_template.h:32-133, max_itr 50) from the
 * lb / ub centroids, and for each of the up to fourteen candidates palette_rd_y (palette.c:245-312: optimize_palette_colors, av1_remove_duplicates, the clip,
 * svt_av1_calc_indices_dim1, extend_palette_color_map) -- and svt_av1_palette_color_cost_y (palette.c:88-153) of every candidate kept.  A job's results are what the
 * reference leaves in palette_cand[0 .. tot_palette_cands), in its order: the dominant-colour candidates n = min(colors, 8) down to 2 in steps of dominant_step, then
 * the k-means candidates n = min(colors, 8) down to 2, each kept only when its palette_size is above 2.  The only neighbour-dependent input, the colour cache of
 * svt_get_palette_cache (palette.c:163-205), is data of the job.
 *   d_plane   : the luma plane (pix_bytes per sample, stride in samples); a job reads rows x cols samples at (x, y), which the caller keeps inside the plane
 *   d_results : [njobs]; colors = the distinct sample values (0 when a 16-bit sample is not below 1 << bd, as the reference returns), n_cands = candidates kept;
 *               nothing is kept unless 1 < colors <= 64
 *   d_cands   : [njobs][14]; job i's kept candidates are records 14 i .. 14 i + n_cands - 1
 *   d_maps    : candidate c of a job at map_off + c * bw * bh: the colour indices of the whole bw x bh block, row stride bw, the part outside rows x cols extended
 *               from the last row / column inside
 * Records and maps at candidate index >= n_cands are unspecified; every store stays inside the job's fourteen records and 14 * bw * bh map bytes.  A job whose
 * bw x bh is not one of the 16 shapes svt_av1_allow_palette admits (Encoder/Codec/EbModeDecision.c:5052: 8x8 .. 64x64 with both sides <= 64, 4x16, 16x4), whose cols /
 * rows is outside 1 .. bw / 1 .. bh, whose x or y is negative, whose n_cache is above 16 or whose dominant_step is not 1 or 2 gets colors = -1, n_cands = 0 and nothing
 * else.  pix_bytes 1 with bd 8, or pix_bytes 2 with bd 8 / 10.  Palette chroma, the colour-map rate (svt_av1_cost_color_map) and intra block copy are not covered.
 * Stream-ordered and asynchronous: no host synchronisation, no allocation, no read-back. */
#define SVT_HIP_PALETTE_MAX_CANDS 14
typedef struct {
    int32_t  x, y;                /* top-left sample of the block in the plane */
    int32_t  bw, bh;              /* the block's full size */
    int32_t  cols, rows;          /* the part inside the picture (av1_get_block_dimensions: mb_to_right_edge / mb_to_bottom_edge), 1 .. bw / 1 .. bh */
    int32_t  n_cache;             /* 0 .. 16 */
    int32_t  dominant_step;       /* 1, or 2 (palette_level == 6) */
    uint16_t cache[16];           /* the sorted colour cache svt_get_palette_cache would return */
    int64_t  map_off;             /* first byte of this job's maps in d_maps */
} SvtHipPaletteJob;
typedef struct {
    int32_t colors;               /* svt_av1_count_colors[_highbd]; -1 for a job with a bad field */
    int32_t n_cands;              /* tot_palette_cands, 0 .. 14 */
} SvtHipPaletteResult;
typedef struct {
    int32_t  color_cost;          /* svt_av1_palette_color_cost_y of this candidate with the job's cache */
    uint16_t colors[8];           /* pmi.palette_colors[0 .. size), ascending; 0 beyond */
    uint16_t raw[8];              /* the n centroids before optimize_palette_colors, in the reference's order: the top colours or the k-means result; 0 beyond */
    uint8_t  size;                /* pmi.palette_size[0], 3 .. 8 */
    uint8_t  n;                   /* the centroids the candidate started from, 2 .. 8 */
    uint8_t  kind;                /* 0 = dominant colours, 1 = k-means */
    uint8_t  reserved;            /* 0 */
} SvtHipPaletteCand;
int svt_hip_palette_search_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_plane, int stride, const SvtHipPaletteJob *d_jobs, int njobs,
                                     SvtHipPaletteResult *d_results, SvtHipPaletteCand *d_cands, uint8_t *d_maps);
/* The same contract on host pointers, serially, from the arithmetic header the kernel shares (csrc/palette.h): no context and no device.  The same refusals. */
int svt_hip_palette_search_host(int pix_bytes, int bd, const void *plane, int stride, const SvtHipPaletteJob *jobs, int njobs, SvtHipPaletteResult *results,
                                SvtHipPaletteCand *cands, uint8_t *maps);
/* is_screen_content (Encoder/Codec/EbPictureAnalysisProcess.c:3519-3601) of a luma plane: over every whole 16x16 block (r + 16 <= height, c + 16 <= width),
 * counts_1 = the blocks is_valid_palette_nb_colors[_highbd] (:3459-3514) accepts with threshold 4 (more than one colour, at most four), counts_2 = those whose
 * svt_av1_get_sby_perpixel_variance / svt_av1_high_get_sby_perpixel_variance (:3434-3454: svt_aom_variance16x16 / svt_aom_highbd_10_variance16x16 against the constant
 * 128 / 512, ROUND_POWER_OF_TWO(var, 8)) is above 0; then color_detection = counts_1 * 2560 > width * height and sc_content_detected = color_detection &&
 * counts_2 * 3072 > width * height (:3594-3599), which decide allow_screen_content_tools and palette_level (Encoder/Codec/EbPictureDecisionProcess.c:912-922).
 * d_out receives four int32: counts_1, counts_2, color_detection, sc_content_detected.  pix_bytes 1 with bd 8, or pix_bytes 2 with bd 10: the 16-bit plane is the
 * packed one (svt_hip_picture_format_dev), where the reference packs each block from its 8 + 2-bit planes first.  width * height must fit 31 bits.  Stream-ordered
 * and asynchronous. */
int svt_hip_screen_content_detect_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_plane, int stride, int width, int height, int32_t *d_out);
/* Intra block copy: the hash table of a picture and the hash search of a list of blocks.  IntraBC searches the SOURCE picture (Encoder/Codec/EbModeDecision.c:4443-4448),
 * so nothing here waits for a neighbour's reconstruction.  pix_bytes 1 with bd 8, or pix_bytes 2 with bd 8 / 10 (the reference has the 16-bit branch of the hashes
 * although its encoder passes 8-bit samples).  The CRC is Encoder/Codec/hash.c:13-62: width 24, polynomials 0x5D6DCB (hash 1) and 0x864CFB (hash 2), the remainder
 * reset per value; a 2x2 block hashes its 4 sample bytes or the 8 bytes of its four 16-bit samples in memory order, a larger block the 16 bytes of its four
 * children's hashes as little-endian words.  Every device entry point is stream-ordered and asynchronous: no allocation, no host synchronisation, no read-back; what
 * it refuses it refuses before any launch.  width, height <= 32767 (an entry's int16), width * height within 31 bits, stride >= width.  The diamond and mesh
 * searches around the hash search and the final choice are svt_hip_ibc_full_search_batch_dev below; a hook in the encoder is not covered. */
#define SVT_HIP_IBC_HASH_BUCKETS (1 << 19)
#define SVT_HIP_IBC_MV_VALS 32767
typedef struct {
    int16_t  x, y;                /* top-left sample of the block */
    uint32_t hash_value2;
} SvtHipIbcHashEntry;             /* BlockHash (Encoder/Codec/hash_motion.h) */
/* bytes of d_scratch for a picture (0 for a size that is refused), and the most entries its table can have (every position of every block size) */
size_t svt_hip_ibc_hash_scratch_bytes(int width, int height);
size_t svt_hip_ibc_hash_max_entries(int width, int height);
/* svt_av1_generate_block_2x2_hash_value (Encoder/Codec/hash_motion.c:138-186) followed by svt_av1_generate_block_hash_value (:188-251) applied 2 -> 4 -> ... ->
 * block_size (2, 4, ... 128): what those calls leave in the valid region x < width - block_size + 1, y < height - block_size + 1 of
 *   d_hash1, d_hash2 : uint32[width * height], indexed y * width + x as the reference indexes them
 *   d_same           : int8[3][width * height]: same_info[0] (rows alike), [1] (columns alike), [2] the "add this position" flag of :238-250 (block_size >= 4 only)
 * Everything outside the valid region is unspecified; a picture smaller than block_size has an empty region and nothing is written.  d_scratch: at least
 * svt_hip_ibc_hash_scratch_bytes(width, height), 256-byte aligned. */
int svt_hip_ibc_block_hashes_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_luma, int stride, int width, int height, int block_size, uint32_t *d_hash1,
                                 uint32_t *d_hash2, int8_t *d_same, void *d_scratch, size_t scratch_bytes);
/* The table the hash generation of an intra picture builds (Encoder/Codec/EbModeDecisionConfigurationProcess.c:939-1051: the two generators and six
 * svt_av1_add_to_hash_map_by_row_with_precal_data calls, hash_motion.c:253-283), as compressed rows:
 *   d_bucket_start : int32[SVT_HIP_IBC_HASH_BUCKETS + 1]; bucket k = (hash1 & 0xFFFF) + (size_index << 16), size_index 0 .. 5 for 4 .. 128, holds entries
 *                    d_bucket_start[k] .. d_bucket_start[k + 1] - 1
 *   d_entries      : [capacity]; inside a bucket in the reference's insertion order, ascending x, then ascending y (the inserter scans column by column and a
 *                    bucket belongs to one block size).  The search keeps the first smallest cost, so the order is part of the result; it never depends on the
 *                    order in which atomics arrive
 *   d_info         : int32[2] = {n_entries, stored}.  d_bucket_start is always complete; when n_entries > capacity no entry is stored, stored = 0, and nothing
 *                    is written outside the buffers
 * d_scratch: at least svt_hip_ibc_hash_scratch_bytes(width, height), 256-byte aligned. */
int svt_hip_ibc_hash_table_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_luma, int stride, int width, int height, int32_t *d_bucket_start,
                               SvtHipIbcHashEntry *d_entries, int64_t capacity, int32_t *d_info, void *d_scratch, size_t scratch_bytes);
/* The hash search of svt_av1_full_pixel_search (Encoder/Codec/av1me.c:1346-1403, the do { } while (0)) for every job in one launch; the comparison with the diamond
 * search's var (:1404-1408) stays with the caller.  Per job: the block's two hash values as svt_av1_get_block_hash_value computes them from the samples
 * (hash_motion.c:285-369); count = the bucket's size, and the job stops when count <= (intra ? 1 : 0); for every entry of equal hash_value2, in bucket order,
 * av1_is_dv_valid (Encoder/Codec/EbAdaptiveMotionVectorPrediction.c:2003-2083, when intra) and is_mv_in (av1me.c:320-323), then the cost svt_av1_get_mvpred_var
 * (av1me.c:328-342): svt_aom_variance{N}x{N} of the block against the entry's block of the same plane (bd 10: the form of svt_aom_highbd_10_variance) plus
 * mv_err_cost (av1me.c:273-282); the strict < keeps the first smallest cost.
 *   d_mv_joint_cost : int32[4]; d_mv_comp_cost : int32[2][SVT_HIP_IBC_MV_VALS], row then column, entry [16383 + d] for a difference d in 1/8 sample
 * An entry whose difference from ref_mv is outside -16383 .. 16383 (the reference would read outside the tables) or whose block is not inside the picture (the
 * table's builder makes none) is passed over like one outside the limits.  A job whose block_size is not 4 .. 128, whose position is negative, whose block is not
 * inside the picture, whose mib_size_log2 is outside 0 .. 16 or whose tile bounds are outside 0 .. 2^20 gets count = -1.  Whenever found = 0: best_cost = INT32_MAX,
 * best_row = best_col = 0. */
typedef struct {
    int32_t x_pos, y_pos;         /* top-left sample of the block */
    int32_t block_size;           /* 4, 8, 16, 32, 64 or 128 */
    int32_t intra;                /* 1: the entries are filtered by av1_is_dv_valid and the block itself is expected in its bucket */
    int32_t col_min, col_max, row_min, row_max;   /* x->mv_limits, whole samples */
    int32_t ref_mv_row, ref_mv_col;               /* 1/8 sample */
    int32_t error_per_bit;
    int32_t mi_row_start, mi_row_end, mi_col_start, mi_col_end;   /* xd->tile */
    int32_t mib_size_log2;        /* av1_is_dv_valid's last argument */
} SvtHipIbcSearchJob;
typedef struct {
    int32_t count;                /* the bucket's size; -1 for a job with a bad field */
    int32_t n_matched;            /* entries of equal hash_value2 */
    int32_t n_valid;              /* ... that passed av1_is_dv_valid and is_mv_in and were costed */
    int32_t found;                /* n_valid > 0 */
    int32_t best_cost, best_row, best_col;   /* best_hash_cost, best_hash_mv (whole samples) */
} SvtHipIbcSearchResult;
int svt_hip_ibc_hash_search_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_luma, int stride, int width, int height, const int32_t *d_bucket_start,
                                      const SvtHipIbcHashEntry *d_entries, const int32_t *d_mv_joint_cost, const int32_t *d_mv_comp_cost, const SvtHipIbcSearchJob *d_jobs,
                                      int njobs, SvtHipIbcSearchResult *d_results);
/* The same contracts on host pointers, serially, from the arithmetic header the kernels share (csrc/ibc_hash.h): no context and no device.  The same refusals; the
 * scratch is host memory of svt_hip_ibc_hash_scratch_bytes(width, height). */
int svt_hip_ibc_hash_table_host(int pix_bytes, int bd, const void *luma, int stride, int width, int height, int32_t *bucket_start, SvtHipIbcHashEntry *entries,
                                int64_t capacity, int32_t *info, void *scratch, size_t scratch_bytes);
int svt_hip_ibc_hash_search_host(int pix_bytes, int bd, const void *luma, int stride, int width, int height, const int32_t *bucket_start,
                                 const SvtHipIbcHashEntry *entries, const int32_t *mv_joint_cost, const int32_t *mv_comp_cost, const SvtHipIbcSearchJob *jobs, int njobs,
                                 SvtHipIbcSearchResult *results);
/* svt_av1_full_pixel_search (Encoder/Codec/av1me.c:1256-1414) whole, for a list of blocks: per job the vector intra_bc_search would put into dv_cand[], with the
 * stages' own results.  In the reference's order: full_pixel_diamond (av1me.c:578-643: svt_av1_diamond_search_sad_c, :437-573, on the sites of
 * svt_av1_init3smotion_compensation at step_param and at the later steps its num00 bookkeeping keeps, each winner re-costed by svt_av1_get_mvpred_var, then
 * svt_av1_refining_search_sad, :712-775); when exhaustive_allowed and var > ((1 << 25) >> (10 - log2(block_w / 4) - log2(block_h / 4))) << ibc_shift,
 * full_pixel_exhaustive (:650-710) over exhuastive_mesh_search (:346-435), which wins on var_ex < var; then case NSTEP's tail (:1306-1411): the hash search above
 * for a square block when use_hash, which wins on best_hash_cost < var; last the caller's av1_is_dv_valid of the final vector (Encoder/Codec/EbModeDecision.c:4523)
 * as dv_valid.  SAD is the plain sum of absolute differences and the variance svt_aom_variance{W}x{H} (bd 10: the form of svt_aom_highbd_10_variance) at every
 * format.  The mesh reproduces the reference's scan exactly, including the last column it never examines when a row of step 1 has a number of columns that is
 * no multiple of 4 (:413-429).  x->second_best_mv is not produced: nothing on this path reads it.  mv_check_bounds (EbModeDecision.c:4522) is left out: it cannot
 * fire on a vector inside limits that are a subset of the outer ones (:4479-4482).
 *   mesh_patterns : HOST int32[8], {range, interval} x 4 (sf->mesh_patterns).  An invalid FIRST pattern is the reference's `return INT_MAX`: mesh_ran = 1,
 *                   mesh_passes = 0, mesh_var = INT32_MAX, not taken.  A later pattern the walk can reach with interval < 1 or range outside 1 .. 256 refuses the call
 *   d_bucket_start, d_entries : the table, or both NULL; then a job that sets use_hash is a bad job
 * A job is bad (status -1) when its shape is not one of the 22 block sizes 4x4 .. 128x128, the block is not inside the picture, a vector inside the limits would
 * put the block outside the picture (the reference would read padding this ABI does not have), the limits reach further than 2047 whole samples from ref_mv >> 3
 * (that keeps every cost-table index within -16383 .. 16383), step_param is outside 0 .. 10, sad_per_bit or error_per_bit is negative, ibc_shift is not 0 or 1, or
 * the tile and mib_size_log2 fields fail SvtHipIbcSearchJob's rule.  Whenever status != 0 every other field is as for "nothing found": the vars INT32_MAX, hash
 * {0, 0, 0, 0, INT32_MAX, 0, 0}, all else 0.  Stream-ordered and asynchronous; a fixed number of launches whatever the data; njobs <= 2^24; d_scratch at
 * least svt_hip_ibc_full_search_scratch_bytes(njobs), 256-byte aligned. */
typedef struct {
    int32_t x_pos, y_pos, block_w, block_h;
    int32_t intra;                                  /* as SvtHipIbcSearchJob */
    int32_t col_min, col_max, row_min, row_max;     /* x->mv_limits as svt_av1_full_pixel_search sees them, whole samples */
    int32_t ref_mv_row, ref_mv_col;                 /* dv_ref, 1/8 sample */
    int32_t mvp_row, mvp_col;                       /* mvp_full, whole samples */
    int32_t step_param, sad_per_bit, error_per_bit;
    int32_t exhaustive_allowed, ibc_shift, use_hash;
    int32_t mi_row_start, mi_row_end, mi_col_start, mi_col_end, mib_size_log2;
} SvtHipIbcFullSearchJob;
typedef struct {
    int32_t status;                                 /* 0 searched; 1 empty limits (the caller's `continue`, EbModeDecision.c:4486-4490); -1 bad job */
    int32_t dia_passes, dia_refined, dia_var, dia_row, dia_col;   /* diamond passes walked, the refinement ran, full_pixel_diamond's value and vector */
    int32_t mesh_ran, mesh_passes, mesh_var, mesh_row, mesh_col;  /* the threshold let the mesh run, scans made, full_pixel_exhaustive's value and vector */
    SvtHipIbcSearchResult hash;                     /* untouched semantics; count = 0, found = 0 when the hash tail does not apply */
    int32_t source;                                 /* 0 diamond, 1 mesh, 2 hash */
    int32_t var, best_row, best_col, dv_valid;
} SvtHipIbcFullSearchResult;
size_t svt_hip_ibc_full_search_scratch_bytes(int njobs);   /* 0 for njobs < 0 */
int svt_hip_ibc_full_search_batch_dev(SvtHipCtx *ctx, int pix_bytes, int bd, const void *d_luma, int stride, int width, int height, const int32_t *d_bucket_start,
                                      const SvtHipIbcHashEntry *d_entries, const int32_t *d_mv_joint_cost, const int32_t *d_mv_comp_cost, const int32_t *mesh_patterns,
                                      const SvtHipIbcFullSearchJob *d_jobs, int njobs, SvtHipIbcFullSearchResult *d_results, void *d_scratch, size_t scratch_bytes);
/* the same on host pointers, serially, from csrc/ibc_search.h: no context, no scratch */
int svt_hip_ibc_full_search_host(int pix_bytes, int bd, const void *luma, int stride, int width, int height, const int32_t *bucket_start,
                                 const SvtHipIbcHashEntry *entries, const int32_t *mv_joint_cost, const int32_t *mv_comp_cost, const int32_t *mesh_patterns,
                                 const SvtHipIbcFullSearchJob *jobs, int njobs, SvtHipIbcFullSearchResult *results);
/* open_loop_intra_search_mb (Encoder/Codec/EbMotionEstimation.c:3043-3155, called from the motion-estimation process when the look-ahead model is on) for every
 * 16x16 macroblock of an 8-bit luma picture, one launch: neighbours from the SOURCE picture (update_neighbor_samples_array_open_loop_mb,
 * Encoder/Codec/EbEncIntraPrediction.c:1201), for mode = DC_PRED .. mode_end the edges conditioned by filter_intra_edge (Common/Codec/EbIntraPrediction.c:2545), the
 * prediction of intra_prediction_open_loop_mb (:2606), and the cost svt_aom_satd(svt_av1_wht_fwd_txfm(src - pred)) = the sum of the 256 absolute coefficients of
 * the 16x16 DCT_DCT of the residual (Encoder/Codec/EbTransforms.c:3827).  The first mode with the smallest cost wins.
 *   d_src    : sample (0, 0) of the picture; w, h multiples of 8 and at least 16; stride >= ceil16(w).  The plane must be readable over ceil16(w) x ceil16(h)
 *              samples (a trailing 8-wide / 8-high macroblock is searched as a full 16x16 block over the picture's padding, as in the reference); nothing
 *              outside that rectangle is read.
 *   mode_end : 0 .. 12 (the reference uses 0, 8, 11, 12)
 *   d_mode   : [mb_rows][mb_cols] OisMbResults.intra_mode, mb_cols = (w + 15) / 16, mb_rows = (h + 15) / 16, raster order
 *   d_cost   : [mb_rows][mb_cols] OisMbResults.intra_cost.  It fits 32 bits with room: the coefficients are 8 x an orthonormal DCT of a residual within
 *              +-255, so their absolute sum is below 16 * 8 * 255 * 16 < 2^20.
 * Stream-ordered and asynchronous: no host synchronisation, no allocation. */
int svt_hip_intra_ois_picture_dev(SvtHipCtx *ctx, const uint8_t *d_src, int stride, int w, int h, int mode_end, uint8_t *d_mode, int32_t *d_cost);

/* ------------------------------------------------------------------ TPL flow dispenser ------------------------------------------------------
 * tpl_mc_flow_dispenser (Encoder/Codec/EbRateControlProcess.c:344-816) for one picture of the look-ahead window: for every 16x16 macroblock the inter cost
 * (SATD of the 16x16 DCT_DCT of source - reference SOURCE at the ME vector) of every valid reference slot, the decision against the open-loop intra cost,
 * svt_av1_quantize_fp + svt_av1_block_error + rate_estimator of the winning residual, the reconstruction (copy from the reference's reconstruction, or intra
 * prediction from this picture's reconstruction, plus the inverse transform of the quantised residual), the second set of costs against that reconstruction,
 * what result_model_store writes, and generate_padding of the reconstruction.  Inter macroblocks depend on no other macroblock of the picture and run in one
 * launch; intra macroblocks read their left / above / above-left neighbours (and in column 0 the above-right one) and run in steps x + 2y, one launch per step.
 *   refs[r]    : slot r = rf_idx of the reference's loop (0..3 list 0, 4..6 list 1); d_src == NULL = slot unused (tpl_ref0_count / tpl_ref1_count)
 *   d_mv       : [7][n_mb] the ME vector of the macroblock's 16x16 PU per slot, (y_mv << 16) | (x_mv & 0xffff) in quarter samples as the ME kernels write it;
 *                the block offset is (int16_t)(x_mv << 1) >> 3.  Only the rows of used slots are read.  n_mb = mb_cols * mb_rows, raster order.
 *   d_ref_mask : [n_mb] bit r = is_me_data_valid for slot r.  d_mv and d_ref_mask may be NULL only when no slot is used.
 *   d_ois_mode / d_ois_cost : the outputs of svt_hip_intra_ois_picture_dev on d_cur (may be NULL when use_ois == 0); a mode above 12 is treated as DC_PRED
 *   d_cur      : sample (0,0) of the source luma, readable over ceil16(w) x ceil16(h)
 *   d_recon    : sample (0,0) of this picture's TPL reconstruction: ceil16(w) x ceil16(h) is written, then the `pad` border around w x h is replicated.
 *                Must not alias any d_rec.  Nothing outside (w + 2 pad) x (h + 2 pad) is written.
 *   d_stats    : [n_mb]
 *   d_scratch  : svt_hip_tpl_dispenser_scratch_bytes(w, h) bytes
 * A block an MV would move outside the padded reference is clamped to [-pad, w + pad - 16] x [-pad, h + pad - 16] (the reference has no defined result there).
 * 8-bit only (the reference runs TPL on the 8-bit pictures at every encoder bit depth).  Stream-ordered and asynchronous: no host synchronisation, no
 * allocation, no read-back. */
typedef struct {
    const uint8_t *d_src;     /* sample (0,0) of this reference's SOURCE luma: read by the cost search */
    const uint8_t *d_rec;     /* sample (0,0) of the picture the reconstruction copies from: that frame's TPL reconstruction when it is inside the sliding
                                 window, else the same pointer as d_src */
    int32_t src_stride, rec_stride;
} SvtHipTplRef;

typedef struct {
    int32_t w, h;             /* luma size: multiples of 8, >= 16 */
    int32_t pad;              /* valid border, in samples, around every reference plane and around d_recon (which receives it); >= 16 */
    SvtHipQuantParams q;      /* variant 2, log_scale 0: round = y_round_fp, quant = y_quant_fp, dequant = y_dequant_qtx of the picture's qindex */
    uint8_t use_ois;          /* 1 = intra mode / cost from d_ois_*; 0 = DC_PRED with cost INT64_MAX */
    uint8_t add_residual;     /* 1 = inverse transform added where eob != 0 */
    uint8_t rate;             /* !tpl_opt_flag: 0 = both rates are 0 */
    uint8_t best_ref_only;    /* tpl_ctrls.get_best_ref: only the valid slot with the smallest 16x16 SAD is evaluated (get_best_reference) */
} SvtHipTplParams;

typedef struct {              /* what result_model_store writes for the macroblock: already divided by 16 and clamped to >= 1 */
    int64_t srcrf_dist, recrf_dist, srcrf_rate, recrf_rate;
    int16_t mv_row, mv_col;   /* TplStats.mv of the best reference (y_mv << 1, x_mv << 1), 0 when rf_idx == -1 */
    int8_t  rf_idx;           /* best_rf_idx, -1 when no reference was evaluated (also set when intra won) */
    uint8_t is_inter;         /* best_mode == NEWMV */
    uint8_t mode;             /* the intra mode used when !is_inter */
    uint8_t pad0;
    uint16_t eob;             /* of the final (reconstruction) pass */
    uint16_t pad1;
} SvtHipTplMbStats;

size_t svt_hip_tpl_dispenser_scratch_bytes(int w, int h);
int svt_hip_tpl_dispenser_picture_dev(SvtHipCtx *ctx, const SvtHipTplParams *p, const uint8_t *d_cur, int cur_stride,
                                      const SvtHipTplRef refs[7], const uint32_t *d_mv, const uint8_t *d_ref_mask,
                                      const uint8_t *d_ois_mode, const int32_t *d_ois_cost,
                                      uint8_t *d_recon, int recon_stride, SvtHipTplMbStats *d_stats, void *d_scratch);
/* Measurement only (tools/tpl_time.py): which parts svt_hip_tpl_dispenser_picture_dev launches, bit 0 = phase A (inter search, decisions, inter macroblocks),
 * bit 1 = phase B (the intra steps), bit 2 = the padding.  The default, 7, is the only value that computes the dispenser. */
int svt_hip_tpl_set_phases(SvtHipCtx *ctx, int mask);

/* ------------------------------------------------------------------ TPL flow synthesizer, r0 / beta / lambda factors -------------------------
 * The rest of tpl_mc_flow (Encoder/Codec/EbRateControlProcess.c:1154-1197) after the dispenser, on the records the dispenser left on the device:
 * tpl_mc_flow_synthesizer -> tpl_model_update -> tpl_model_update_b (:887-998) for every picture of the sliding window, last picture first, then
 * generate_r0beta (:1000-1075) with generate_lambda_scaling_factor (:39-84) on the window's first picture.  The accumulators TplStats.mc_dep_rate and
 * mc_dep_dist are int64_t (Encoder/Codec/EbCodingUnit.h:421-430) and every scatter adds an integer computed from the scattering block alone (:940-944), so
 * 64-bit atomic adds give the reference's sums in any order; the floating point is per block (:911-914, :73-79, :1020-1022, :1065-1071) and IEEE exact.
 *
 * Grid.  cell_log2 is 4 (the reference's is_720p_or_larger, min(w, h) >= 720: EbPictureControlSet.c:1252) or 3; s = 4 - cell_log2.  A picture's grid is
 * [mb_rows << s][mb_cols << s] cells (mb_cols = (w + 15) / 16, mb_rows = (h + 15) / 16: the reference's mi_cols_sr >> shift stride), a cell is
 * int64_t[2] = {mc_dep_rate, mc_dep_dist}; svt_hip_tpl_dep_bytes(w, h, cell_log2) is its size (0 for arguments the entry points refuse).  The other TplStats
 * fields of a cell are those of its macroblock's SvtHipTplMbStats record (result_model_store replicates them, :130-161).
 *
 * Source blocks.  One per cell: a macroblock, or each of its four 8x8 quarters (the quarters past mi_rows / mi_cols of a trailing half macroblock too, as
 * the reference's loops at :966-967 run them).  A block reads its macroblock's record and the mc_dep_* of ITS OWN cell, moves by GET_MV_RAWPEL of the
 * record's vector (Common/Codec/EbBlockStructures.h:41-60) and adds into the up to four cells of the target picture it overlaps (round_floor, :847-855; a
 * target cell is accepted only inside the aligned picture, 0 <= row < h and 0 <= col < w in samples, :927-928).
 *   rf_idx == -1: the reference's ref_frame_poc keeps its memset value 0 with a zero vector (:579, :795-798): the target is ref_window[0] and the record's
 *                 vector is not read.  rf_idx outside -1 .. 6: no target.
 *   recrf_dist == 0: the reference divides by zero; here the propagated part mc_dep_dist' is 0.  A double outside int64_t converts to INT64_MIN, NaN to 0.
 *
 * rate must be 0 (the reference's tpl_opt_flag == 1): delta_rate_cost (:857-883) goes through libm's log and pow on doubles and is not built; mc_dep_rate'
 * is 0, the records' recrf_rate - srcrf_rate is still scattered and the full RDCOST (EbRateDistortionCost.h:104-107) is still evaluated.
 *
 * Stream-ordered and asynchronous: no host synchronisation, no allocation, no read-back.  The frame descriptors are host memory, read during the call. */
#define SVT_HIP_TPL_MAX_WINDOW 60   /* MAX_TPL_LA_SW */

typedef struct {
    const SvtHipTplMbStats *d_stats;   /* [n_mb] the dispenser's records of this picture */
    int64_t *d_dep;                    /* this picture's grid, svt_hip_tpl_dep_bytes(w, h, cell_log2) bytes; no two pictures share one */
    int32_t on;                        /* the reference's tpl_on (:1182-1191): 0 = not synthesized, d_stats is never read as a source; still a target */
    int32_t ref_window[8];             /* [rf_idx + 1] = window index of the picture that slot names (the first i with picture_number == the slot's POC,
                                          :972-976), -1 = not in the window.  Entry 0 serves rf_idx == -1: the index of the picture whose picture_number is
                                          0; it may be this picture's own index (the zero vector then adds into the block's own cell only).  An entry
                                          1..7 equal to this picture's own index is refused: the result would depend on the order of the blocks. */
    int32_t reserved;
} SvtHipTplWindowFrame;

typedef struct {
    int32_t w, h;                      /* luma size: multiples of 8, >= 16 */
    int32_t cell_log2;                 /* 4 or 3 */
    int32_t sb_size;                   /* 64 or 128 */
    int32_t base_rdmult;               /* pcs->base_rdmult, >= 0 */
    int32_t rate;                      /* must be 0 */
    double r0_in;                      /* pcs->r0 before the call: kept when mc_dep_cost_base == 0 (:1020-1022) */
} SvtHipTplSynthParams;

typedef struct {                       /* the head of d_out */
    double r0;
    int64_t intra_cost_base, mc_dep_cost_base;   /* the reference's DEBUG_TPL values (:1023-1030) */
} SvtHipTplR0BetaHeader;

size_t svt_hip_tpl_dep_bytes(int w, int h, int cell_log2);
/* d_out: SvtHipTplR0BetaHeader, then double factors[mb_rows * mb_cols] (tpl_rdmult_scaling_factors), then double beta[sb_rows * sb_cols] (tpl_beta),
 * sb_cols = (w + sb_size - 1) / sb_size.  0 for arguments the entry points refuse. */
size_t svt_hip_tpl_r0beta_out_bytes(int w, int h, int sb_size);
size_t svt_hip_tpl_r0beta_scratch_bytes(void);
/* The scatter of window picture frame_idx (tpl_mc_flow_synthesizer(pcs_array, frame_idx, frames_in_sw)); nothing is launched when that picture is off. */
int svt_hip_tpl_synth_picture_dev(SvtHipCtx *ctx, const SvtHipTplSynthParams *params, const SvtHipTplWindowFrame *frames, int n_frames, int frame_idx);
/* generate_r0beta on one picture: d_stats its records (only recrf_dist is read; the reference has zeros there for a picture that is off), d_dep its grid. */
int svt_hip_tpl_r0beta_dev(SvtHipCtx *ctx, const SvtHipTplSynthParams *params, const SvtHipTplMbStats *d_stats, const int64_t *d_dep, void *d_out,
                           void *d_scratch);
/* The whole window: every grid zeroed (:1159-1163), the scatters of pictures n_frames - 1 .. 0 that are on, generate_r0beta on picture 0.  Every grid stays
 * on the device. */
int svt_hip_tpl_window_dev(SvtHipCtx *ctx, const SvtHipTplSynthParams *params, const SvtHipTplWindowFrame *frames, int n_frames, void *d_out, void *d_scratch);
/* The same contract on host pointers (d_stats, d_dep and out are host memory), serial, no context. */
int svt_hip_tpl_window_host(const SvtHipTplSynthParams *params, const SvtHipTplWindowFrame *frames, int n_frames, void *out);

/* ------------------------------------------------------------------ global motion: warp error and parameter refinement -----------------------
 * The source-only arithmetic of compute_global_motion (Encoder/Codec/EbGlobalMotionEstimation.c:171-405) after the model fit: the warp error of
 * integer models and the coordinate descent over their parameters.  8-bit luma, no subsampling (the reference calls this path with EB_8BIT only, :339-340).
 * Planes: d_* points at sample (0, 0), any stride >= width, any base offset; width and height >= 8, not necessarily multiples of 8; nothing outside
 * [0, width) x [0, height) of a plane is read (the warp clamps to the reference plane's edges as the reference does).  The source is w x h; a reference
 * plane has its own width / height / stride (they bound the clamp; the error is always summed over the source's w x h).
 * Corner detection, the correspondence search and the RANSAC model fit have device forms too (the svt_hip_gm_corners / cross_correlation / correspondences /
 * svt_hip_gm_fit entry points below); the decision loop with gm_get_params_cost / svt_av1_is_enough_erroradvantage is host arithmetic
 * (svt_hip_gm_decide_host); only the high-bit-depth twins stay on the host. */
typedef struct {
    int32_t mat[6];                     /* EbWarpedMotionParams::wmmat[0..5] as svt_warp_plane uses them */
    int16_t alpha, beta, gamma, delta;  /* its shear parameters */
    int32_t valid;                      /* what svt_get_shear_params returned; 0 = the warp error is 1 and nothing is warped */
} SvtHipGmModel;
typedef struct {
    const uint8_t *d_plane;
    int32_t width, height, stride, reserved;
} SvtHipGmRef;
typedef struct {
    int32_t ref;                        /* index into the table of reference planes */
    int32_t wmtype;                     /* 0 IDENTITY (initial error only), 1 TRANSLATION, 2 ROTZOOM, 3 AFFINE */
    int32_t wmmat[8];
    int32_t n_refinements;              /* 0 .. SVT_HIP_GM_MAX_REFINEMENTS; 0 = initial error only */
    int32_t reserved;
    int64_t best_frame_error;           /* INT64_MAX = none */
} SvtHipGmJob;
typedef struct {
    int32_t wmmat[8];                   /* after the final force_wmtype */
    int32_t wmtype;                     /* get_wmtype of them; -1 = the job was refused (ref / wmtype / n_refinements out of range), nothing else is set */
    int32_t probes;                     /* warp errors the reference evaluates on this walk (what the replay consumed, not what speculation computed) */
    int64_t best_error;
    int32_t rounds;                     /* device rounds (error launch + step launch) the job took */
    int32_t invalid_probes;             /* of `probes`, how many had invalid shear parameters (error 1) */
} SvtHipGmResult;
#define SVT_HIP_GM_MAX_REFS 8
#define SVT_HIP_GM_MAX_REFINEMENTS 12
#define SVT_HIP_GM_MAX_DIM 16384
#define SVT_HIP_GM_MAX_MODELS (1 << 20)
#define SVT_HIP_GM_MAX_JOBS 1024
#define SVT_HIP_GM_MAX_CORNERS 4096

/* svt_get_shear_params (Common/Codec/EbWarpedMotion.c:921-950, with is_affine_valid :359, is_affine_shear_allowed :364 and the divisor of :343-357) of n
 * models: d_wmmat = n x int32[6]; d_out[i] = {the six parameters, alpha .. delta after the 6-bit reduction, valid}.  alpha .. delta are 0 when wmmat[2] <= 0
 * (the reference leaves them untouched there). */
int svt_hip_gm_shear_params_batch_dev(SvtHipCtx *ctx, const int32_t *d_wmmat, int n, SvtHipGmModel *d_out);
/* svt_av1_warp_error(wm, 0, 8, ref, ..., src, 0, 0, w, h, src_stride, 0, 0, INT64_MAX) (Encoder/Codec/EbEncWarpedMotion.c:171-211, :227-264) of n models over
 * one picture in one launch: d_err[i] = the sum of error_measure_lut over the source against the reference warped in 32x32 blocks; 1 where !valid. */
int svt_hip_gm_warp_error_batch_dev(SvtHipCtx *ctx, const uint8_t *d_src, int src_stride, int w, int h, const uint8_t *d_ref, int ref_width, int ref_height,
                                    int ref_stride, const SvtHipGmModel *d_models, int n, int64_t *d_err);
/* svt_av1_frame_error(0, 8, ref, stride, src, w, h, src_stride) = svt_av1_calc_frame_error_c (EbEncWarpedMotion.c:160-169, :213-225), the ref_frame_error of
 * compute_global_motion (EbGlobalMotionEstimation.c:376), of n_refs <= 8 planes against the source; refs is a host array, width / height are not used. */
int svt_hip_gm_frame_error_batch_dev(SvtHipCtx *ctx, const uint8_t *d_src, int src_stride, int w, int h, const SvtHipGmRef *refs, int n_refs, int64_t *d_err);
/* svt_av1_refine_integerized_param (Encoder/Codec/global_motion.c:135-259) of njobs walks in lockstep: rounds of one warp-error launch over every job's
 * current batch of speculated candidates and one launch that replays the reference's comparisons and writes the next batches; the host polls one counter
 * per chunk of rounds (it synchronises the stream).  refs is a host array of n_refs <= 8 planes; d_jobs / d_results live in device memory; d_scratch holds
 * svt_hip_gm_refine_scratch_bytes(njobs) bytes.  *polls_out (may be NULL) = how many times the host read the counter.  docs/kernels/gm.md. */
size_t svt_hip_gm_refine_scratch_bytes(int njobs);
int svt_hip_gm_refine_picture_dev(SvtHipCtx *ctx, const uint8_t *d_src, int src_stride, int w, int h, const SvtHipGmRef *refs, int n_refs,
                                  const SvtHipGmJob *d_jobs, int njobs, SvtHipGmResult *d_results, void *d_scratch, int *polls_out);
/* The error table the three kernels use, min(16384, floor(16384 (|i - 255| / 255)^0.7 + 0.5)), i = 0..511 (host; needs no device). */
int svt_hip_gm_error_table(uint16_t out[512]);

/* The front half of compute_global_motion_feature_based (Encoder/Codec/global_motion.c:274-320): corners and correspondences, bit for bit; the model fit
 * (svt_hip_gm_fit_batch_dev) takes the correspondence lists where they are.
 * Lists and counts live in device memory: the kernels clamp a count to [0, max_points] and pass every coordinate, any int,
 * through the reference's eligibility tests before it becomes an address.
 *
 * svt_av1_fast_corner_detect (Encoder/Codec/corner_detect.c:19-32: FAST-9 at barrier 18, third_party/fastfeat/fast_9.c, the score of :8-2937, the non-maximum
 * suppression of nonmax.c:8-119) of n_planes <= 1 + SVT_HIP_GM_MAX_REFS planes, each of its own size, in one call.  planes is a host array.
 * d_points[p][max_points][2] = x, y of the first max_points kept corners of plane p in raster order (the reference's truncation); d_counts[p] = min(kept,
 * max_points); d_kept[p] (may be NULL) = kept before the truncation.  d_scratch holds svt_hip_gm_corners_scratch_bytes(planes, n_planes) bytes (0 = the planes
 * would be refused), 8-byte aligned. */
size_t svt_hip_gm_corners_scratch_bytes(const SvtHipGmRef *planes, int n_planes);
int svt_hip_gm_corners_batch_dev(SvtHipCtx *ctx, const SvtHipGmRef *planes, int n_planes, int max_points, int32_t *d_points, int32_t *d_counts, int32_t *d_kept,
                                 void *d_scratch);
/* svt_av1_compute_cross_correlation_c (Encoder/Codec/corner_match.c:43-64) of n point pairs: d_pairs[i] = x1, y1, x2, y2; d_out[i] = cov / sqrt(var2) of the 13x13
 * windows centred there, the reference's double (NaN where window 2 is flat).  Both planes are w x h.  A pair either of whose windows does not lie inside
 * (6 <= x < w - 6, 6 <= y < h - 6) is not read and gets 0.0. */
int svt_hip_gm_cross_correlation_batch_dev(SvtHipCtx *ctx, const uint8_t *d_im1, int stride1, const uint8_t *d_im2, int stride2, int w, int h, const int32_t *d_pairs,
                                           int n, double *d_out);
/* svt_av1_determine_correspondence (Encoder/Codec/corner_match.c:151-212, with improve_correspondence :78-149) of one source against n_refs <= 8 references.
 * d_src_points / d_src_count: one plane's list and count as svt_hip_gm_corners_batch_dev writes them; d_ref_points[n_refs][max_points][2] / d_ref_counts[n_refs]
 * likewise, so the two calls chain on one stream with no host round trip.  refs is a host array; every plane is read as w x h, the source's size, as the reference
 * does (width / height of a table entry are not used; stride >= w).  d_corr[r][max_points][4] = x, y, rx, ry of the d_ncorr[r] correspondences, in the source
 * list's order; the rest of d_corr[r] is unspecified. */
int svt_hip_gm_correspondences_batch_dev(SvtHipCtx *ctx, const uint8_t *d_src, int src_stride, int w, int h, const int32_t *d_src_points, const int32_t *d_src_count,
                                         const SvtHipGmRef *refs, int n_refs, const int32_t *d_ref_points, const int32_t *d_ref_counts, int max_points,
                                         int32_t *d_corr, int32_t *d_ncorr);

/* The model fit: ransac() (Encoder/Codec/ransac.c:359-542, reached through svt_av1_get_ransac_type :779-786, with least_squares / linsolve of
 * Encoder/Codec/mathutils.h:26-111 and lcg_rand16 of random.h:20-23), svt_av1_convert_model_to_params (Encoder/Codec/global_motion.c:41-86) and the
 * MIN_INLIER_PROB rule (global_motion.c:310-318), one workgroup per job, bit for bit: every operation is an IEEE double in the reference's order
 * (svt-av1_amd/csrc/gm_fit.h; docs/kernels/gm.md "The fit").  A job fits one model type to one correspondence list.
 *   d_corr[n_lists][max_points][4], d_ncorr[n_lists] : as svt_hip_gm_correspondences_batch_dev writes them (device memory); a count is clamped to [0, max_points]
 *   jobs       : host array of njobs <= SVT_HIP_GM_FIT_MAX_JOBS; ref = the list (and the reference plane of the refinement job), 0 <= ref < n_lists;
 *                type = 1 TRANSLATION, 2 ROTZOOM, 3 AFFINE
 *   num_motions: must be 1 (RANSAC_NUM_MOTIONS; the reference's qsort of equal motions is unspecified beyond that)
 *   d_fits[njobs], d_inliers[njobs][max_points] (may be NULL: the indices of the kept motion's inliers, the first num_inliers entries are specified when
 *   num_inliers >= 3), d_refine_jobs[njobs] (may be NULL): what svt_hip_gm_refine_picture_dev reads: ref, wmtype / wmmat of the converted model, n_refinements,
 *   best_frame_error = INT64_MAX; wmtype = -1 where compute_global_motion would not refine (no inliers after the rule, or an IDENTITY model:
 *   EbGlobalMotionEstimation.c:331-335), which the refinement finishes at once with result wmtype -1.
 *   d_scratch  : svt_hip_gm_fit_scratch_bytes(njobs, max_points) bytes, 8-byte aligned
 * ret = 1 with num_inliers = 0 and identity params: fewer than 15 points, a draw degenerate more than 10 times in one trial.  A kept motion of 2 inliers
 * reports its count and identity params (the reference recomputes from 3 inliers on).  params = the identity the reference's caller stores first
 * (EbGlobalMotionEstimation.c:308-313) wherever the fit writes none.  A parameter whose scaled value leaves int32 has no defined conversion in the reference;
 * here it is clamped in double first, and such models are outside the contract.  The *_double_prec variants are not built.
 * Stream-ordered and asynchronous: no host synchronisation, no allocation. */
typedef struct {
    int32_t ref;                        /* index of the correspondence list = of the reference plane */
    int32_t type;                       /* 1 TRANSLATION, 2 ROTZOOM, 3 AFFINE */
} SvtHipGmFitJob;
typedef struct {
    int32_t ret;                        /* what the fit function returns */
    int32_t npoints;                    /* the list's count after the clamp */
    int32_t num_inliers;                /* num_inliers_by_motion[0] as the fit reports it */
    int32_t num_inliers_kept;           /* after the MIN_INLIER_PROB rule: 0 = compute_global_motion ignores the motion */
    double  params[8];                  /* MotionModel::params */
    int32_t wmmat[8];                   /* svt_av1_convert_model_to_params of them */
    int32_t wmtype;
    int32_t reserved;
} SvtHipGmFit;
#define SVT_HIP_GM_FIT_MAX_JOBS 64
size_t svt_hip_gm_fit_scratch_bytes(int njobs, int max_points);
int svt_hip_gm_fit_batch_dev(SvtHipCtx *ctx, const int32_t *d_corr, const int32_t *d_ncorr, int n_lists, int max_points, const SvtHipGmFitJob *jobs, int njobs,
                             int num_motions, int n_refinements, SvtHipGmFit *d_fits, int32_t *d_inliers, SvtHipGmJob *d_refine_jobs, void *d_scratch);

/* The decision of compute_global_motion (Encoder/Codec/EbGlobalMotionEstimation.c:303-399) for one reference picture, replayed from per-model records: the loop
 * over ROTZOOM, AFFINE (ROTZOOM only when rotzoom_model_only) with ONE global_motion that persists across iterations: svt_get_shear_params resets an invalid
 * model, a TRANSLATION result is rewritten by convert_to_trans_prec, IDENTITY and ref_frame_error == 0 `continue` (without resetting the model),
 * svt_av1_is_enough_erroradvantage((double)best / ref_frame_error, gm_get_params_cost(model, default, allow_high_precision_mv), GM_ERRORADV_TR_0) decides, a
 * non-identity model ends the loop.  models[0] = ROTZOOM's record, models[1] = AFFINE's (not read when rotzoom_model_only).  Needs no device. */
typedef struct {
    int32_t num_inliers_kept;           /* SvtHipGmFit::num_inliers_kept: 0 = the motion is skipped */
    int32_t fit_wmtype;                 /* SvtHipGmFit::wmtype: 0 = not refined */
    int32_t wmmat[8];                   /* SvtHipGmResult::wmmat of the refinement */
    int32_t wmtype;                     /* SvtHipGmResult::wmtype (-1 = not refined) */
    int32_t reserved;
    int64_t best_error;                 /* SvtHipGmResult::best_error */
} SvtHipGmModelRecord;
/* gm_get_params_cost(gm, &default_warp_params, allow_hp) (Encoder/Codec/EbGlobalMotionEstimationCost.c:17-75 with svt_aom_count_primitive_refsubexpfin) */
int svt_hip_gm_params_cost_host(const int32_t wmmat[8], int wmtype, int allow_high_precision_mv);
int svt_hip_gm_decide_host(const SvtHipGmModelRecord models[2], int64_t ref_frame_error, int rotzoom_model_only, int allow_high_precision_mv,
                           int32_t wmmat_out[8], int32_t *wmtype_out);

/* compute_global_motion (Encoder/Codec/EbGlobalMotionEstimation.c:262-405) of one source against n_refs <= 8 references in one call, on one stream: corners of
 * the source and of every reference (one call), correspondences (one call), the ROTZOOM and, unless rotzoom_model_only, AFFINE fit of every reference (one
 * launch), the refinement of all the jobs that launch wrote (svt_hip_gm_refine_picture_dev: its poll of the done counter is the only synchronisation before the
 * end), the frame errors, one download, svt_hip_gm_decide_host.  The AFFINE fit and walk are speculated: the reference runs them only when ROTZOOM ends as
 * IDENTITY; they depend on nothing the ROTZOOM iteration computes, and the decision discards them when the loop would have ended.  Corners and
 * correspondences are found once per reference (the reference finds the same ones once per model type).
 * A reference plane is read over the source's w x h for corners, correspondences and the frame error (so it must be at least that large) and clamps the warp
 * to its own width x height.  results = host array of n_refs records.  d_scratch: svt_hip_gm_estimate_scratch_bytes bytes (0 = the arguments would be refused),
 * 256-byte aligned.  8-bit only.  Not part of this call: the level / list / identity-exit logic of global_motion_estimation (:186-245). */
typedef struct {
    int32_t rotzoom_model_only;         /* gm_ctrls.rotzoom_model_only */
    int32_t allow_high_precision_mv;
    int32_t n_refinements;              /* the reference uses 5 */
    int32_t max_points;                 /* 1 .. SVT_HIP_GM_MAX_CORNERS; the reference uses MAX_CORNERS = 4096 */
} SvtHipGmEstimateOptions;
typedef struct {
    int32_t wmmat[8];                   /* *bestWarpedMotion */
    int32_t wmtype;
    int32_t num_correspondences;
    int32_t n_models;                   /* 1 (ROTZOOM) or 2 (ROTZOOM, AFFINE): how many entries of fits / models are set */
    int32_t reserved;
    int64_t ref_frame_error;
    SvtHipGmFit fits[2];                /* what the decision consumed, per model type */
    SvtHipGmModelRecord models[2];
} SvtHipGmEstimate;
size_t svt_hip_gm_estimate_scratch_bytes(int w, int h, int n_refs, const SvtHipGmEstimateOptions *options);
int svt_hip_gm_estimate_picture_dev(SvtHipCtx *ctx, const uint8_t *d_src, int stride, int w, int h, const SvtHipGmRef *refs, int n_refs,
                                    const SvtHipGmEstimateOptions *options, SvtHipGmEstimate *results, void *d_scratch);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SVT_HIP_H */
