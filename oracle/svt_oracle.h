/*
 * svt_oracle.h — CPU restatement ("port") of the SVT-AV1 v0.8.6 per-superblock hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is part of the shipped product path: only
 * tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library, and there
 * only as the checker.  The product (svt-av1_amd/csrc) never links or calls it.
 *
 * Parity status: PINNED.  Every function here is checked bit-for-bit against the reference's own
 * C functions (oracle/_ref/libsvtav1_ref.so, built by oracle/Makefile.ref from the sources under
 * /root/reference) by tests/test_oracle_vs_ref.py on the reference unit tests' input
 * distributions, and against the committed fixtures in tests/golden/ generated from that library
 * by tests/golden/make_golden.py.
 *
 * All citations are file:line under /root/reference/Source/Lib.
 */
#ifndef SVT_ORACLE_H
#define SVT_ORACLE_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ORC_SQUARE_PU_COUNT 85 /* Encoder/Codec/EbMotionEstimationLcuResults.h:22 */
#define ORC_MAX_SAD_VALUE (128 * 128 * 255) /* Encoder/Codec/EbMotionEstimation.h:93 */

/* ---------------------------------------------------------------- ME: SAD kernels ------------ */
/* Encoder/C_DEFAULT/EbComputeSAD_C.c:20  (svt_fast_loop_nxm_sad_kernel / svt_nxm_sad_kernel) */
uint32_t orc_nxm_sad(const uint8_t *src, uint32_t src_stride, const uint8_t *ref, uint32_t ref_stride,
                     uint32_t height, uint32_t width);
/* Encoder/C_DEFAULT/EbComputeSAD_C.c:39 (sad_16b_kernel_c) */
uint32_t orc_sad_16b(const uint16_t *src, uint32_t src_stride, const uint16_t *ref, uint32_t ref_stride,
                     uint32_t height, uint32_t width);
/* Encoder/C_DEFAULT/EbComputeSAD_C.c:58 (svt_sad_loop_kernel_c) */
void orc_sad_loop(const uint8_t *src, uint32_t src_stride, const uint8_t *ref, uint32_t ref_stride,
                  uint32_t block_height, uint32_t block_width, uint64_t *best_sad, int16_t *x_center,
                  int16_t *y_center, uint32_t src_stride_raw, int16_t sa_width, int16_t sa_height);
/* Encoder/Codec/EbMotionEstimation.c:362 (svt_ext_all_sad_calculation_8x8_16x16_c) */
void orc_ext_all_sad_8x8_16x16(const uint8_t *src, uint32_t src_stride, const uint8_t *ref,
                               uint32_t ref_stride, uint32_t mv, uint32_t *best_sad8, uint32_t *best_sad16,
                               uint32_t *best_mv8, uint32_t *best_mv16, uint32_t eight_sad16[16][8],
                               uint32_t eight_sad8[64][8], int sub_sad);
/* Encoder/Codec/EbMotionEstimation.c:396 (svt_ext_eight_sad_calculation_32x32_64x64_c) */
void orc_ext_eight_sad_32x32_64x64(uint32_t sad16[16][8], uint32_t *best_sad32, uint32_t *best_sad64,
                                   uint32_t *best_mv32, uint32_t *best_mv64, uint32_t mv,
                                   uint32_t sad32[4][8]);
/* Encoder/Codec/EbMotionEstimation.c:122 (svt_ext_sad_calculation_8x8_16x16_c) */
void orc_ext_sad_8x8_16x16(const uint8_t *src, uint32_t src_stride, const uint8_t *ref, uint32_t ref_stride,
                           uint32_t *best_sad8, uint32_t *best_sad16, uint32_t *best_mv8,
                           uint32_t *best_mv16, uint32_t mv, uint32_t *sad16, uint32_t *sad8, int sub_sad);
/* Encoder/Codec/EbMotionEstimation.c:191 (svt_ext_sad_calculation_32x32_64x64_c) */
void orc_ext_sad_32x32_64x64(const uint32_t *sad16, uint32_t *best_sad32, uint32_t *best_sad64,
                             uint32_t *best_mv32, uint32_t *best_mv64, uint32_t mv, uint32_t *sad32);

/* Encoder/Codec/EbMotionEstimation.c:814 (open_loop_me_fullpel_search_sblock) + the best-SAD
 * initialisation of integer_search_sb (:2086).  `ref_tl` points at the reference sample of the
 * top-left candidate (x_sa_origin, y_sa_origin relative to the SB); outputs use the 85-PU layout
 * of EbMeTierZeroPu (Encoder/Codec/EbMotionEstimationContext.h:51-137). */
void orc_me_fullpel_sb(const uint8_t *src, uint32_t src_stride, const uint8_t *ref_tl, uint32_t ref_stride,
                       int x_sa_origin, int y_sa_origin, uint32_t sa_width, uint32_t sa_height, int sub_sad,
                       uint32_t best_sad[ORC_SQUARE_PU_COUNT], uint32_t best_mv[ORC_SQUARE_PU_COUNT]);

/* Search-window arithmetic of integer_search_sb, Encoder/Codec/EbMotionEstimation.c:1922-2066
 * (unrestricted-MV branch, int16 arithmetic, 63-px pad).  In/out: sa_w, sa_h (already scaled by the
 * temporal-distance factor and divisor, :1930-1936), centre -> origin. */
typedef struct {
    int16_t x_origin, y_origin; /* search-area origin relative to the SB origin */
    int16_t width, height;      /* adjusted search area */
} OrcSearchWindow;
OrcSearchWindow orc_me_search_window(int sb_origin_x, int sb_origin_y, int x_center, int y_center,
                                     int sa_width, int sa_height, int pic_width, int pic_height);

/* dlf_oracle.c, E2: edges, filter lengths and levels of a frame (set_lpf_parameters, EbDeblockingFilter.c:168-319) */
int  orc_block_width(int bsize);
int  orc_block_height(int bsize);
void orc_tx_dims_for_depth(int bsize, int depth, int *tw, int *th);
void orc_uv_tx_dims(int bsize, int *tw, int *th);
void orc_dlf_level_table(const int32_t *lf, uint8_t lvl[3][2][8][2]);
void orc_dlf_mode_info_summary(int n_units, const uint8_t *sb_type, const uint8_t *tx_depth, const uint8_t *ref_frame0, const uint8_t *skip, const uint8_t *mode,
                               const uint8_t lvl[3][2][8][2], uint8_t *out);
int  orc_dlf_filtered_units(int coded_luma, int pad, int sb_size, int ss);
void orc_dlf_build_edges(const uint8_t *mi, int mi_cols, int mi_rows, int plane, int ss_x, int ss_y, int pw, int ph, int filt_units_w, int filt_units_h,
                         uint16_t *edges_v, uint16_t *edges_h);
/* md_oracle.c: mode decision stage 0, full-pel single-reference candidates (fast_loop_core, EbProductCodingLoop.c:907) */
uint32_t orc_md_fullpel_candidate(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, int x, int y, int w, int h, int mx, int my);
void orc_md_fullpel_sad_picture(const uint8_t *src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const uint8_t (*pus)[4], int n_refs,
                                const uint8_t *const *refs, const int *ref_stride, const int (*ref_box)[4], const uint32_t *mv, uint32_t *sad);
uint32_t orc_md_fullpel_avg_candidate(const uint8_t *src, int src_stride, const uint8_t *ref0, int ref0_stride, const uint8_t *ref1, int ref1_stride, int x, int y, int w, int h,
                                      int mx0, int my0, int mx1, int my1);
void orc_md_fullpel_avg_sad_picture(const uint8_t *src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const uint8_t (*pus)[4], int n_refs,
                                    const uint8_t *const *refs, const int *ref_stride, const int (*ref_box)[4], const uint32_t *mv, int n_pairs, const uint8_t (*pairs)[2],
                                    uint32_t *sad);
uint32_t orc_md_fullpel_candidate16(const uint16_t *src, int src_stride, const uint16_t *ref, int ref_stride, int x, int y, int w, int h, int mx, int my);
uint32_t orc_md_fullpel_avg_candidate16(const uint16_t *src, int src_stride, const uint16_t *ref0, int ref0_stride, const uint16_t *ref1, int ref1_stride, int x, int y, int w,
                                        int h, int mx0, int my0, int mx1, int my1, int bd);
void orc_md_fullpel_sad_picture16(const uint16_t *src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const uint8_t (*pus)[4], int n_refs,
                                  const uint16_t *const *refs, const int *ref_stride, const int (*ref_box)[4], const uint32_t *mv, uint32_t *sad);
void orc_md_fullpel_avg_sad_picture16(const uint16_t *src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const uint8_t (*pus)[4], int n_refs,
                                      const uint16_t *const *refs, const int *ref_stride, const int (*ref_box)[4], const uint32_t *mv, int n_pairs, const uint8_t (*pairs)[2],
                                      int bd, uint32_t *sad);
uint32_t orc_md_subpel_probe(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, int x, int y, int s, int mvx8, int mvy8, int bank, uint32_t *sse);
void orc_md_subpel_grid_picture(const uint8_t *src, int src_stride, int pic_w, int pic_h, int sb_cols, int n_sb, int n_pus, const uint8_t (*pus)[4], int n_refs,
                                const uint8_t *const *refs, const int *ref_stride, const int (*ref_box)[4], const uint32_t *mv, int bank, uint32_t *out);
/* Frame driver used by tests/bench: loops orc_me_fullpel_sb over all SBs.
 * planes are the *padded* luma pictures; (org_x,org_y) is the offset of pixel (0,0) in them. */
typedef struct {
    int32_t sb_x, sb_y;       /* SB origin in pixels */
    int16_t x_origin, y_origin, width, height; /* search window (from orc_me_search_window) */
} OrcSbSearch;
void orc_me_fullpel_frame(const uint8_t *src, const uint8_t *ref, int stride, int org_x, int org_y,
                          const OrcSbSearch *sbs, int n_sb, int sub_sad, uint32_t *best_sad /*[n_sb][85]*/,
                          uint32_t *best_mv /*[n_sb][85]*/, int sb_begin, int sb_end);

/* ---------------------------------------------------------------- transforms (txfm_oracle.c) -- */
/* tx_type: TxType enum order (DCT_DCT=0 .. H_FLIPADST=15), tx_size: TxSize enum order (TX_4X4=0 ..
 * TX_64X16=18), Common/Codec/EbDefinitions.h. */
const int32_t *orc_cospi_arr(int bit);
int  orc_tx_width(int tx_size);
int  orc_tx_height(int tx_size);
void orc_fdct(const int32_t *in, int32_t *out, int n, int cos_bit);
void orc_idct(const int32_t *in, int32_t *out, int n, int cos_bit, int clamp_bit);
void orc_fadst(const int32_t *in, int32_t *out, int n, int cos_bit);
void orc_iadst(const int32_t *in, int32_t *out, int n, int cos_bit, int clamp_bit);
void orc_identity(const int32_t *in, int32_t *out, int n);
void orc_fwd_txfm2d(const int16_t *input, int32_t *output, uint32_t stride, int tx_type, int tx_size, int bd);
uint64_t orc_handle_transform(int32_t *coeff, int tx_size);
uint64_t orc_estimate_transform(const int16_t *residual, uint32_t stride, int32_t *coeff, int tx_type, int tx_size, int bd, int shape);
void orc_inv_txfm2d_add(const int32_t *input, const uint16_t *pred, int32_t stride_r, uint16_t *recon,
                        int32_t stride_w, int tx_type, int tx_size, int bd);
void orc_inv_txfm_add_8bit(const int32_t *input, const uint8_t *pred, int32_t stride_r, uint8_t *recon,
                           int32_t stride_w, int tx_type, int tx_size);
void orc_residual_8bit(const uint8_t *src, uint32_t src_stride, const uint8_t *pred, uint32_t pred_stride,
                       int16_t *res, uint32_t res_stride, uint32_t w, uint32_t h);

/* ---------------------------------------------------------------- quantisation (quant_oracle.c) */
void orc_quantize(int variant, const int32_t *coeff, int n, const int16_t *zbin, const int16_t *round,
                  const int16_t *quant, const int16_t *quant_shift, int32_t *qcoeff, int32_t *dqcoeff,
                  const int16_t *dequant, uint16_t *eob_out, const int16_t *scan, int log_scale);
void orc_coeff_distortion(const int32_t *coeff, const int32_t *recon, int n, uint64_t out[3]);
int32_t orc_cul_level(const int32_t *qcoeff, const int16_t *scan, int eob);

/* ---------------------------------------------------------------- deblocking (dlf_oracle.c) ---- */
void orc_lpf_core(int *px, int len, int blimit, int limit, int thresh, int bd);
void orc_lpf_edge(void *s, int pix_bytes, int pitch, int dir, int len, int blimit, int limit, int thresh, int bd);
void orc_lf_limits(int level, int sharpness, int *lim, int *mblim, int *hev_thr);
void orc_deblock_plane(void *plane, int pix_bytes, int stride, int bd, const uint16_t *edges_v, const uint16_t *edges_h,
                       int units_w, int units_h, int sharpness);
uint64_t orc_plane_sse(int pix_bytes, const void *a, int a_stride, const void *b, int b_stride, int w, int h);
int orc_dlf_search_level(const void *recon, void *tmp, int pix_bytes, int stride, int bd, int w, int h, const void *src, int src_stride,
                         const uint16_t *ev, const uint16_t *eh, int uw, int uh, int sharpness, int plane, int dir, int other_level,
                         int start_level, int loop_filter_mode, int tx_mode_only_4x4, int64_t *best_err_out, int64_t *probes);

/* ---------------------------------------------------------------- CDEF (cdef_oracle.c) --------- */
int  orc_cdef_adjust_strength(int strength, int var);
int  orc_cdef_find_dir(const uint16_t *img, int stride, int32_t *var, int coeff_shift);
void orc_cdef_filter_block(uint8_t *dst8, uint16_t *dst16, int dstride, const uint16_t *in, int istride, int pri_strength,
                           int sec_strength, int dir, int pri_damping, int sec_damping, int bw, int bh, int coeff_shift);
uint64_t orc_cdef_dist_8x8(const uint16_t *a, int astride, const uint16_t *b, int bstride, int coeff_shift);
int  orc_cdef_strength_count(int pick_method);
void orc_cdef_strength(int pick_method, int gi, int *pri, int *sec);
void orc_cdef_search_frame(const void *const rec[3], const int rec_stride[3], const void *const src[3], const int src_stride[3],
                           int pix_bytes, int w, int h, const uint8_t *skip8, int pri_damping, int bd, int pick_method,
                           uint64_t *mse, int fb_begin, int fb_end);
void orc_cdef_apply_frame(const void *const in[3], void *const out[3], const int stride[3], int pix_bytes, int w, int h,
                          const uint8_t *skip8, const uint8_t *y_strength, const uint8_t *uv_strength, int damping_hdr, int bd);

/* ---------------------------------------------------------------- sub-pel convolve (conv_oracle.c) */
extern const int16_t orc_interp_kernels[6][16][8];
void orc_convolve_sr(const void *src, int src_stride, void *dst, int dst_stride, int pix_bytes, int w, int h, int bank_x, int bank_y,
                     int subpel_x_q4, int subpel_y_q4, int bd);
void orc_upsampled_pred(const uint8_t *ref, int ref_stride, uint8_t *pred, int width, int height, int subpel_x_q3, int subpel_y_q3, int bank);
uint32_t orc_variance(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, int w, int h, uint32_t *sse);
uint32_t orc_variance_hbd10(const uint16_t *a, int a_stride, const uint16_t *b, int b_stride, int w, int h, uint32_t *sse);

/* ---------------------------------------------------------------- pyramids (pyramid_oracle.c) --- */
void orc_sad_loop_batch(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, const void *jobs /* SvtHipSadLoop[] */, int begin,
                        int end, uint32_t *best_sad, int16_t *best_xy);
void orc_subpel_predict_batch(int pix_bytes, int bd, const void *ref, int ref_stride, void *dst, int dst_stride, const void *blks /* SvtHipConvBlk[] */,
                              int begin, int end);
void orc_downsample_2d(const uint8_t *in, int in_stride, int w, int h, uint8_t *out, int out_stride, int step, int filtered);
void orc_variance_pyramid_sb(const uint8_t *sb, int stride, int full_precision, uint8_t mean_out[85], uint16_t var_out[85]);

/* ---------------------------------------------------------------- self-guided restoration (sgr_oracle.c) */
extern const int32_t orc_sgr_params[16][4];
int32_t orc_x_by_xplus1(int z);
int32_t orc_one_by_x(int n);
void orc_sgr_filter(const void *dgd, int pix_bytes, int w, int h, int stride, int32_t *flt0, int32_t *flt1, int flt_stride, int ep, int bd);
void orc_sgr_decode_xq(const int32_t *xqd, int32_t *xq, int ep);
void orc_sgr_apply(const void *dat, int pix_bytes, int w, int h, int stride, int ep, const int32_t *xqd, void *dst, int dst_stride, int bd);
void orc_sgr_proj_sums(const void *src, int src_stride, const void *dat, int dat_stride, int pix_bytes, int w, int h, const int32_t *flt0,
                       int f0_stride, const int32_t *flt1, int f1_stride, int ep, int64_t sums[5]);
void orc_sgr_solve(const int64_t sums[5], int size, int ep, int32_t xq[2]);
void orc_sgr_encode_xq(const int32_t *xq, int32_t *xqd, int ep);
int64_t orc_sgr_finer_search(const void *src, int src_stride, const void *dat, int dat_stride, int pix_bytes, int w, int h, const int32_t *flt0,
                             int f0_stride, const int32_t *flt1, int f1_stride, int start_step, int32_t *xqd, int ep);
void orc_sgr_search_units_plane(const void *dgd, int pix_bytes, int stride, const void *src, int src_stride, int pw, int ph, int ss_x, int ss_y,
                                int unit_size, int bd, uint32_t ep_mask, int32_t *xqd_out, int64_t *err_out, uint8_t *best_ep);
int orc_rest_units(int size, int unit_size);
int orc_rest_unit_limits(int pw, int ph, int ss_y, int unit_size, int32_t *limits);
void orc_sgr_search_plane(const void *dgd, int pix_bytes, int stride, const void *src, int src_stride, int pw, int ph, int ss_x, int ss_y,
                          int unit_size, int bd, uint32_t ep_mask, int64_t *sums);
void orc_sgr_apply_plane(const void *dbl, int dbl_stride, void *cdef, int stride, int pix_bytes, int pw, int ph, int ss_x, int ss_y,
                         int unit_size, int bd, const uint8_t *unit_ep, const int32_t *unit_xqd, void *dst, int dst_stride);
void orc_lr_apply_plane(const void *dbl, int dbl_stride, void *cdef, int stride, int pix_bytes, int pw, int ph, int ss_x, int ss_y, int unit_size,
                        int bd, const uint8_t *unit_ep, const int32_t *unit_xqd, const int16_t *unit_wiener, void *dst, int dst_stride);
/* ---------------------------------------------------------------- Wiener restoration (wiener_oracle.c) */
void orc_wiener_compute_stats(int win, const void *dgd, const void *src, int pix_bytes, int bd, int h_start, int h_end, int v_start, int v_end,
                              int dgd_stride, int src_stride, int64_t *M, int64_t *H);
void orc_wiener_convolve_add_src(const void *src, int src_stride, void *dst, int dst_stride, int pix_bytes, const int16_t *filter_x,
                                 const int16_t *filter_y, int w, int h, int bd);
void orc_wiener_convolve_add_src_rounds(const void *src, int src_stride, void *dst, int dst_stride, int pix_bytes, const int16_t *filter_x,
                                        const int16_t *filter_y, int w, int h, int bd, int r0, int r1);
void orc_wiener_stats_plane(int win, const void *dgd, int dgd_stride, const void *src, int src_stride, int pix_bytes, int bd, int pw, int ph, int ss_y,
                            int unit_size, int64_t *M, int64_t *H);
/* search_wiener_seg between the statistics and the refinement (EbRestorationPick.c:1388-1407): 1 = refine vfilter / hfilter, 2 = no Wiener filter for the unit */
int orc_wiener_unit_init(int win, const int64_t *M, const int64_t *H, int16_t vfilter[8], int16_t hfilter[8]);
int64_t orc_sgr_proj_error(const void *src, int src_stride, const void *dat, int dat_stride, int pix_bytes, int w, int h, const int32_t *flt0,
                           int f0_stride, const int32_t *flt1, int f1_stride, const int32_t xq[2], int ep);

/* ---------------------------------------------------------------- temporal filtering (8(f) rank 3) */
/* MeContext's TF fields of one 64x64 block after tf_32x32 / tf_16x16_sub_pel_search (Encoder/Codec/EbMotionEstimationContext.h:447-454) */
typedef struct OrcTfBlk64 {
    int16_t  mv16_x[16], mv16_y[16];
    uint64_t err16[16];
    int16_t  mv32_x[4], mv32_y[4];
    uint64_t err32[4];
    int32_t  split[4];
} OrcTfBlk64;
typedef struct OrcTfRef {       /* one frame of the filtering window; blocks == NULL marks the central picture */
    const void *pred[3];
    int pred_stride[3];
    const OrcTfBlk64 *blocks;   /* raster over (w / 64) x (h / 64) */
} OrcTfRef;
/* Encoder/Codec/EbTemporalFiltering.c:643 / :829 (svt_av1_apply_temporal_filter_planewise(_hbd)_c) */
void orc_tf_planewise(const OrcTfBlk64 *blk, int block_row, int block_col, int tf_chroma, int min_frame_size, int pix_bytes, int bd,
                      const void *y_src, int y_src_stride, const void *y_pre, int y_pre_stride, const void *u_src, const void *v_src,
                      int uv_src_stride, const void *u_pre, const void *v_pre, int uv_pre_stride, unsigned block_width,
                      unsigned block_height, int ss_x, int ss_y, const double *noise_levels, int decay_control, uint32_t *y_accum,
                      uint16_t *y_count, uint32_t *u_accum, uint16_t *u_count, uint32_t *v_accum, uint16_t *v_count);
/* Encoder/Codec/EbTemporalFiltering.c:2136-2412 (pixel side of produce_temporally_filtered_pic) */
void orc_tf_filter_frame(int pix_bytes, int bd, const void *const src[3], const int src_stride[3], void *const dst[3], const int dst_stride[3],
                         int w, int h, int ss_x, int ss_y, int tf_chroma, const OrcTfRef *refs, int n_refs, const double *noise_levels,
                         int decay_control, int min_frame_size, uint64_t sse[2]);
/* Encoder/Codec/EbTemporalFiltering.c:2414 / :2451 (estimate_noise / estimate_noise_highbd); out = {sum, num} */
double orc_tf_estimate_noise(const void *src, int pix_bytes, int bd, int width, int height, int stride, int64_t out[2]);

/* Encoder/Codec/EbTemporalFiltering.c:1469, :1133, :284, :1768 (the TF sub-pel searches, split decision and final prediction); jobs = SvtHipTfSubpelBlk[] */
void orc_tf_subpel_frame(int pix_bytes, int bd, const void *const src[3], const int src_stride[3], const void *const ref[3], const int ref_stride[3],
                         void *const pred[3], const int pred_stride[3], int mi_cols, int mi_rows, uint64_t th16, int tf_hp, int tf_chroma, const void *jobs,
                         int n_jobs, OrcTfBlk64 *blocks);

/* ---------------------------------------------------------------- compound prediction (8(f) rank 4, conv_oracle.c) */
void orc_jnt_convolve_d16(const void *src, int src_stride, int pix_bytes, int w, int h, int bank_x, int bank_y, int subpel_x_q4, int subpel_y_q4, int bd,
                          uint16_t *out, int out_stride);
void orc_compound_predict_batch(int pix_bytes, int bd, const void *ref0, int ref0_stride, const void *ref1, int ref1_stride, void *dst, int dst_stride,
                                uint8_t *masks, const void *blks, int begin, int end);

/* OBMC costs (8(f) rank 4, conv_oracle.c) */
void orc_obmc_block(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, int w, int h, int xoffset, int yoffset, uint32_t out[3]);
void orc_obmc_batch(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, const void *blks, int n, uint32_t *out);

/* warped prediction (8(f) rank 4, warp_oracle.c) */
void orc_warp_affine(const int32_t *mat, const void *ref, int pix_bytes, int bd, int width, int height, int stride, void *pred, int p_col, int p_row, int p_width,
                     int p_height, int p_stride, int ss_x, int ss_y, int alpha, int beta, int gamma, int delta);
void orc_warp_predict_batch(int pix_bytes, int bd, const void *ref, int width, int height, int stride, void *dst, int dst_stride, int ss_x, int ss_y,
                            const void *blks, int n);
/* the is_compound branches on a SvtHipWarpCompBlk list: the arguments of svt_hip_warp_compound_batch_dev, host memory */
void orc_warp_compound_batch(int pix_bytes, int bd, const void *ref, int width, int height, int stride, void *dst, int dst_stride, int ss_x, int ss_y,
                             uint16_t *convbuf, const void *blks, int n);

void orc_blend_a64_batch(int pix_bytes, const void *src0, int src0_stride, const void *src1, int src1_stride, void *dst, int dst_stride, const uint8_t *masks,
                         const void *blks, int n);

/* picture-format conversions around the high-bit-depth path (format_oracle.c) */
void orc_picture_format(int mode, const void *in0, int in0_stride, const void *in1, int in1_stride, void *out0, int out0_stride, void *out1, int out1_stride,
                        int w, int h);

void orc_generate_padding(void *plane, int pix_bytes, int stride, int w, int h, int pad_w, int pad_h);

void orc_sad_loop16_batch(const uint16_t *src, int src_stride, const uint16_t *ref, int ref_stride, const void *jobs, int begin, int end, uint32_t *best_sad,
                          int16_t *best_xy);

#ifdef __cplusplus
}
#endif
int orc_cdef_finish(const uint64_t *mse0, const uint64_t *mse1, int sb_count, const int32_t (*lev0)[8], const int32_t (*lev1)[8], const uint64_t *tot, uint64_t lambda,
                    int32_t *y, int32_t *uv, int32_t *sel, uint64_t *best_cost);
#endif
