/*
 * warp_oracle.c — CPU restatement of AV1 warped (affine) prediction: single reference, and the two passes of a compound prediction
 * (SURVEY 8(f) rank 4).  TEST INFRASTRUCTURE ONLY (see svt_oracle.h).  Pinned by tests/test_oracle_vs_ref.py against svt_av1_warp_affine_c /
 * svt_av1_highbd_warp_affine_c (Common/Codec/EbWarpedMotion.c:577-694, :733-842), non-compound path and is_compound branches.
 */
#include <stdint.h>
#include <stddef.h>
#include "svt_oracle.h"
#include "warp_filter_table.h"

static const int16_t warped_filter[193][8] = SVT_WARPED_FILTER_TABLE;

static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static inline int rp2(int v, int n) { return n == 0 ? v : ((v + ((1 << n) >> 1)) >> n); }
static inline int rd(const void *p, int pb, size_t i) { return pb == 1 ? ((const uint8_t *)p)[i] : ((const uint16_t *)p)[i]; }

/* the compound tail of one block (:660-683, :812-835): cb = ConvolveParams::dst at the block's top-left sample */
typedef struct { uint16_t *cb; int cb_stride, do_average, use_jnt_comp_avg, fwd_offset, bck_offset; } WarpComp;

/* one block (p_col, p_row, p_width, p_height) of a plane under the affine model mat[6] / shear alpha, beta, gamma, delta;
 * round_0 = 3 (5 at 12 bits); non-compound (cmp == NULL): reduce_bits_vert = 2 * FILTER_BITS - reduce_bits_horiz; compound: round_1 = 7 */
static void warp_block(const int32_t *mat, const void *ref, int pix_bytes, int bd, int width, int height, int stride, void *pred, int p_col, int p_row, int p_width,
                       int p_height, int p_stride, int ss_x, int ss_y, int alpha, int beta, int gamma, int delta, const WarpComp *cmp) {
    const int round_0 = bd == 12 ? 5 : 3, round_1 = 7;
    const int extra = bd + 7 - round_0 - 14;
    const int rbh = pix_bytes == 1 ? round_0 : round_0 + (extra > 0 ? extra : 0);      /* :584 / :739-740 */
    const int rbv = cmp ? round_1 : 14 - rbh, obh = bd + 6, obv = bd + 14 - rbh;
    const int round_bits = 14 - round_0 - round_1, offset_bits = bd + 14 - round_0;
    for (int i = p_row; i < p_row + p_height; i += 8)
        for (int j = p_col; j < p_col + p_width; j += 8) {
            int32_t tmp[15 * 8];
            const int32_t src_x = (j + 4) << ss_x, src_y = (i + 4) << ss_y;
            const int32_t dst_x = mat[2] * src_x + mat[3] * src_y + mat[0], dst_y = mat[4] * src_x + mat[5] * src_y + mat[1];
            const int32_t x4 = dst_x >> ss_x, y4 = dst_y >> ss_y;
            const int32_t ix4 = x4 >> 16, iy4 = y4 >> 16;
            int32_t sx4 = x4 & 0xffff, sy4 = y4 & 0xffff;
            sx4 += alpha * (-4) + beta * (-4); sy4 += gamma * (-4) + delta * (-4);
            sx4 &= ~63; sy4 &= ~63;
            for (int k = -7; k < 8; k++) {
                const int iy = clampi(iy4 + k, 0, height - 1);
                int sx = sx4 + beta * (k + 4);
                for (int l = -4; l < 4; l++) {
                    const int ix = ix4 + l - 3;
                    const int16_t *c = warped_filter[rp2(sx, 10) + 64];
                    int32_t sum = 1 << obh;
                    for (int m = 0; m < 8; m++) sum += rd(ref, pix_bytes, (size_t)iy * stride + clampi(ix + m, 0, width - 1)) * c[m];
                    tmp[(k + 7) * 8 + (l + 4)] = rp2(sum, rbh);
                    sx += alpha;
                }
            }
            const int kmax = p_row + p_height - i - 4 < 4 ? p_row + p_height - i - 4 : 4, lmax = p_col + p_width - j - 4 < 4 ? p_col + p_width - j - 4 : 4;
            for (int k = -4; k < kmax; k++) {
                int sy = sy4 + delta * (k + 4);
                for (int l = -4; l < lmax; l++) {
                    const int16_t *c = warped_filter[rp2(sy, 10) + 64];
                    int32_t sum = 1 << obv;
                    for (int m = 0; m < 8; m++) sum += tmp[(k + m + 4) * 8 + (l + 4)] * c[m];
                    sy += gamma;
                    sum = rp2(sum, rbv);
                    if (cmp) {
                        uint16_t *p = cmp->cb + (size_t)(i - p_row + k + 4) * cmp->cb_stride + (j - p_col + l + 4);
                        if (!cmp->do_average) { *p = (uint16_t)sum; continue; }
                        int t = *p;
                        t = cmp->use_jnt_comp_avg ? (t * cmp->fwd_offset + sum * cmp->bck_offset) >> 4 : (t + sum) >> 1;      /* DIST_PRECISION_BITS */
                        t -= (1 << (offset_bits - round_1)) + (1 << (offset_bits - round_1 - 1));
                        sum = rp2(t, round_bits);
                    } else sum -= (1 << (bd - 1)) + (1 << bd);
                    sum = clampi(sum, 0, (1 << bd) - 1);
                    const size_t o = (size_t)(i - p_row + k + 4) * p_stride + (j - p_col + l + 4);
                    if (pix_bytes == 1) ((uint8_t *)pred)[o] = (uint8_t)sum; else ((uint16_t *)pred)[o] = (uint16_t)sum;
                }
            }
        }
}

void orc_warp_affine(const int32_t *mat, const void *ref, int pix_bytes, int bd, int width, int height, int stride, void *pred, int p_col, int p_row, int p_width,
                     int p_height, int p_stride, int ss_x, int ss_y, int alpha, int beta, int gamma, int delta) {
    warp_block(mat, ref, pix_bytes, bd, width, height, stride, pred, p_col, p_row, p_width, p_height, p_stride, ss_x, ss_y, alpha, beta, gamma, delta, NULL);
}

/* the block list of svt_hip_warp_predict_batch_dev (include/svt_hip.h, SvtHipWarpBlk): pred is the destination PLANE, block at (p_col, p_row) */
typedef struct { int32_t mat[6]; int16_t alpha, beta, gamma, delta; int32_t p_col, p_row; uint8_t p_width, p_height, reserved[2]; } OrcWarpBlk;
void orc_warp_predict_batch(int pix_bytes, int bd, const void *ref, int width, int height, int stride, void *dst, int dst_stride, int ss_x, int ss_y,
                            const void *blks_, int n) {
    const OrcWarpBlk *b = (const OrcWarpBlk *)blks_;
    for (int i = 0; i < n; i++)
        orc_warp_affine(b[i].mat, ref, pix_bytes, bd, width, height, stride, (uint8_t *)dst + ((size_t)b[i].p_row * dst_stride + b[i].p_col) * pix_bytes, b[i].p_col,
                        b[i].p_row, b[i].p_width, b[i].p_height, dst_stride, ss_x, ss_y, b[i].alpha, b[i].beta, b[i].gamma, b[i].delta);
}

/* the block list of svt_hip_warp_compound_batch_dev (SvtHipWarpCompBlk), same arguments on host memory: do_average = 0 writes the block's 16-bit
 * prediction to convbuf + cb_off (stride cb_stride) and leaves dst alone (it may be NULL); do_average = 1 combines the prediction with what the
 * buffer holds and writes pixels to the destination PLANE at (p_col, p_row) */
typedef struct { OrcWarpBlk blk; int32_t cb_off, cb_stride; uint8_t do_average, use_jnt_comp_avg, fwd_offset, bck_offset; } OrcWarpCompBlk;
void orc_warp_compound_batch(int pix_bytes, int bd, const void *ref, int width, int height, int stride, void *dst, int dst_stride, int ss_x, int ss_y,
                             uint16_t *convbuf, const void *blks_, int n) {
    const OrcWarpCompBlk *c = (const OrcWarpCompBlk *)blks_;
    for (int i = 0; i < n; i++) {
        const OrcWarpBlk *b = &c[i].blk;
        const WarpComp cmp = { convbuf + c[i].cb_off, c[i].cb_stride, c[i].do_average, c[i].use_jnt_comp_avg, c[i].fwd_offset, c[i].bck_offset };
        void *pred = c[i].do_average ? (uint8_t *)dst + ((size_t)b->p_row * dst_stride + b->p_col) * pix_bytes : NULL;
        warp_block(b->mat, ref, pix_bytes, bd, width, height, stride, pred, b->p_col, b->p_row, b->p_width, b->p_height, dst_stride, ss_x, ss_y, b->alpha,
                   b->beta, b->gamma, b->delta, &cmp);
    }
}
