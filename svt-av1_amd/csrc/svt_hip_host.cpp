// svt_hip_host.cpp — the HOST-side logic of libsvtav1_hip.so that involves no device work: mode-info -> edge descriptors
// (set_lpf_parameters), the ME search-window clamp, the control flow of the deblocking filter-level search.  No HIP header is
// included here on purpose: the same translation unit is compiled into the CPU test double of the library (test
// infrastructure) so that end-to-end encodes on a box without a GPU exercise exactly this code against the reference encoder.
#include <stdint.h>
#include "../../include/svt_hip.h"
#include "svt_hip_host.h"
#include "gm_walk.h"
#include "tpl_synth.h"
#include "palette.h"
#include "ibc_hash.h"
#include "ibc_search.h"
#include "comp_search.h"
#include "obmc_search.h"
#include "ifs_search.h"
#include <vector>

extern "C" {

/* ------------------------------------------------------------------------------------------- ME */
// Host-side restatement of the search-window clamp (EbMotionEstimation.c:1945-2066, unrestricted-MV
// branch; int16 arithmetic with int intermediates, statements in the reference's order).
SvtHipSbSearch svt_hip_me_search_window(int sb_origin_x, int sb_origin_y, int x_center, int y_center, int sa_width,
                                        int sa_height, int pic_width, int pic_height) {
    const int16_t pad = 63;
    const int16_t ox = (int16_t)sb_origin_x, oy = (int16_t)sb_origin_y, pw = (int16_t)pic_width, ph = (int16_t)pic_height;
    int16_t w = (int16_t)sa_width, h = (int16_t)sa_height;
    int16_t xo = (int16_t)(x_center - (w >> 1)), yo = (int16_t)(y_center - (h >> 1));
    xo = (int16_t)((ox + xo < -pad) ? -pad - ox : xo);
    w  = (int16_t)((ox + xo < -pad) ? w - (-pad - (ox + xo)) : w);
    xo = (int16_t)((ox + xo > pw - 1) ? xo - ((ox + xo) - (pw - 1)) : xo);
    if (ox + xo + w > pw) { const int v = w - ((ox + xo + w) - pw); w = (int16_t)(v > 1 ? v : 1); }
    w  = (int16_t)((w < 8) ? w : (w & ~0x07));
    yo = (int16_t)((oy + yo < -pad) ? -pad - oy : yo);
    h  = (int16_t)((oy + yo < -pad) ? h - (-pad - (oy + yo)) : h);
    yo = (int16_t)((oy + yo > ph - 1) ? yo - ((oy + yo) - (ph - 1)) : yo);
    if (oy + yo + h > ph) { const int v = h - ((oy + yo + h) - ph); h = (int16_t)(v > 1 ? v : 1); }
    SvtHipSbSearch s;
    s.sb_x = sb_origin_x; s.sb_y = sb_origin_y; s.x_origin = xo; s.y_origin = yo; s.width = w; s.height = h;
    return s;
}

/* ------------------------------------------------------------------------------- deblocking */
// Restatement of set_lpf_parameters (Encoder/Codec/EbDeblockingFilter.c:168-319) over a plain grid.
// svt_av1_filter_block_plane_vert / _horz (Encoder/Codec/EbDeblockingFilter.c:338-367, :479-508): the 4x4 units of a plane the reference's loops
// visit along one axis.  Every superblock covers sb_size >> ss samples, except that the LAST superblock row / column of a coded size that is
// not a multiple of the superblock size stops at the unpadded source extent (rounded up to 4 samples).  A coded size that IS a multiple of the
// superblock size is filtered completely even when it contains padding (the reference's `mi_row ==` test then never fires).
int svt_hip_dlf_filtered_units(int coded_luma, int pad, int sb_size, int ss) {
    if (coded_luma <= 0 || pad < 0 || pad >= coded_luma || (sb_size != 64 && sb_size != 128) || ss < 0 || ss > 1) return -1;
    const int full = ((coded_luma >> ss) + 3) >> 2;
    if (coded_luma % sb_size == 0) return full;
    const int last = coded_luma / sb_size * sb_size, rem = (coded_luma - pad) % sb_size;
    const int units = ((last >> ss) >> 2) + (((rem >> ss) + 3) >> 2);
    return units < full ? units : full;
}

int svt_hip_dlf_build_edges(const SvtHipDlfModeInfo* mi, int mi_cols, int mi_rows, int plane, int ss_x, int ss_y, int plane_w,
                            int plane_h, uint16_t* edges_v, uint16_t* edges_h) {
    return svt_hip_dlf_build_edges_crop(mi, mi_cols, mi_rows, plane, ss_x, ss_y, plane_w, plane_h, (plane_w + 3) >> 2, (plane_h + 3) >> 2, edges_v, edges_h);
}

int svt_hip_dlf_build_edges_crop(const SvtHipDlfModeInfo* mi, int mi_cols, int mi_rows, int plane, int ss_x, int ss_y, int plane_w,
                                 int plane_h, int filt_units_w, int filt_units_h, uint16_t* edges_v, uint16_t* edges_h) {
    if (!mi || mi_cols <= 0 || mi_rows <= 0 || plane < 0 || plane > 2 || !edges_v || !edges_h || filt_units_w < 0 || filt_units_h < 0) return SVT_HIP_ERR_BAD_ARG;
    const int uw = (plane_w + 3) >> 2, uh = (plane_h + 3) >> 2;
    for (int dir = 0; dir < 2; dir++) {
        uint16_t* out = dir == 0 ? edges_v : edges_h;
        for (int uy = 0; uy < uh; uy++)
            for (int ux = 0; ux < uw; ux++) {
                uint16_t v = 0;
                if (ux >= filt_units_w || uy >= filt_units_h) { out[uy * uw + ux] = 0; continue; }   // outside the loops' range: never visited
                const int x = 4 * ux, y = 4 * uy;
                // chroma maps to the bottom/right mi of the co-located 8x8 (:196-197)
                int mr = ss_y | ((y << ss_y) >> 2), mc = ss_x | ((x << ss_x) >> 2);
                if (mr >= mi_rows) mr = mi_rows - 1;
                if (mc >= mi_cols) mc = mi_cols - 1;
                const SvtHipDlfModeInfo& cur = mi[mr * mi_cols + mc];
                const int ts = plane == 0 ? (dir == 0 ? cur.tx_w_log2 : cur.tx_h_log2) : (dir == 0 ? cur.uv_tx_w_log2 : cur.uv_tx_h_log2);
                const int coord = dir == 0 ? x : y;
                if (!(coord & ((1 << ts) - 1)) && coord) {
                    const int pr = dir == 0 ? mr : mr - (1 << ss_y), pc = dir == 0 ? mc - (1 << ss_x) : mc;
                    if (pr >= 0 && pc >= 0) {
                        const SvtHipDlfModeInfo& prv = mi[pr * mi_cols + pc];
                        const int pts = plane == 0 ? (dir == 0 ? prv.tx_w_log2 : prv.tx_h_log2) : (dir == 0 ? prv.uv_tx_w_log2 : prv.uv_tx_h_log2);
                        const int cl = cur.level[plane][dir], pl = prv.level[plane][dir];
                        int bdim = dir == 0 ? cur.bw_log2 - (plane ? ss_x : 0) : cur.bh_log2 - (plane ? ss_y : 0);
                        if (bdim < 2) bdim = 2;
                        const bool pu_edge = !(coord & ((1 << bdim) - 1));
                        if ((cl || pl) && (!prv.skip_inter || !cur.skip_inter || pu_edge)) {
                            const int mts = ts < pts ? ts : pts;
                            const int len = mts <= 2 ? 4 : (mts == 3 ? (plane ? 6 : 8) : (plane ? 6 : 14));
                            v = (uint16_t)(((cl ? cl : pl) << 8) | len);
                        }
                    }
                }
                out[uy * uw + ux] = v;
            }
    }
    return SVT_HIP_OK;
}


// search_filter_level (Encoder/Codec/EbDeblockingFilter.c:1026-1187): the probe sequence, the integer bias rule and the
// mode <= 2 single refinement, as a PLAN over the errors known so far: the walk is replayed on ss_err[] (-1 = not measured) until it needs a level that has not been
// measured; the one or two levels that iteration needs (filt_low and filt_high are both measured before either is compared when the direction is open) come back in
// need[], the caller measures them (try_filter_frame, :966-1024), stores them in ss_err[] and asks again.  Return value: how many levels are needed; 0 = the walk is
// over, *best_level / *best_err_out are its result.  Measuring the two levels of an iteration together halves the round trips of a device search, and the three planes'
// searches of a picture can be advanced in lockstep (svt_hip_dlf_search_levels_picture_dev).
int svt_hip_dlf_search_plan(const SvtHipDlfSearch* p, const int64_t* ss_err, int need[2], int* best_level, int64_t* best_err_out) {
    if (!p || !ss_err || !need || !best_level) return SVT_HIP_ERR_BAD_ARG;
    const int kMaxLoopFilter = 63;   // MAX_LOOP_FILTER
    int filt_direction = 0;
    int filt_mid = p->start_level < 0 ? 0 : (p->start_level > kMaxLoopFilter ? kMaxLoopFilter : p->start_level);
    int filter_step = filt_mid < 16 ? 4 : filt_mid / 4;
    if (ss_err[filt_mid] < 0) { need[0] = filt_mid; return 1; }
    int64_t best_err = ss_err[filt_mid];
    int filt_best = filt_mid;
    const bool single = p->loop_filter_mode <= 2;
    if (single) filter_step = 2;
    while (filter_step > 0) {
        const int filt_high = filt_mid + filter_step > kMaxLoopFilter ? kMaxLoopFilter : filt_mid + filter_step;
        const int filt_low = filt_mid - filter_step < 0 ? 0 : filt_mid - filter_step;
        int64_t bias = (best_err >> (15 - (filt_mid / 8))) * filter_step;   // bias against raising the level
        if (!p->tx_mode_only_4x4) bias >>= 1;
        const bool want_low = filt_direction <= 0 && filt_low != filt_mid, want_high = filt_direction >= 0 && filt_high != filt_mid;
        int n = 0;
        if (want_low && ss_err[filt_low] < 0) need[n++] = filt_low;
        if (want_high && ss_err[filt_high] < 0 && !(n && need[0] == filt_high)) need[n++] = filt_high;
        if (n) return n;
        if (want_low && ss_err[filt_low] < best_err + bias) {
            if (ss_err[filt_low] < best_err) best_err = ss_err[filt_low];
            filt_best = filt_low;
        }
        if (want_high && ss_err[filt_high] < best_err - bias) {
            if (!single) best_err = ss_err[filt_high];   // the mode <= 2 branch does not update best_err (:1121-1122)
            filt_best = filt_high;
        }
        if (single) break;
        if (filt_best == filt_mid) {
            filter_step /= 2;
            filt_direction = 0;
        } else {
            filt_direction = filt_best < filt_mid ? -1 : 1;
            filt_mid = filt_best;
        }
    }
    *best_level = filt_best;
    if (best_err_out) *best_err_out = ss_err[filt_best];
    return 0;
}
// the levels a probe of `lvl` filters with: plane 0 with dir 2 (svt_av1_pick_filter_level :1281) and chroma use the probed level in both directions
void svt_hip_dlf_search_probe_levels(const SvtHipDlfSearch* p, int lvl, int* lv_v, int* lv_h) {
    *lv_v = lvl; *lv_h = lvl;
    if (p->plane == 0 && p->dir == 0) *lv_h = p->other_level;
    if (p->plane == 0 && p->dir == 1) *lv_v = p->other_level;
}
// the whole walk with a callback per probe (one probe at a time: svt_hip_dlf_search_level_dev, the CPU test double)
int svt_hip_dlf_search_levels_host(const SvtHipDlfSearch* p, SvtHipTryLevelFn try_fn, void* user, int* best_level, int64_t* best_err_out) {
    if (!p || !try_fn || !best_level) return SVT_HIP_ERR_BAD_ARG;
    int64_t ss_err[64];
    for (int i = 0; i < 64; i++) ss_err[i] = -1;
    for (;;) {
        int need[2];
        const int n = svt_hip_dlf_search_plan(p, ss_err, need, best_level, best_err_out);
        if (n <= 0) return n < 0 ? n : SVT_HIP_OK;
        for (int i = 0; i < n; i++) {
            int lv_v, lv_h;
            svt_hip_dlf_search_probe_levels(p, need[i], &lv_v, &lv_h);
            const int64_t e = try_fn(user, lv_v, lv_h);
            if (e < 0) return SVT_HIP_ERR_RUNTIME;
            ss_err[need[i]] = e;
        }
    }
}

/* ------------------------------------------------------------------------------- temporal filter */
double svt_hip_tf_noise_sigma(int64_t sum, int64_t num) {   // EbTemporalFiltering.c:2442-2447
    if (num < 16) return -1.0;
    return (double)sum / (6 * num) * 1.25331413732;
}


/* ------------------------------------------------------------------------------- global motion: the decision */
// svt_aom_count_primitive_refsubexpfin (Encoder/Codec/EbEntropyCoding.c:3385-3401, :3430-3436, :3486-3533) with the reference's 16-bit parameter types
static uint16_t gm_recenter_nonneg(uint16_t r, uint16_t v) {
    if (v > (r << 1)) return v;
    else if (v >= r) return (uint16_t)((v - r) << 1);
    else return (uint16_t)(((r - v) << 1) - 1);
}
static uint16_t gm_recenter_finite_nonneg(uint16_t n, uint16_t r, uint16_t v) {
    if ((r << 1) <= n) return gm_recenter_nonneg(r, v);
    else return gm_recenter_nonneg((uint16_t)(n - 1 - r), (uint16_t)(n - 1 - v));
}
static int32_t gm_count_primitive_quniform(uint16_t n, uint16_t v) {
    if (n <= 1) return 0;
    const int32_t l = (31 - __builtin_clz((unsigned)(n - 1))) + 1;
    const int32_t m = (1 << l) - n;
    return v < m ? l - 1 : l;
}
static int32_t gm_count_primitive_subexpfin(uint16_t n, uint16_t k, uint16_t v) {
    int32_t count = 0, i = 0, mk = 0;
    while (1) {
        const int32_t b = (i ? k + i - 1 : k);
        const int32_t a = (1 << b);
        if (n <= mk + 3 * a) {
            count += gm_count_primitive_quniform((uint16_t)(n - mk), (uint16_t)(v - mk));
            break;
        } else {
            const int32_t t = (v >= mk + a);
            count++;
            if (t) {
                i = i + 1;
                mk += a;
            } else {
                count += b;
                break;
            }
        }
    }
    return count;
}
// aom_count_signed_primitive_refsubexpfin (Encoder/Codec/EbGlobalMotionEstimationCost.c:17-22): the int arguments narrow to int16_t at the call
static int gm_count_signed_refsubexpfin(uint16_t n, uint16_t k, int16_t ref, int16_t v) {
    ref = (int16_t)(ref + n - 1);
    v = (int16_t)(v + n - 1);
    const uint16_t scaled_n = (uint16_t)((n << 1) - 1);
    return gm_count_primitive_subexpfin(scaled_n, k, gm_recenter_finite_nonneg(scaled_n, (uint16_t)ref, (uint16_t)v));
}

// gm_get_params_cost (EbGlobalMotionEstimationCost.c:25-75) against default_warp_params, the only ref_gm compute_global_motion passes
int svt_hip_gm_params_cost_host(const int32_t wmmat[8], int wmtype, int allow_hp) {
    if (!wmmat || wmtype < 0 || wmtype > 3) return -1;
    const int32_t ref[8] = {0, 0, 1 << 16, 0, 0, 1 << 16, 0, 0};
    const int kAlphaMax = 1 << 12, kK = 3, kAlphaBits = 15;
    int params_cost = 0;
    if (wmtype >= 2) {
        params_cost += gm_count_signed_refsubexpfin((uint16_t)(kAlphaMax + 1), kK, (int16_t)((ref[2] >> 1) - (1 << kAlphaBits)), (int16_t)((wmmat[2] >> 1) - (1 << kAlphaBits)));
        params_cost += gm_count_signed_refsubexpfin((uint16_t)(kAlphaMax + 1), kK, (int16_t)(ref[3] >> 1), (int16_t)(wmmat[3] >> 1));
        if (wmtype >= 3) {
            params_cost += gm_count_signed_refsubexpfin((uint16_t)(kAlphaMax + 1), kK, (int16_t)(ref[4] >> 1), (int16_t)(wmmat[4] >> 1));
            params_cost += gm_count_signed_refsubexpfin((uint16_t)(kAlphaMax + 1), kK, (int16_t)((ref[5] >> 1) - (1 << kAlphaBits)), (int16_t)((wmmat[5] >> 1) - (1 << kAlphaBits)));
        }
    }
    if (wmtype >= 1) {
        const int trans_bits = (wmtype == 1) ? 9 - !allow_hp : 12;        // GM_ABS_TRANS_ONLY_BITS - !allow_hp : GM_ABS_TRANS_BITS
        const int trans_prec_diff = (wmtype == 1) ? 13 + !allow_hp : 10;  // GM_TRANS_ONLY_PREC_DIFF + !allow_hp : GM_TRANS_PREC_DIFF
        params_cost += gm_count_signed_refsubexpfin((uint16_t)((1 << trans_bits) + 1), kK, (int16_t)(ref[0] >> trans_prec_diff), (int16_t)(wmmat[0] >> trans_prec_diff));
        params_cost += gm_count_signed_refsubexpfin((uint16_t)((1 << trans_bits) + 1), kK, (int16_t)(ref[1] >> trans_prec_diff), (int16_t)(wmmat[1] >> trans_prec_diff));
    }
    return params_cost << 9;   // AV1_PROB_COST_SHIFT
}

// The model loop of compute_global_motion (Encoder/Codec/EbGlobalMotionEstimation.c:303-399), statement by statement, on records instead of calls: an iteration
// left by `continue` does not reset global_motion, so a ROTZOOM model on a pair whose frame error is 0 survives into (and out of) the AFFINE iteration untested.
int svt_hip_gm_decide_host(const SvtHipGmModelRecord models[2], int64_t ref_frame_error, int rotzoom_model_only, int allow_high_precision_mv, int32_t wmmat_out[8],
                           int32_t* wmtype_out) {
    if (!models || !wmmat_out || !wmtype_out) return SVT_HIP_ERR_BAD_ARG;
    const int32_t kDefault[8] = {0, 0, 1 << 16, 0, 0, 1 << 16, 0, 0};   // default_warp_params
    int32_t gm[8], gm_type = 0;
    for (int k = 0; k < 8; k++) gm[k] = kDefault[k];
    for (int model = 2; model <= (rotzoom_model_only ? 2 : 3); ++model) {
        const SvtHipGmModelRecord* rec = models + (model - 2);
        int64_t best_warp_error = INT64_MAX;
        if (rec->num_inliers_kept != 0 && rec->fit_wmtype != 0) {
            const int64_t warp_error = rec->best_error;
            if (warp_error < best_warp_error) {
                best_warp_error = warp_error;
                for (int k = 0; k < 8; k++) gm[k] = rec->wmmat[k];
                gm_type = rec->wmtype;
            }
        }
        if (gm_type <= 3) {
            SvtHipGmModel shear;
            gm_shear_params(gm, &shear);
            if (!shear.valid) {
                for (int k = 0; k < 8; k++) gm[k] = kDefault[k];
                gm_type = 0;
            }
        }
        if (gm_type == 1) {   // convert_to_trans_prec(allow_hp, .) * GM_TRANS_ONLY_DECODE_FACTOR
            for (int k = 0; k < 2; k++)
                gm[k] = (allow_high_precision_mv ? gm_round_signed(gm[k], 13) : gm_round_signed(gm[k], 14) * 2) * (1 << 13);
        }
        if (gm_type == 0) continue;
        if (ref_frame_error == 0) continue;
        const double adv = (double)best_warp_error / ref_frame_error;
        const int cost = svt_hip_gm_params_cost_host(gm, gm_type, allow_high_precision_mv);
        if (!(adv < 0.65 && adv * cost < 20000)) {   // svt_av1_is_enough_erroradvantage, GM_ERRORADV_TR_0
            for (int k = 0; k < 8; k++) gm[k] = kDefault[k];
            gm_type = 0;
        }
        if (gm_type != 0) break;
    }
    for (int k = 0; k < 8; k++) wmmat_out[k] = gm[k];
    *wmtype_out = gm_type;
    return SVT_HIP_OK;
}

/* ------------------------------------------------------------------------------------------- TPL synthesizer, r0 / beta */
/* svt_hip_tpl_window_dev's contract on host pointers: tpl_synth.h run serially in the reference's order */
int svt_hip_tpl_window_host(const SvtHipTplSynthParams* p, const SvtHipTplWindowFrame* frames, int n_frames, void* out) {
    if (!tplsyn::params_ok(p) || p->rate != 0 || tplsyn::frames_check(frames, n_frames) || !out || ((uintptr_t)out & 7)) return SVT_HIP_ERR_BAD_ARG;
    tplsyn::window_host(*p, frames, n_frames, out);
    return SVT_HIP_OK;
}

/* ------------------------------------------------------------------------------------------- palette luma search */
/* svt_hip_palette_search_batch_dev's contract on host pointers: palette.h run serially, job by job, sample by sample */
int svt_hip_palette_search_host(int pix_bytes, int bd, const void* plane, int stride, const SvtHipPaletteJob* jobs, int njobs, SvtHipPaletteResult* results,
                                SvtHipPaletteCand* cands, uint8_t* maps) {
    if (!pal::search_args_ok(pix_bytes, bd, plane, stride, jobs, njobs, results, cands, maps)) return SVT_HIP_ERR_BAD_ARG;
    pal::search_host(pix_bytes, bd, plane, stride, jobs, njobs, results, cands, maps);
    return SVT_HIP_OK;
}

/* ------------------------------------------------------------------------------------------- intra block copy: hash table, hash search */
/* the contracts of svt_hip_ibc_hash_table_dev / svt_hip_ibc_hash_search_batch_dev on host pointers: ibc_hash.h run serially */
int svt_hip_ibc_hash_table_host(int pix_bytes, int bd, const void* luma, int stride, int width, int height, int32_t* bucket_start, SvtHipIbcHashEntry* entries,
                                int64_t capacity, int32_t* info, void* scratch, size_t scratch_bytes) {
    if (!ibc::table_args_ok(pix_bytes, bd, luma, stride, width, height, bucket_start, entries, capacity, info, scratch, scratch_bytes)) return SVT_HIP_ERR_BAD_ARG;
    ibc::table_host(pix_bytes, luma, stride, width, height, bucket_start, entries, capacity, info, scratch);
    return SVT_HIP_OK;
}

int svt_hip_ibc_hash_search_host(int pix_bytes, int bd, const void* luma, int stride, int width, int height, const int32_t* bucket_start, const SvtHipIbcHashEntry* entries,
                                 const int32_t* mv_joint_cost, const int32_t* mv_comp_cost, const SvtHipIbcSearchJob* jobs, int njobs, SvtHipIbcSearchResult* results) {
    if (!ibc::search_args_ok(pix_bytes, bd, luma, stride, width, height, bucket_start, entries, mv_joint_cost, mv_comp_cost, jobs, njobs, results)) return SVT_HIP_ERR_BAD_ARG;
    ibc::search_host(pix_bytes, bd, luma, stride, width, height, bucket_start, entries, mv_joint_cost, mv_comp_cost, jobs, njobs, results);
    return SVT_HIP_OK;
}

/* the contract of svt_hip_ibc_full_search_batch_dev on host pointers: ibc_search.h run serially */
int svt_hip_ibc_full_search_host(int pix_bytes, int bd, const void* luma, int stride, int width, int height, const int32_t* bucket_start, const SvtHipIbcHashEntry* entries,
                                 const int32_t* mv_joint_cost, const int32_t* mv_comp_cost, const int32_t* mesh_patterns, const SvtHipIbcFullSearchJob* jobs, int njobs,
                                 SvtHipIbcFullSearchResult* results) {
    if (!ibcs::full_search_args_ok(pix_bytes, bd, luma, stride, width, height, bucket_start, entries, mv_joint_cost, mv_comp_cost, mesh_patterns, jobs, njobs, results))
        return SVT_HIP_ERR_BAD_ARG;
    ibcs::full_search_host(pix_bytes, bd, luma, stride, width, height, bucket_start, entries, mv_joint_cost, mv_comp_cost, mesh_patterns, jobs, njobs, results);
    return SVT_HIP_OK;
}

/* ------------------------------------------------------------------------------------------- masked compound and inter-intra: choosing the mask */
int svt_hip_wedge_masks_host(uint8_t* dst) {
    if (!dst) return SVT_HIP_ERR_BAD_ARG;
    cs::wedge_table_build(dst);
    return SVT_HIP_OK;
}

/* the contract of svt_hip_compound_search_batch_dev on host pointers: comp_search.h run serially */
int svt_hip_compound_search_host(const double* rate, const double* dist, const int32_t* bsize_cat, int pix_bytes, int bd, const void* src, int src_stride, int width,
                                 int height, const void* pred, int64_t pred_samples, const int32_t* rates, int nrates, const SvtHipCompSearchJob* jobs, int njobs,
                                 SvtHipCompSearchResult* results, SvtHipCompSearchCand* cand) {
    if (!cs::rd_tables_ok(rate, dist, bsize_cat) || !cs::search_args_ok(pix_bytes, bd, src, src_stride, width, height, pred, pred_samples, rates, nrates, jobs, njobs, results))
        return SVT_HIP_ERR_BAD_ARG;
    if (!njobs) return SVT_HIP_OK;
    std::vector<uint8_t> masks(cs::WEDGE_TABLE_BYTES);
    cs::wedge_table_build(masks.data());
    cs::search_host(pix_bytes, bd, src, src_stride, pred, rates, masks.data(), cs::RdTables{rate, dist, bsize_cat}, jobs, njobs, results, cand);
    return SVT_HIP_OK;
}

/* ------------------------------------------------------------------------------------------- OBMC in mode decision: obmc_search.h run serially */
int svt_hip_obmc_neighbours_host(const uint8_t* above_sb_type, const uint8_t* above_overlappable, const uint8_t* left_sb_type, const uint8_t* left_overlappable, int mi_rows,
                                 int mi_cols, int mi_row, int mi_col, int bsize, SvtHipObmcTargetJob* job) {
    return obmc::neighbours_host(above_sb_type, above_overlappable, left_sb_type, left_overlappable, mi_rows, mi_cols, mi_row, mi_col, bsize, job) ? SVT_HIP_OK
                                                                                                                                                   : SVT_HIP_ERR_BAD_ARG;
}

/* the contract of svt_hip_obmc_target_batch_dev on host pointers */
int svt_hip_obmc_target_host(const uint8_t* src, int src_stride, int width, int height, const uint8_t* nbr, int64_t nbr_samples, const SvtHipObmcTargetJob* jobs, int njobs,
                             int32_t* wsrc, int32_t* mask, int64_t wm_samples) {
    if (!obmc::target_args_ok(src, src_stride, width, height, nbr, nbr_samples, jobs, njobs, wsrc, mask, wm_samples)) return SVT_HIP_ERR_BAD_ARG;
    obmc::target_host(src, src_stride, nbr, jobs, njobs, wsrc, mask);
    return SVT_HIP_OK;
}

/* the contract of svt_hip_obmc_search_batch_dev on host pointers */
int svt_hip_obmc_search_host(const uint8_t* ref, int ref_stride, int width, int height, int pad_w, int pad_h, int mi_rows, int mi_cols, const int32_t* wsrc,
                             const int32_t* mask, int64_t wm_samples, const int32_t* mv_joint_cost, const int32_t* mv_comp_cost, const SvtHipObmcSearchJob* jobs, int njobs,
                             SvtHipObmcSearchResult* results) {
    const obmc::Plane P{ref, ref_stride, width, height, pad_w, pad_h, mi_rows, mi_cols};
    if (!obmc::search_args_ok(P, wsrc, mask, wm_samples, mv_joint_cost, mv_comp_cost, jobs, njobs, results)) return SVT_HIP_ERR_BAD_ARG;
    obmc::search_host(P, wsrc, mask, wm_samples, mv_joint_cost, mv_comp_cost, jobs, njobs, results);
    return SVT_HIP_OK;
}

/* ------------------------------------------------------------------------------------------- the dual interpolation filter search: ifs_search.h run serially */
/* the contract of svt_hip_ifs_search_batch_dev on host pointers */
int svt_hip_ifs_search_host(int pix_bytes, int bd, const void* src, int src_stride, int width, int height, const void* ref0, int ref0_stride, const void* ref1, int ref1_stride,
                            void* dst, int dst_stride, const SvtHipIfsJob* jobs, int njobs, SvtHipIfsResult* results, SvtHipIfsCand* cand) {
    if (!ifs::search_args_ok(pix_bytes, bd, src, src_stride, width, height, ref0, ref0_stride, ref1, ref1_stride, dst, dst_stride, jobs, njobs, results)) return SVT_HIP_ERR_BAD_ARG;
    ifs::search_host(pix_bytes, bd, src, src_stride, ref0, ref0_stride, ref1, ref1_stride, dst, dst_stride, jobs, njobs, results, cand);
    return SVT_HIP_OK;
}

}  // extern "C"
