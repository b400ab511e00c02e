// obmc_search.h — the arithmetic of OBMC in mode decision that is the same on the host and on the device, written once: the weighted target of a block
// (svt_hip_obmc_target_batch_dev) and the motion refinement against it (svt_hip_obmc_search_batch_dev).  obmc_search.hip evaluates the probes of a step across a
// workgroup and runs the walks in every lane with the same values; svt_hip_obmc_target_host / svt_hip_obmc_search_host (svt_hip_host.cpp) and
// tests/obmc_search_host_test.cpp run them serially.  Plain C++17, no HIP.  mv_err_cost and mvsad_err_cost are ibc_hash.h's and ibc_search.h's and the block-size
// tables comp_search.h's: not restated.
// File:line under Source/Lib of the reference:
//   Common/Codec/EbInterPrediction.c:2233-2260        obmc_mask_N, svt_av1_get_obmc_mask: the specification's Obmc_Mask_N (7.11.3.10, overlapped motion compensation)
//   Encoder/Codec/EbEncInterPrediction.c:918-996      foreach_overlappable_nb_above / _left, max_neighbor_obmc (:912)
//   Encoder/Codec/EbEncInterPrediction.c:2196-2256    calc_target_weighted_pred_above / _left
//   Encoder/Codec/EbEncInterPrediction.c:2376-2437    calc_target_weighted_pred
//   Encoder/Codec/EbModeDecision.c:2951-3036          single_motion_search
//   Encoder/Codec/av1me.c:249-270                     svt_av1_set_mv_search_range
//   Encoder/Codec/av1me.c:776-790, :791-834, :836-855 get_obmc_mvpred_var, obmc_refining_search_sad, svt_av1_obmc_full_pixel_search
//   Encoder/Codec/av1me.c:857-869, :973-1060, :1069-1254   set_subpel_mv_search_range, upsampled_obmc_pref_error, upsampled_setup_obmc_center_error,
//                                                     svt_av1_find_best_obmc_sub_pixel_tree_up with SECOND_LEVEL_CHECKS_BEST(1) (:957-971) and CHECK_BETTER1 (:925-955)
//   Encoder/C_DEFAULT/variance.c:212-269, :270-299    svt_aom_upsampled_pred_c (USE_8_TAPS: EIGHTTAP_REGULAR), svt_aom_obmc_variance{W}x{H}_c
//   Encoder/C_DEFAULT/sad_av1.c:18-38                 svt_aom_obmc_sad{W}x{H}_c
//   Encoder/Codec/EbRateDistortionCost.c:85-99        svt_av1_mv_bit_cost
// Two things are restated in another form, and why that is the reference's result:
//  * the target is computed sample by sample, not pass by pass.  The passes write a sample at most once each (the segments of a side do not overlap: a list that
//    does is refused), the scaling by 64 and the last line touch every sample once, so a sample's value depends on nothing but its own position.
//  * the probes of a step are evaluated before the step's decisions are taken.  A probe's value does not depend on the decisions (the positions of the four
//    refinement sites, of the four axis probes and of the first two second-level probes are fixed when the step begins); the decisions then run in the
//    reference's order on those values, with its unsigned / int mix.  A probe the reference would not evaluate (outside the range) is not evaluated here either.
// docs/kernels/obmc.md.
#pragma once
#include "comp_search.h"
#include "ibc_search.h"

namespace obmc {

using TargetJob = SvtHipObmcTargetJob;
using Job = SvtHipObmcSearchJob;
using Result = SvtHipObmcSearchResult;

constexpr int BLOCK_SIZES = cs::BLOCK_SIZES, MAX_SEGS = 4, MAX_JOBS = 1 << 24;
constexpr int MI_SIZE = 4, INTERP_EXTEND = 4;                       // AOM_INTERP_EXTEND
constexpr int MAX_FULL_PEL_VAL = 1023, MV_LOW = -(1 << 14), MV_UPP = 1 << 14;
constexpr int REFINE_RANGE = 8, MV_COST_WEIGHT = 108;
constexpr int FILTER_REACH_LO = 3, FILTER_REACH_HI = 4;             // an 8-tap filter reads -3 .. +4 around a sample
constexpr int MAX_DIM = 1 << 16, MAX_MI = 1 << 14;
constexpr int STATUS_SEARCHED = 0, STATUS_EMPTY_LIMITS = 1;

// Obmc_Mask_1, _2, _4, _8, _16, _32, _64 back to back: the table of length N starts at N - 1
constexpr uint8_t kObmcMask[127] = {64,                                                                                                              // 1
                                    45, 64,                                                                                                          // 2
                                    39, 50, 59, 64,                                                                                                  // 4
                                    36, 42, 48, 53, 57, 61, 64, 64,                                                                                  // 8
                                    34, 37, 40, 43, 46, 49, 52, 54, 56, 58, 60, 61, 64, 64, 64, 64,                                                  // 16
                                    33, 35, 36, 38, 40, 41, 43, 44, 45, 47, 48, 50, 51, 52, 53, 55, 56, 57, 58, 59, 60, 60, 61, 62, 64, 64, 64, 64, 64, 64, 64, 64,   // 32
                                    33, 34, 35, 35, 36, 37, 38, 39, 40, 40, 41, 42, 43, 44, 44, 44, 45, 46, 47, 47, 48, 49, 50, 51, 51, 51, 52, 52, 53, 54, 55, 56,
                                    56, 56, 57, 57, 58, 58, 59, 60, 60, 60, 60, 60, 61, 62, 62, 62, 62, 62, 63, 63, 63, 63, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64};  // 64
// EIGHTTAP_REGULAR at the eight 1/8 positions (av1_get_interp_filter_subpel_kernel(filter, q3 << 1)): the even rows of the specification's Subpel_Filters[0]
constexpr int16_t kTaps[8][8] = {{0, 0, 0, 128, 0, 0, 0, 0},   // position 0 is never filtered: svt_aom_upsampled_pred copies
                                {0, 2, -10, 122, 18, -4, 0, 0}, {0, 2, -14, 110, 38, -10, 2, 0}, {0, 2, -16, 94, 58, -12, 2, 0}, {0, 2, -14, 76, 76, -14, 2, 0},
                                {0, 2, -12, 58, 94, -16, 2, 0}, {0, 2, -10, 38, 110, -14, 2, 0}, {0, 0, -4, 18, 122, -10, 2, 0}};

using cs::block_w;   // the 22 block sizes: comp_search.h's tables
using cs::block_h;
using ibcs::imin;
using ibcs::imax;
IBC_HD bool bsize_ok(int b) { return cs::bsize_ok(b) && block_w(b) >= 8 && block_h(b) >= 8; }   // is_motion_variation_allowed_bsize: 17 sizes
IBC_HD int  obmc_mask(int length, int pos) { return kObmcMask[length - 1 + pos]; }
IBC_HD int  overlap_of(int side) { return imin(side, 64) >> 1; }

// ---------------------------------------------------------------------------------------------------------------- the neighbour lists
// foreach_overlappable_nb_above / _left on one side: sb_side[i] = the side (in 4-sample units) of the neighbour at unit i along the block's edge
// (mi_size_wide / mi_size_high of its sb_type), flag[i] = is_neighbor_overlappable.  n4 = the block's side in units, pos = mi_col / mi_row, end = mi_cols / mi_rows.
template <class SIDE> inline int neighbours_side(SIDE sb_side, const uint8_t* flag, int n4, int pos, int end, int32_t* rel, int32_t* len) {
    constexpr int kMaxNeighbors[6] = {0, 1, 2, 3, 4, 4};   // max_neighbor_obmc
    const int     nb_max = kMaxNeighbors[ibcs::ilog2(n4)], last = imin(pos + n4, end);
    int           count = 0, step;
    for (int at = pos; at < last && count < nb_max; at += step) {
        int pick = at - pos;
        step = imin(sb_side(pick), 16);   // mi_size_wide[BLOCK_64X64]
        if (step == 1) {                  // a 4-wide block is half of a pair: back to the even position, the odd one decides
            at &= ~1;
            pick = at - pos + 1;
            step = 2;
        }
        if (flag[pick]) {
            rel[count] = at - pos;
            len[count] = imin(n4, step);
            ++count;
        }
    }
    for (int i = count; i < MAX_SEGS; ++i) rel[i] = len[i] = 0;
    return count;
}
inline bool neighbours_host(const uint8_t* above_sb, const uint8_t* above_flag, const uint8_t* left_sb, const uint8_t* left_flag, int mi_rows, int mi_cols, int mi_row,
                            int mi_col, int bsize, TargetJob* job) {
    if (!job || !bsize_ok(bsize) || mi_rows < 1 || mi_cols < 1 || mi_rows > MAX_MI || mi_cols > MAX_MI || mi_row < 0 || mi_col < 0 || mi_row >= mi_rows ||
        mi_col >= mi_cols || (mi_row & 1) || (mi_col & 1) || !above_sb != !above_flag || !left_sb != !left_flag)
        return false;
    const int n4_w = block_w(bsize) / MI_SIZE, n4_h = block_h(bsize) / MI_SIZE;
    for (int i = 0; above_sb && i < n4_w; ++i)
        if (above_sb[i] >= BLOCK_SIZES) return false;
    for (int i = 0; left_sb && i < n4_h; ++i)
        if (left_sb[i] >= BLOCK_SIZES) return false;
    job->n_above = job->n_left = 0;
    for (int i = 0; i < MAX_SEGS; ++i) job->above_rel[i] = job->above_len[i] = job->left_rel[i] = job->left_len[i] = 0;
    if (above_sb) job->n_above = neighbours_side([&](int i) { return block_w(above_sb[i]) / MI_SIZE; }, above_flag, n4_w, mi_col, mi_cols, job->above_rel, job->above_len);
    if (left_sb) job->n_left = neighbours_side([&](int i) { return block_h(left_sb[i]) / MI_SIZE; }, left_flag, n4_h, mi_row, mi_rows, job->left_rel, job->left_len);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- the weighted target
IBC_HD bool segs_ok(int n, const int32_t* rel, const int32_t* len, int n4) {
    if (n < 0 || n > MAX_SEGS) return false;
    int next = 0;
    for (int i = 0; i < n; ++i) {
        if (rel[i] < next || len[i] < 1 || len[i] > n4 || rel[i] > n4 - len[i]) return false;
        next = rel[i] + len[i];
    }
    return true;
}
IBC_HD bool covered(int n, const int32_t* rel, const int32_t* len, int unit) {
    for (int i = 0; i < n; ++i)
        if (unit >= rel[i] && unit < rel[i] + len[i]) return true;
    return false;
}
IBC_HD bool target_job_ok(const TargetJob& j, int width, int height, int64_t nbr_samples, int64_t wm_samples) {
    if (!bsize_ok(j.bsize)) return false;
    const int bw = block_w(j.bsize), bh = block_h(j.bsize);
    if (j.x < 0 || j.y < 0 || j.x > width - bw || j.y > height - bh) return false;
    if (!segs_ok(j.n_above, j.above_rel, j.above_len, bw / MI_SIZE) || !segs_ok(j.n_left, j.left_rel, j.left_len, bh / MI_SIZE)) return false;
    if (j.wm_off < 0 || (int64_t)j.wm_off + bw * bh > wm_samples) return false;
    // the samples the two passes read: rows 0 .. overlap - 1 of the above segments' columns, columns 0 .. overlap - 1 of the left segments' rows
    if (j.n_above) {
        const int     c0 = j.above_rel[0] * MI_SIZE, c1 = (j.above_rel[j.n_above - 1] + j.above_len[j.n_above - 1]) * MI_SIZE - 1;
        const int64_t lo = (int64_t)j.above_off + c0, hi = (int64_t)j.above_off + (int64_t)(overlap_of(bh) - 1) * j.above_stride + c1;
        if (j.above_stride < 0 || lo < 0 || hi >= nbr_samples) return false;
    }
    if (j.n_left) {
        const int     r0 = j.left_rel[0] * MI_SIZE, r1 = (j.left_rel[j.n_left - 1] + j.left_len[j.n_left - 1]) * MI_SIZE - 1;
        const int64_t lo = (int64_t)j.left_off + (int64_t)r0 * j.left_stride, hi = (int64_t)j.left_off + (int64_t)r1 * j.left_stride + overlap_of(bw) - 1;
        if (j.left_stride < 0 || lo < 0 || hi >= nbr_samples) return false;
    }
    return true;
}
inline bool target_args_ok(const uint8_t* src, int stride, int width, int height, const uint8_t* nbr, int64_t nbr_samples, const TargetJob* jobs, int njobs,
                           const int32_t* wsrc, const int32_t* mask, int64_t wm_samples) {
    if (!src || !jobs || !wsrc || !mask || njobs < 0 || njobs > MAX_JOBS || width < 1 || height < 1 || width > MAX_DIM || height > MAX_DIM || stride < width ||
        nbr_samples < 0 || nbr_samples > INT32_MAX || (nbr_samples && !nbr) || wm_samples < 0 || wm_samples > INT32_MAX)
        return false;
    for (int i = 0; i < njobs; ++i)
        if (!target_job_ok(jobs[i], width, height, nbr_samples, wm_samples)) return false;
    return true;
}
// wsrc and mask of sample (r, c) of the block; src = the source sample
IBC_HD void target_sample(const TargetJob& J, int bw, int bh, int r, int c, int src, const uint8_t* nbr, int32_t* wsrc, int32_t* mask) {
    int32_t   w = 0, m = 64;
    const int ov_a = overlap_of(bh), ov_l = overlap_of(bw);
    if (r < ov_a && covered(J.n_above, J.above_rel, J.above_len, c / MI_SIZE)) {
        const int m0 = obmc_mask(ov_a, r);
        w = (64 - m0) * (int)nbr[(int64_t)J.above_off + (int64_t)r * J.above_stride + c];
        m = m0;
    }
    w *= 64;
    m *= 64;
    if (c < ov_l && covered(J.n_left, J.left_rel, J.left_len, r / MI_SIZE)) {
        const int m0 = obmc_mask(ov_l, c);
        w = (w >> 6) * m0 + ((int)nbr[(int64_t)J.left_off + (int64_t)r * J.left_stride + c] << 6) * (64 - m0);
        m = (m >> 6) * m0;
    }
    *wsrc = src * 4096 - w;
    *mask = m;
}
inline void target_host(const uint8_t* src, int stride, const uint8_t* nbr, const TargetJob* jobs, int njobs, int32_t* wsrc, int32_t* mask) {
    for (int i = 0; i < njobs; ++i) {
        const TargetJob& J = jobs[i];
        const int        bw = block_w(J.bsize), bh = block_h(J.bsize);
        for (int r = 0; r < bh; ++r)
            for (int c = 0; c < bw; ++c)
                target_sample(J, bw, bh, r, c, src[(size_t)(J.y + r) * stride + J.x + c], nbr, wsrc + J.wm_off + r * bw + c, mask + J.wm_off + r * bw + c);
    }
}

// ---------------------------------------------------------------------------------------------------------------- limits
struct Limits {
    int col_min, col_max, row_min, row_max;
};
IBC_HD bool limits_empty(const Limits& L) { return L.col_max < L.col_min || L.row_max < L.row_min; }
IBC_HD bool mv_in(const Limits& L, int row, int col) { return col >= L.col_min && col <= L.col_max && row >= L.row_min && row <= L.row_max; }
// single_motion_search's x->mv_limits
IBC_HD Limits block_limits(const Job& J, int mi_rows, int mi_cols) {
    const int mi_w = block_w(J.bsize) / MI_SIZE, mi_h = block_h(J.bsize) / MI_SIZE;
    return Limits{-((J.mi_col + mi_w) * MI_SIZE + INTERP_EXTEND), (mi_cols - J.mi_col) * MI_SIZE + INTERP_EXTEND, -((J.mi_row + mi_h) * MI_SIZE + INTERP_EXTEND),
                  (mi_rows - J.mi_row) * MI_SIZE + INTERP_EXTEND};
}
// svt_av1_set_mv_search_range
IBC_HD Limits search_range(Limits L, int ref_row, int ref_col) {
    const int col_min = imax((ref_col >> 3) - MAX_FULL_PEL_VAL + ((ref_col & 7) != 0), (MV_LOW >> 3) + 1), col_max = imin((ref_col >> 3) + MAX_FULL_PEL_VAL, (MV_UPP >> 3) - 1);
    const int row_min = imax((ref_row >> 3) - MAX_FULL_PEL_VAL + ((ref_row & 7) != 0), (MV_LOW >> 3) + 1), row_max = imin((ref_row >> 3) + MAX_FULL_PEL_VAL, (MV_UPP >> 3) - 1);
    L.col_min = imax(L.col_min, col_min);
    L.col_max = imin(L.col_max, col_max);
    L.row_min = imax(L.row_min, row_min);
    L.row_max = imin(L.row_max, row_max);
    return L;
}
// set_subpel_mv_search_range, in 1/8 sample
IBC_HD Limits subpel_range(const Limits& L, int ref_row, int ref_col) {
    const int max_mv = MAX_FULL_PEL_VAL * 8;
    return Limits{imax(MV_LOW + 1, imax(L.col_min * 8, ref_col - max_mv)), imin(MV_UPP - 1, imin(L.col_max * 8, ref_col + max_mv)),
                  imax(MV_LOW + 1, imax(L.row_min * 8, ref_row - max_mv)), imin(MV_UPP - 1, imin(L.row_max * 8, ref_row + max_mv))};
}
// the reference plane as the search sees it: sample (0, 0) of the picture, the border around it
struct Plane {
    const uint8_t* ref;
    int            stride, width, height, pad_w, pad_h, mi_rows, mi_cols;
};
// 0: to be searched; 1: empty limits; -1: refused.  The window is derived from the limits, not from the walk: the block displaced by the limits, one more whole
// sample (MV_LOW + 1 is one sample below the narrowed minimum; a sub-pel probe stays inside the whole-sample limits), and the filter's reach.
IBC_HD int job_status(const Job& J, const Plane& P, int64_t wm_samples) {
    if (!bsize_ok(J.bsize) || J.mi_row < 0 || J.mi_col < 0 || J.mi_row >= P.mi_rows || J.mi_col >= P.mi_cols) return -1;
    const int bw = block_w(J.bsize), bh = block_h(J.bsize);
    if (J.wm_off < 0 || (int64_t)J.wm_off + bw * bh > wm_samples) return -1;
    if (J.mv_row < INT16_MIN || J.mv_row > INT16_MAX || J.mv_col < INT16_MIN || J.mv_col > INT16_MAX || J.ref_mv_row < INT16_MIN || J.ref_mv_row > INT16_MAX ||
        J.ref_mv_col < INT16_MIN || J.ref_mv_col > INT16_MAX)
        return -1;
    if (J.sad_per_bit < 0 || J.error_per_bit < 0 || J.allow_hp < 0 || J.allow_hp > 1) return -1;
    const Limits L = search_range(block_limits(J, P.mi_rows, P.mi_cols), J.ref_mv_row, J.ref_mv_col);
    if (limits_empty(L)) return STATUS_EMPTY_LIMITS;
    const int x0 = J.mi_col * MI_SIZE, y0 = J.mi_row * MI_SIZE;
    if (x0 + L.col_min - 1 - FILTER_REACH_LO < -P.pad_w || x0 + L.col_max + 1 + bw - 1 + FILTER_REACH_HI > P.width + P.pad_w - 1 ||
        y0 + L.row_min - 1 - FILTER_REACH_LO < -P.pad_h || y0 + L.row_max + 1 + bh - 1 + FILTER_REACH_HI > P.height + P.pad_h - 1)
        return -1;
    return STATUS_SEARCHED;
}
inline bool search_args_ok(const Plane& P, const int32_t* wsrc, const int32_t* mask, int64_t wm_samples, const int32_t* joint_cost, const int32_t* comp_cost,
                           const Job* jobs, int njobs, const Result* results) {
    if (!P.ref || !wsrc || !mask || !joint_cost || !comp_cost || !jobs || !results || njobs < 0 || njobs > MAX_JOBS || P.width < 1 || P.height < 1 || P.width > MAX_DIM ||
        P.height > MAX_DIM || P.pad_w < 0 || P.pad_h < 0 || P.pad_w > MAX_DIM || P.pad_h > MAX_DIM || P.stride < P.width + 2 * P.pad_w || P.mi_rows < 1 || P.mi_cols < 1 ||
        P.mi_rows > MAX_MI || P.mi_cols > MAX_MI || wm_samples < 0 || wm_samples > INT32_MAX)
        return false;
    for (int i = 0; i < njobs; ++i)
        if (job_status(jobs[i], P, wm_samples) < 0) return false;
    return true;
}
IBC_HD Result empty_result(int status) { return Result{status, 0, 0, INT32_MAX, 0, INT32_MAX, 0, 0, (uint32_t)INT32_MAX, 0, 0, 0}; }

// ---------------------------------------------------------------------------------------------------------------- a probe's arithmetic
IBC_HD int round_shift(int v, int n) { return (v + (1 << (n - 1))) >> n; }
IBC_HD int round_shift_signed(int v, int n) { return v < 0 ? -round_shift(-v, n) : round_shift(v, n); }   // ROUND_POWER_OF_TWO_SIGNED
IBC_HD int clip_pixel(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// one output of convolve_horiz / convolve_vert: eight samples `step` apart, the first three before the output's position
template <class T> IBC_HD int filter8(const T* p, ptrdiff_t step, int q3) {
    int sum = 0;
    for (int k = 0; k < 8; ++k) sum += kTaps[q3][k] * (int)p[(k - FILTER_REACH_LO) * step];
    return clip_pixel(round_shift(sum, 7));
}
IBC_HD uint32_t sad_term(int wsrc, int mask, int pre) { return (uint32_t)round_shift(ibcs::iabs(wsrc - pre * mask), 12); }   // svt_aom_obmc_sad
IBC_HD int      var_diff(int wsrc, int mask, int pre) { return round_shift_signed(wsrc - pre * mask, 12); }                 // obmc_variance
IBC_HD uint32_t variance_of(uint32_t sse, int sum, int count) { return sse - (uint32_t)(((int64_t)sum * sum) / count); }
// svt_av1_mv_bit_cost with MV_COST_WEIGHT; the clamp to MV_LOW .. MV_UPP cannot act on a difference the limits allow
IBC_HD int mv_bit_cost(int row, int col, int ref_row, int ref_col, const int32_t* jc, const int32_t* cc) {
    const int d_row = ibcs::clampi(row - ref_row, -ibc::MV_MAX, ibc::MV_MAX), d_col = ibcs::clampi(col - ref_col, -ibc::MV_MAX, ibc::MV_MAX);
    const int joint = d_row == 0 ? (d_col == 0 ? 0 : 1) : (d_col == 0 ? 2 : 3);
    return round_shift((jc[joint] + cc[ibc::MV_MAX + d_row] + cc[SVT_HIP_IBC_MV_VALS + ibc::MV_MAX + d_col]) * MV_COST_WEIGHT, 7);
}
// the job as ibcs::mvsad_err_cost and ibcs::mvpred_cost read it: ref_mv and the two multipliers
IBC_HD ibcs::Job cost_job(const Job& J) {
    ibcs::Job c{};
    c.ref_mv_row = J.ref_mv_row;
    c.ref_mv_col = J.ref_mv_col;
    c.sad_per_bit = J.sad_per_bit;
    c.error_per_bit = J.error_per_bit;
    return c;
}

// ---------------------------------------------------------------------------------------------------------------- the two walks
// An evaluator EV gives the walks their sums, up to four probes at a time; bit i of `live` says that probe i is to be evaluated.
//   void sads(rows, cols, n, live, out)              svt_aom_obmc_sad of the block displaced by whole samples (row, col)
//   void probes(rows, cols, n, live, var, sse)       upsampled_obmc_pref_error at (row, col) in 1/8 sample: the variance and its sse
// svt_av1_obmc_full_pixel_search: the start in whole samples in, the refined vector out
template <class EV> IBC_HD void full_pixel_search(const EV& ev, const Job& J, const Limits& L, const int32_t* jc, const int32_t* cc, Result* R) {
    const ibcs::Job cj = cost_job(J);
    int             row = ibcs::clampi(J.mv_row >> 3, L.row_min, L.row_max), col = ibcs::clampi(J.mv_col >> 3, L.col_min, L.col_max);   // clamp_mv
    uint32_t        sad[4];
    ev.sads(&row, &col, 1, 1u, sad);
    uint32_t best = sad[0] + ibcs::mvsad_err_cost(cj, row, col, jc, cc);
    int      steps = 0;
    for (int i = 0; i < REFINE_RANGE; ++i) {
        int      rows[4], cols[4], best_site = -1;
        unsigned live = 0;
        for (int j = 0; j < 4; ++j) {
            rows[j] = row + ibcs::unpack(ibcs::NEIGH_ROWS, j);
            cols[j] = col + ibcs::unpack(ibcs::NEIGH_COLS, j);
            if (mv_in(L, rows[j], cols[j])) live |= 1u << j;
        }
        ev.sads(rows, cols, 4, live, sad);
        for (int j = 0; j < 4; ++j) {
            if (!(live >> j & 1)) continue;
            uint32_t s = sad[j];
            if (s < best) {
                s += ibcs::mvsad_err_cost(cj, rows[j], cols[j], jc, cc);
                if (s < best) {
                    best = s;
                    best_site = j;
                }
            }
        }
        if (best_site == -1) break;
        row = rows[best_site];
        col = cols[best_site];
        ++steps;
    }
    R->full_row = row;
    R->full_col = col;
    R->refining = (int32_t)best;
    R->steps = steps;
    R->bestsme = (int32_t)best;
    if ((int32_t)best < INT32_MAX) {   // get_obmc_mvpred_var
        int      r8 = row * 8, c8 = col * 8;
        uint32_t var[4], sse[4];
        ev.probes(&r8, &c8, 1, 1u, var, sse);
        R->bestsme = ibc::pred_cost(var[0], ibcs::mvpred_cost(cj, row, col, jc, cc));
    }
}
// svt_av1_find_best_obmc_sub_pixel_tree_up from the whole-sample vector (R->full_row, R->full_col); S = subpel_range of the limits before the narrowing
template <class EV> IBC_HD void sub_pixel_tree(const EV& ev, const Job& J, const Limits& S, const int32_t* jc, const int32_t* cc, Result* R) {
    const int      minc = S.col_min, maxc = S.col_max, minr = S.row_min, maxr = S.row_max;
    const auto     in = [&](int r, int c) { return c >= minc && c <= maxc && r >= minr && r <= maxr; };
    const auto     cost = [&](int r, int c) { return ibc::mv_err_cost(r - J.ref_mv_row, c - J.ref_mv_col, jc, cc, J.error_per_bit); };
    const uint32_t kIntMax = (uint32_t)INT32_MAX;
    int            br = R->full_row * 8, bc = R->full_col * 8, hstep = 4, best_idx = -1, tr = br, tc = bc;
    const int      round = J.allow_hp ? 3 : 2;
    uint32_t       var[4], sse[4], cost_array[5] = {0, 0, 0, 0, 0};
    ev.probes(&br, &bc, 1, 1u, var, sse);   // upsampled_setup_obmc_center_error
    uint32_t besterr = var[0] + (uint32_t)cost(br, bc), sse1 = sse[0];
    int      distortion = (int)var[0];
    for (int iter = 0; iter < round; ++iter) {
        // left, right, up, down
        int      rows[4] = {br, br, br - hstep, br + hstep}, cols[4] = {bc - hstep, bc + hstep, bc, bc};
        unsigned live = 0;
        for (int idx = 0; idx < 4; ++idx)
            if (in(rows[idx], cols[idx])) live |= 1u << idx;
        ev.probes(rows, cols, 4, live, var, sse);
        for (int idx = 0; idx < 4; ++idx) {
            tr = rows[idx];
            tc = cols[idx];
            if (live >> idx & 1) {
                cost_array[idx] = var[idx] + (uint32_t)cost(tr, tc);
                if (cost_array[idx] < besterr) {
                    best_idx = idx;
                    besterr = cost_array[idx];
                    distortion = (int)var[idx];
                    sse1 = sse[idx];
                }
            } else {
                cost_array[idx] = kIntMax;
            }
        }
        int kc = cost_array[0] <= cost_array[1] ? -hstep : hstep, kr = cost_array[2] <= cost_array[3] ? -hstep : hstep;
        tc = bc + kc;
        tr = br + kr;
        if (in(tr, tc)) {
            ev.probes(&tr, &tc, 1, 1u, var, sse);
            cost_array[4] = var[0] + (uint32_t)cost(tr, tc);
            if (cost_array[4] < besterr) {
                best_idx = 4;
                besterr = cost_array[4];
                distortion = (int)var[0];
                sse1 = sse[0];
            }
        } else {
            cost_array[4] = kIntMax;   // cost_array[idx] with idx == 4 after the loop
        }
        if (best_idx >= 0 && best_idx < 4) {
            br = rows[best_idx];
            bc = cols[best_idx];
        } else if (best_idx == 4) {
            br = tr;
            bc = tc;
        }
        if (best_idx != -1) {   // iters_per_step 2: SECOND_LEVEL_CHECKS_BEST(1)
            const int br0 = br, bc0 = bc;
            if (tr == br && tc != bc) kc = bc - tc;
            else if (tr != br && tc == bc) kr = br - tr;
            int pr[2] = {br0 + kr, br0}, pc[2] = {bc0, bc0 + kc};
            live = (in(pr[0], pc[0]) ? 1u : 0u) | (in(pr[1], pc[1]) ? 2u : 0u);
            ev.probes(pr, pc, 2, live, var, sse);
            const auto check_better = [&](int r, int c, uint32_t v, uint32_t s) {   // CHECK_BETTER1 of a probe inside the range
                const uint32_t total = (uint32_t)cost(r, c) + v;
                if (total < besterr) {
                    besterr = total;
                    br = r;
                    bc = c;
                    distortion = (int)v;
                    sse1 = s;
                }
            };
            for (int k = 0; k < 2; ++k)
                if (live >> k & 1) check_better(pr[k], pc[k], var[k], sse[k]);
            if (br0 != br || bc0 != bc) {
                int r3 = br0 + kr, c3 = bc0 + kc;
                if (in(r3, c3)) {
                    ev.probes(&r3, &c3, 1, 1u, var, sse);
                    check_better(r3, c3, var[0], sse[0]);
                }
            }
        }
        hstep >>= 1;
        best_idx = -1;
    }
    R->row = br;
    R->col = bc;
    R->besterr = besterr;
    R->distortion = distortion;
    R->sse = sse1;
}
// single_motion_search of a job whose status is 0
template <class EV> IBC_HD Result search_job(const EV& ev, const Job& J, int mi_rows, int mi_cols, const int32_t* jc, const int32_t* cc) {
    Result       R = empty_result(STATUS_SEARCHED);
    const Limits L0 = block_limits(J, mi_rows, mi_cols);
    full_pixel_search(ev, J, search_range(L0, J.ref_mv_row, J.ref_mv_col), jc, cc, &R);
    R.row = R.full_row;   // x->best_mv when the sub-pel stage does not run: whole samples, as the reference leaves it
    R.col = R.full_col;
    if (R.bestsme < INT32_MAX) sub_pixel_tree(ev, J, subpel_range(L0, J.ref_mv_row, J.ref_mv_col), jc, cc, &R);
    R.rate_mv = mv_bit_cost(R.row, R.col, J.ref_mv_row, J.ref_mv_col, jc, cc);
    return R;
}

// ---------------------------------------------------------------------------------------------------------------- the serial host form
struct HostEv {
    const uint8_t* y;   // the block's position in the reference plane
    int            stride, bw, bh;
    const int32_t *wsrc, *mask;
    void sads(const int* rows, const int* cols, int n, unsigned live, uint32_t* out) const {
        for (int p = 0; p < n; ++p) {
            if (!(live >> p & 1)) continue;
            const uint8_t* pre = y + (ptrdiff_t)rows[p] * stride + cols[p];
            uint32_t       sad = 0;
            for (int r = 0; r < bh; ++r)
                for (int c = 0; c < bw; ++c) sad += sad_term(wsrc[r * bw + c], mask[r * bw + c], pre[(ptrdiff_t)r * stride + c]);
            out[p] = sad;
        }
    }
    void probes(const int* rows, const int* cols, int n, unsigned live, uint32_t* var, uint32_t* sse) const {
        uint8_t temp[(128 + 7) * 128];   // svt_aom_upsampled_pred_c's intermediate, rows -3 .. bh + 3
        for (int p = 0; p < n; ++p) {
            if (!(live >> p & 1)) continue;
            const int      sx = cols[p] & 7, sy = rows[p] & 7;
            const uint8_t* pre = y + (ptrdiff_t)(rows[p] >> 3) * stride + (cols[p] >> 3);
            if (sx && sy)
                for (int r = 0; r < bh + 7; ++r)
                    for (int c = 0; c < bw; ++c) temp[r * bw + c] = (uint8_t)filter8(pre + (ptrdiff_t)(r - FILTER_REACH_LO) * stride + c, 1, sx);
            uint32_t s = 0;
            int      sum = 0;
            for (int r = 0; r < bh; ++r)
                for (int c = 0; c < bw; ++c) {
                    const uint8_t* q = pre + (ptrdiff_t)r * stride + c;
                    const int      v = sx && sy ? filter8(temp + (r + FILTER_REACH_LO) * bw + c, bw, sy) : (sx ? filter8(q, 1, sx) : (sy ? filter8(q, stride, sy) : (int)*q));
                    const int      d = var_diff(wsrc[r * bw + c], mask[r * bw + c], v);
                    sum += d;
                    s += (uint32_t)(d * d);
                }
            sse[p] = s;
            var[p] = variance_of(s, sum, bw * bh);
        }
    }
};
// the arguments have passed search_args_ok
inline void search_host(const Plane& P, const int32_t* wsrc, const int32_t* mask, int64_t wm_samples, const int32_t* jc, const int32_t* cc, const Job* jobs, int njobs,
                        Result* results) {
    for (int i = 0; i < njobs; ++i) {
        const Job& J = jobs[i];
        const int  status = job_status(J, P, wm_samples);
        if (status != STATUS_SEARCHED) {
            results[i] = empty_result(status);
            continue;
        }
        const HostEv ev{P.ref + (ptrdiff_t)J.mi_row * MI_SIZE * P.stride + J.mi_col * MI_SIZE, P.stride, block_w(J.bsize), block_h(J.bsize), wsrc + J.wm_off, mask + J.wm_off};
        results[i] = search_job(ev, J, P.mi_rows, P.mi_cols, jc, cc);
    }
}

}  // namespace obmc
