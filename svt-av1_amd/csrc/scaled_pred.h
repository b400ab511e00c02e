// scaled_pred.h — the arithmetic of inter prediction from a reference of another size, each formula once for the host (svt_hip_scale_factors,
// svt_hip_scaled_block_params) and the device (csrc/scaled_pred.hip).  Plain C++17; under hipcc the functions are __host__ __device__.
// Reference: Common/Codec/EbInterPrediction.c:178-241 (scale factors, scaled_x / scaled_y), :471-550 / :867-946 (svt_av1_[highbd_]convolve_2d_scale_c),
// Common/Codec/EbInterPrediction.h:169 (valid_ref_frame_size), Common/Codec/convolve.h:44 (get_conv_params_no_round),
// Encoder/Codec/EbEncInterPrediction.c:3591-3661 (compute_subpel_params, the scaled branch).
#pragma once
#include <stdint.h>
#include "../../include/svt_hip.h"

#if defined(__HIPCC__)
#define SP_HD __host__ __device__ inline
#else
#define SP_HD inline
#endif

enum {
    SP_REF_SCALE_SHIFT = 14, SP_REF_NO_SCALE = 1 << 14, SP_REF_INVALID_SCALE = -1,
    SP_SUBPEL_BITS = 4, SP_SCALE_SUBPEL_BITS = 10, SP_SCALE_SUBPEL_MASK = 1023, SP_SCALE_EXTRA_BITS = 6, SP_SCALE_EXTRA_OFF = 32,
    SP_INTERP_EXTEND = 4, SP_BORDER = 288,   // AOM_INTERP_EXTEND, AOM_BORDER_IN_PIXELS
    SP_FILTER_BITS = 7, SP_TAPS = 8, SP_COMPOUND_ROUND1_BITS = 7, SP_DIST_PRECISION_BITS = 4,
    SP_MAX_STEP = 2048, SP_MAX_BLOCK = 128
};

// ---- scale factors
SP_HD bool sp_valid_ref_frame_size(int ref_w, int ref_h, int this_w, int this_h) {
    return 2 * this_w >= ref_w && 2 * this_h >= ref_h && this_w <= 16 * ref_w && this_h <= 16 * ref_h;
}
SP_HD int32_t sp_fixed_point_scale_factor(int32_t other_size, int32_t this_size) { return ((other_size << SP_REF_SCALE_SHIFT) + this_size / 2) / this_size; }
SP_HD int32_t sp_coarse_step(int32_t scale_fp) { return (scale_fp + (1 << (SP_REF_SCALE_SHIFT - SP_SCALE_SUBPEL_BITS - 1))) >> (SP_REF_SCALE_SHIFT - SP_SCALE_SUBPEL_BITS); }
// false (and the invalid mark) for a pair the reference refuses
SP_HD bool sp_scale_factors(int other_w, int other_h, int this_w, int this_h, SvtHipScaleFactors* sf) {
    if (other_w < 1 || other_h < 1 || this_w < 1 || this_h < 1 || other_w > 65535 || other_h > 65535 || this_w > 65535 || this_h > 65535 ||
        !sp_valid_ref_frame_size(other_w, other_h, this_w, this_h)) {
        sf->x_scale_fp = sf->y_scale_fp = SP_REF_INVALID_SCALE;
        sf->x_step_q4 = sf->y_step_q4 = 0;
        return false;
    }
    sf->x_scale_fp = sp_fixed_point_scale_factor(other_w, this_w);
    sf->y_scale_fp = sp_fixed_point_scale_factor(other_h, this_h);
    sf->x_step_q4 = sp_coarse_step(sf->x_scale_fp);
    sf->y_step_q4 = sp_coarse_step(sf->y_scale_fp);
    return true;
}
SP_HD bool sp_scale_factors_ok(const SvtHipScaleFactors& sf) {
    return sf.x_scale_fp >= SP_REF_NO_SCALE / 16 && sf.x_scale_fp <= 2 * SP_REF_NO_SCALE && sf.y_scale_fp >= SP_REF_NO_SCALE / 16 && sf.y_scale_fp <= 2 * SP_REF_NO_SCALE &&
           sf.x_step_q4 == sp_coarse_step(sf.x_scale_fp) && sf.y_step_q4 == sp_coarse_step(sf.y_scale_fp);
}

// ---- scaled values: val in q4 -> 1/1024 sample.  ROUND_POWER_OF_TWO_SIGNED_64: positions left of and above the picture are negative
SP_HD int64_t sp_round_pow2_signed_64(int64_t v, int n) { return v < 0 ? -((-v + ((int64_t)1 << (n - 1))) >> n) : (v + ((int64_t)1 << (n - 1))) >> n; }
SP_HD int32_t sp_scaled(int32_t val, int32_t scale_fp) {
    const int32_t off = (scale_fp - SP_REF_NO_SCALE) * (1 << (SP_SUBPEL_BITS - 1));
    const int64_t tval = (int64_t)val * scale_fp + off;
    return (int32_t)sp_round_pow2_signed_64(tval, SP_REF_SCALE_SHIFT - SP_SCALE_EXTRA_BITS);
}

// ---- the scaled branch of compute_subpel_params along one axis: pre = the block's position in the plane, mv in 1/8 luma sample, ss the plane's
// sub-sampling, frame = the luma size.  -> integer position, phase 0 .. 1023
SP_HD void sp_block_axis(int pre, int mv, int ss, int frame, int32_t scale_fp, int32_t* pos, int32_t* subpel) {
    const int orig = (pre << SP_SUBPEL_BITS) + mv * (1 << (1 - ss));
    int p = sp_scaled(orig, scale_fp) + SP_SCALE_EXTRA_OFF;
    const int lo = -(((SP_BORDER >> ss) - SP_INTERP_EXTEND) << SP_SCALE_SUBPEL_BITS), hi = ((frame >> ss) + SP_INTERP_EXTEND) << SP_SCALE_SUBPEL_BITS;
    p = p < lo ? lo : p > hi ? hi : p;
    *subpel = p & SP_SCALE_SUBPEL_MASK;
    *pos = p >> SP_SCALE_SUBPEL_BITS;
}
SP_HD void sp_block_params(const SvtHipScaleFactors& sf, int pre_x, int pre_y, int mv_row, int mv_col, int ss_x, int ss_y, int frame_w, int frame_h, int32_t* pos_x,
                           int32_t* pos_y, int32_t* subpel_x, int32_t* subpel_y, int32_t* xs, int32_t* ys) {
    sp_block_axis(pre_y, mv_row, ss_y, frame_h, sf.y_scale_fp, pos_y, subpel_y);
    sp_block_axis(pre_x, mv_col, ss_x, frame_w, sf.x_scale_fp, pos_x, subpel_x);
    *xs = sf.x_step_q4;
    *ys = sf.y_step_q4;
}
// one record -> one job (svt_hip_scaled_jobs_dev)
SP_HD SvtHipScaledBlk sp_job_of_record(const SvtHipScaledRec& r, const SvtHipScaleFactors& sf0, const SvtHipScaleFactors& sf1, int fw0, int fh0, int fw1, int fh1) {
    SvtHipScaledBlk b = {};
    int32_t px, py, sx, sy, xs, ys;
    sp_block_params(sf0, r.pre_x, r.pre_y, r.mv0_row, r.mv0_col, r.ss_x, r.ss_y, fw0, fh0, &px, &py, &sx, &sy, &xs, &ys);
    b.pos0_x = px; b.pos0_y = py; b.subpel0_x = (uint16_t)sx; b.subpel0_y = (uint16_t)sy; b.xs0 = (uint16_t)xs; b.ys0 = (uint16_t)ys;
    if (r.compound) {
        sp_block_params(sf1, r.pre_x, r.pre_y, r.mv1_row, r.mv1_col, r.ss_x, r.ss_y, fw1, fh1, &px, &py, &sx, &sy, &xs, &ys);
        b.pos1_x = px; b.pos1_y = py; b.subpel1_x = (uint16_t)sx; b.subpel1_y = (uint16_t)sy; b.xs1 = (uint16_t)xs; b.ys1 = (uint16_t)ys;
    }
    b.dst_x = r.dst_x; b.dst_y = r.dst_y; b.w = r.w; b.h = r.h; b.bank_x = r.bank_x; b.bank_y = r.bank_y;
    b.compound = r.compound; b.fwd_offset = r.fwd_offset; b.bck_offset = r.bck_offset;
    return b;
}

// ---- where sample i of a run that starts at phase `subpel` with step `step` reads: first tap row / column (relative to pos - 3) and filter index
SP_HD int sp_tap0(int subpel, int step, int i) { return (subpel + i * step) >> SP_SCALE_SUBPEL_BITS; }
SP_HD int sp_filter_idx(int subpel, int step, int i) { return ((subpel + i * step) & SP_SCALE_SUBPEL_MASK) >> SP_SCALE_EXTRA_BITS; }
// samples a run of n outputs needs along its axis, from pos - 3 on (im_h of the reference, and the same along x)
SP_HD int sp_span(int subpel, int step, int n) { return (((n - 1) * step + subpel) >> SP_SCALE_SUBPEL_BITS) + SP_TAPS; }

// ---- sample arithmetic of the two convolve functions, once for every format.  round_0 / round_1 as get_conv_params_no_round sets them: round_0 = 3, and
// 5 at bit depth 12 (intbufrange = bd + 7 - 3 + 2 > 16); round_1 = COMPOUND_ROUND1_BITS for a compound block, else 14 - round_0
template <int BD> struct SpRound {
    static constexpr int r0 = BD == 12 ? 5 : 3;
    static constexpr int offset_bits = BD + 2 * SP_FILTER_BITS - r0;
    static constexpr int r1(bool compound) { return compound ? SP_COMPOUND_ROUND1_BITS : 2 * SP_FILTER_BITS - r0; }
    static constexpr int bits(bool compound) { return 2 * SP_FILTER_BITS - r0 - r1(compound); }
    static constexpr int round_offset(bool compound) { return (1 << (offset_bits - r1(compound))) + (1 << (offset_bits - r1(compound) - 1)); }
};
SP_HD int sp_rp2(int v, int n) { return n == 0 ? v : (v + (1 << (n - 1))) >> n; }
// horizontal: s[0 .. 7] = the eight samples from tap 0 on; kept as int16 (im_block)
template <int BD, class F, class S> SP_HD int16_t sp_horiz(const F* f, const S* s) {
    int sum = 1 << (BD + SP_FILTER_BITS - 1);
    for (int k = 0; k < SP_TAPS; k++) sum += f[k] * (int)s[k];
    return (int16_t)sp_rp2(sum, SpRound<BD>::r0);
}
// vertical: im[0], im[pitch], ... = the eight intermediate rows from tap 0 on -> the CONV_BUF_TYPE value (16 bits)
template <int BD, class F> SP_HD int sp_vert(const F* f, const int16_t* im, int pitch, bool compound) {
    int sum = 1 << SpRound<BD>::offset_bits;
    for (int k = 0; k < SP_TAPS; k++) sum += f[k] * (int)im[k * pitch];
    return (int)(uint16_t)sp_rp2(sum, SpRound<BD>::r1(compound));
}
// the two ways a compound pair is combined, then "subtract round offset and convolve round" and the clip; for a single reference res is the value itself
SP_HD int sp_combine(int d0, int d1, int compound, int fwd, int bck) { return compound == 2 ? (d0 * fwd + d1 * bck) >> SP_DIST_PRECISION_BITS : (d0 + d1) >> 1; }
template <int BD> SP_HD int sp_final(int res, bool compound) {
    const int v = sp_rp2(res - SpRound<BD>::round_offset(compound), SpRound<BD>::bits(compound));
    return v < 0 ? 0 : v > (1 << BD) - 1 ? (1 << BD) - 1 : v;
}
