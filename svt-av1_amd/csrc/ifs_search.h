// ifs_search.h — the arithmetic of the dual interpolation filter search that is the same on the host and on the device, written once: the order of the nine filter
// pairs, the rounding of the four single-reference and the four two-reference convolve branches, the Laplacian rate/distortion model, RDCOST, both decision walks and
// the serial host form of svt_hip_ifs_search_batch_dev.  ifs_search.hip stages windows and horizontal passes in LDS and sums across a workgroup;
// svt_hip_ifs_search_host (svt_hip_host.cpp) and tests/ifs_search_host_test.cpp run search_host serially, sample by sample from the planes.  Plain C++17, no HIP.
// The block-size tables are comp_search.h's and the filter taps interp_kernels.h's: not restated.  File:line under Source/Lib of the reference:
//   Encoder/Codec/EbEncInterPrediction.c:3034-3045   filter_sets                          Common/Codec/filter.h:59-67  av1_make_interp_filters, av1_extract_interp_filter
//   Encoder/Codec/EbEncInterPrediction.c:3047-3297   interpolation_filter_search          :2760-2789  svt_av1_get_switchable_rate (dir 0 = the y filter, dir 1 = the x filter)
//   Encoder/Codec/EbEncInterPrediction.c:2792-2793   RDCOST as this file of the reference defines it
//   Encoder/Codec/EbEncInterPrediction.c:2795-2853, :2855-2875, :2877-2901   model_rd_norm, svt_av1_model_rd_from_var_lapndz, model_rd_from_sse
//   Encoder/Codec/EbEncInterPrediction.c:2903-2996   model_rd_for_sb (luma)
//   Common/Codec/EbInterPrediction.c:349-469, :744-866      svt_av1_[highbd_]convolve_{2d,y,x,2d_copy}_sr_c
//   Common/Codec/EbInterPrediction.c:552-741, :944-1143     svt_av1_[highbd_]jnt_convolve_{2d,y,x,2d_copy}_c
//
// The two decision walks.  order 0 is the `interpolation_search_level && enable_dual_filter` branch: an ascending walk over all nine pairs with a strict `<`, so the
// first minimum wins.  Its second loop (`i = best_dual_mode + 3; i < 9; i += 3`) evaluates again pairs the first loop has already compared against the running
// minimum: each of them gave tmp_rd >= rd then, rd has not grown since, and the same inputs give the same tmp_rd, so `tmp_rd < rd` is false for every one of them.
// It is left out here; the results recorded from the running reference (tests/golden/ifs_search.npz) show the loop running and changing nothing.  order 1 is the `else` branch: a descending walk from
// pair 8 to pair 0 with a strict `<`, so among equals the highest index wins; with dual = 0 only the pairs with equal filters (0, 4, 8) are evaluated.  It sets
// ifs_is_regular_last on every improvement, so after the walk the flag is `the winner is pair 0`.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/svt_hip.h"
#include "comp_search.h"
#include "interp_kernels.h"

#if defined(__HIPCC__)
#define IFS_HD __host__ __device__ inline
#else
#define IFS_HD inline
#endif

namespace ifs {

using Job = SvtHipIfsJob;
using Result = SvtHipIfsResult;
using Cand = SvtHipIfsCand;
using cs::block_h;
using cs::block_w;
using cs::bsize_ok;
using cs::fmt_ok;

constexpr int FILTERS = 3, NCAND = SVT_HIP_IFS_CANDS, MAX_JOBS = 1 << 24;
constexpr int REACH_LO = 3, REACH_HI = 4;   // the border contract: samples read left / above and right / below of every reference block
constexpr int TAPS = 8;
constexpr int ROUND_0 = 3, ROUND_1_SR = 11, ROUND_1_COMP = 7, FILTER_BITS = 7;   // bd <= 10: round_0 = 3; COMPOUND_ROUND1_BITS = 7
static_assert(NCAND == FILTERS * FILTERS, "DUAL_FILTER_SET_SIZE");
// filter_sets[i] = {y filter, x filter}: EIGHTTAP_REGULAR 0, EIGHTTAP_SMOOTH 1, MULTITAP_SHARP 2, the banks 0 .. 2 of interp_kernels.h
IFS_HD int      filter_y(int i) { return i / FILTERS; }
IFS_HD int      filter_x(int i) { return i % FILTERS; }
IFS_HD uint32_t interp_filters(int i) { return (uint32_t)filter_y(i) | ((uint32_t)filter_x(i) << 16); }
// the taps on the host: sizes with both dimensions >= 8 only, so the 4-tap banks 4 and 5 are never reached
constexpr int16_t kTaps[6][16][TAPS] = SVT_HIP_INTERP_TABLE;

IFS_HD int rp2(int v, int n) { return n == 0 ? v : ((v + (1 << (n - 1))) >> n); }
IFS_HD int clip_pixel(int v, int bd) { return v < 0 ? 0 : (v > (1 << bd) - 1 ? (1 << bd) - 1 : v); }

// ------------------------------------------------------------------------------------------------------------------ the convolve branches
// `res` is the plain sum of taps times samples.  The horizontal pass of both 2-D forms: im_block, int16
IFS_HD int im_sample(int res, int bd) { return (int16_t)rp2(res + (1 << (bd + FILTER_BITS - 1)), ROUND_0); }
// single reference: convolve_x_sr, convolve_y_sr, convolve_2d_sr (`sum` = taps times im_block); lowbd keeps the 2-D result in an int16
IFS_HD int sr_x(int res, int bd) { return clip_pixel(rp2(rp2(res, ROUND_0), FILTER_BITS - ROUND_0), bd); }
IFS_HD int sr_y(int res, int bd) { return clip_pixel(rp2(res, FILTER_BITS), bd); }
IFS_HD int sr_2d(int sum, int bd, bool lowbd) {
    const int offset_bits = bd + 2 * FILTER_BITS - ROUND_0;
    int       res = rp2(sum + (1 << offset_bits), ROUND_1_SR) - ((1 << (offset_bits - ROUND_1_SR)) + (1 << (offset_bits - ROUND_1_SR - 1)));
    if (lowbd) res = (int16_t)res;
    return clip_pixel(res, bd);   // bits = 2 * FILTER_BITS - round_0 - round_1 = 0
}
// two references: the 16-bit value of one reference (do_average = 0) in jnt_convolve_2d_copy, _x, _y, _2d
IFS_HD int d16_offset(int bd) {
    const int offset_bits = bd + 2 * FILTER_BITS - ROUND_0;
    return (1 << (offset_bits - ROUND_1_COMP)) + (1 << (offset_bits - ROUND_1_COMP - 1));
}
IFS_HD int d16_copy(int v, int bd) { return (v << (2 * FILTER_BITS - ROUND_1_COMP - ROUND_0)) + d16_offset(bd); }
IFS_HD int d16_x(int res, int bd) { return (1 << (FILTER_BITS - ROUND_1_COMP)) * rp2(res, ROUND_0) + d16_offset(bd); }
IFS_HD int d16_y(int res, int bd) { return rp2(res * (1 << (FILTER_BITS - ROUND_0)), ROUND_1_COMP) + d16_offset(bd); }
IFS_HD int d16_2d(int sum, int bd) { return (uint16_t)rp2(sum + (1 << (bd + 2 * FILTER_BITS - ROUND_0)), ROUND_1_COMP); }
// the do_average branch on the second reference: type 0 the plain average, type 1 use_jnt_comp_avg with fwd_offset / bck_offset (DIST_PRECISION_BITS = 4)
IFS_HD int comp_pixel(int d0, int d1, int type, int fwd, int bck, int bd) {
    int tmp = type ? (d0 * fwd + d1 * bck) >> 4 : (d0 + d1) >> 1;
    tmp -= d16_offset(bd);
    return clip_pixel(rp2(tmp, 2 * FILTER_BITS - ROUND_0 - ROUND_1_COMP), bd);
}

// ------------------------------------------------------------------------------------------------------------------ the model
constexpr int32_t kRateTabQ10[] = {65536, 6086, 5574, 5275, 5063, 4899, 4764, 4651, 4553, 4389, 4255, 4142, 4044, 3958, 3881, 3811, 3748, 3635, 3538, 3453, 3376,
                                   3307,  3244, 3186, 3133, 3037, 2952, 2877, 2809, 2747, 2690, 2638, 2589, 2501, 2423, 2353, 2290, 2232, 2179, 2130, 2084, 2001,
                                   1928,  1862, 1802, 1748, 1698, 1651, 1608, 1530, 1460, 1398, 1342, 1290, 1243, 1199, 1159, 1086, 1021, 963,  911,  864,  821,
                                   781,   745,  680,  623,  574,  530,  490,  455,  424,  395,  345,  304,  269,  239,  213,  190,  171,  154,  126,  104,  87,
                                   73,    61,   52,   44,   38,   28,   21,   16,   12,   10,   8,    6,    5,    3,    2,    1,    1,    1,    0,    0};
constexpr int32_t kDistTabQ10[] = {0,   0,   1,   1,   1,   2,   2,   2,   3,   3,   4,   5,   5,   6,   7,   7,   8,   9,   11,  12,  13,  15,   16,   17,   18,   21,
                                   24,  26,  29,  31,  34,  36,  39,  44,  49,  54,  59,  64,  69,  73,  78,  88,  97,  106, 115, 124,  133,  142,  151,  167,  184,  200,
                                   215, 231, 245, 260, 274, 301, 327, 351, 375, 397, 418, 439, 458, 495, 528, 559, 587, 613, 637,  659,  680,  717,  749,  777,  801,  823,
                                   842, 859, 874, 899, 919, 936, 949, 960, 969, 977, 983, 994, 1001, 1006, 1010, 1013, 1015, 1017, 1018, 1020, 1022, 1022, 1023, 1023, 1023, 1024};
constexpr int32_t kXsqIqQ10[] = {0,     4,     8,     12,    16,    20,    24,    28,    32,    40,    48,    56,    64,    72,    80,    88,    96,     112,    128,    144,    160,
                                 176,   192,   208,   224,   256,   288,   320,   352,   384,   416,   448,   480,   544,   608,   672,   736,   800,    864,    928,    992,    1120,
                                 1248,  1376,  1504,  1632,  1760,  1888,  2016,  2272,  2528,  2784,  3040,  3296,  3552,  3808,  4064,  4576,  5088,   5600,   6112,   6624,   7136,
                                 7648,  8160,  9184,  10208, 11232, 12256, 13280, 14304, 15328, 16352, 18400, 20448, 22496, 24544, 26592, 28640,  30688,  32736,  36832,  40928,  45024,
                                 49120, 53216, 57312, 61408, 65504, 73696, 81888, 90080, 98272, 106464, 114656, 122848, 131040, 147424, 163808, 180192, 196576, 212960, 229344, 245728};
constexpr int MODEL_POINTS = 104;
static_assert(sizeof(kRateTabQ10) == MODEL_POINTS * 4 && sizeof(kDistTabQ10) == MODEL_POINTS * 4 && sizeof(kXsqIqQ10) == MODEL_POINTS * 4, "the three tables have one size");
constexpr uint32_t MAX_XSQ_Q10 = 245727;
IFS_HD int get_msb(uint32_t v) {
    int n = 0;
    while (v >>= 1) ++n;
    return n;
}
// the segment of model_rd_norm an abscissa falls into
IFS_HD int model_xq(int32_t xsq_q10) {
    const int32_t tmp = (xsq_q10 >> 2) + 8;
    const int32_t k = get_msb((uint32_t)tmp) - 3;
    return (k << 3) + ((tmp >> k) & 0x7);
}
IFS_HD void model_rd_norm(int32_t xsq_q10, int32_t* r_q10, int32_t* d_q10) {
    const int32_t tmp = (xsq_q10 >> 2) + 8;
    const int32_t k = get_msb((uint32_t)tmp) - 3;
    const int32_t xq = (k << 3) + ((tmp >> k) & 0x7);
    const int32_t one_q10 = 1 << 10;
    const int32_t a_q10 = ((xsq_q10 - kXsqIqQ10[xq]) << 10) >> (2 + k);
    const int32_t b_q10 = one_q10 - a_q10;
    *r_q10 = (kRateTabQ10[xq] * b_q10 + kRateTabQ10[xq + 1] * a_q10) >> 10;
    *d_q10 = (kDistTabQ10[xq] * b_q10 + kDistTabQ10[xq + 1] * a_q10) >> 10;
}
// the clamped abscissa of svt_av1_model_rd_from_var_lapndz; var > 0
IFS_HD int32_t model_xsq_q10(int64_t var, uint32_t n_log2, uint32_t qstep) {
    const uint64_t xsq_q10_64 = ((((uint64_t)qstep * qstep) << (n_log2 + 10)) + (uint64_t)(var >> 1)) / (uint64_t)var;
    return (int32_t)(xsq_q10_64 < MAX_XSQ_Q10 ? xsq_q10_64 : MAX_XSQ_Q10);
}
IFS_HD void model_rd_from_var_lapndz(int64_t var, uint32_t n_log2, uint32_t qstep, int32_t* rate, int64_t* dist) {
    if (var == 0) {
        *rate = 0;
        *dist = 0;
        return;
    }
    int32_t d_q10, r_q10;
    model_rd_norm(model_xsq_q10(var, n_log2, qstep), &r_q10, &d_q10);
    *rate = ((r_q10 << n_log2) + 1) >> 1;   // ROUND_POWER_OF_TWO(r_q10 << n_log2, 10 - AV1_PROB_COST_SHIFT)
    *dist = (var * (int64_t)d_q10 + 512) >> 10;
}
IFS_HD int num_pels_log2(int bsize) { return get_msb((uint32_t)(block_w(bsize) * block_h(bsize))); }
// model_rd_from_sse with simple_model_rd_from_var = 0
IFS_HD void model_rd_from_sse(int bsize, int quantizer, int bd, uint64_t sse, int32_t* rate, int64_t* dist) {
    model_rd_from_var_lapndz((int64_t)sse, (uint32_t)num_pels_log2(bsize), (uint32_t)(quantizer >> (bd - 5)), rate, dist);
    *dist <<= 4;
}
// RDCOST (AV1_PROB_COST_SHIFT 9, RDDIV_BITS 7): unsigned 64-bit arithmetic, as the macro's operands make it
IFS_HD uint64_t rdcost(uint32_t rm, int rate, int64_t dist) { return (((uint64_t)(int64_t)rate * rm + 256) >> 9) + (uint64_t)dist * 128; }

// ------------------------------------------------------------------------------------------------------------------ candidates and the decision
IFS_HD bool two_refs(const Job& J) { return J.type >= 0; }
// which pairs a job evaluates
IFS_HD bool evaluated(const Job& J, int i) { return !(J.order == 1 && !J.dual && filter_y(i) != filter_x(i)); }
IFS_HD int  switchable_rate(const Job& J, int i) { return J.rate_tab[0][filter_y(i)] + J.rate_tab[1][filter_x(i)]; }
// a pair's record from the sum of squared differences of its prediction, as model_rd_for_sb composes it
IFS_HD Cand candidate(const Job& J, int bd, int i, uint64_t sse) {
    if (!evaluated(J, i)) return Cand{-1, 0, 0, 0};
    int32_t rate;
    int64_t dist;
    model_rd_from_sse(J.bsize, J.quantizer, bd, (sse + ((1ull << (2 * (bd - 8))) >> 1)) >> (2 * (bd - 8)), &rate, &dist);
    rate += switchable_rate(J, i);
    return Cand{rate, (int64_t)sse, dist, (int64_t)rdcost(J.full_lambda, rate, dist)};
}
IFS_HD Result decide(const Job& J, const Cand* c) {
    uint64_t rd = ~(uint64_t)0;
    int      best = 0;   // best_filters starts as 0
    if (J.order == 0) {
        for (int i = 0; i < NCAND; ++i)
            if ((uint64_t)c[i].rd < rd) {
                rd = (uint64_t)c[i].rd;
                best = i;
            }
    } else {
        for (int i = NCAND - 1; i >= 0; --i)
            if (evaluated(J, i) && (uint64_t)c[i].rd < rd) {
                rd = (uint64_t)c[i].rd;
                best = i;
            }
    }
    return Result{best, interp_filters(best), switchable_rate(J, best), J.order == 1 ? (best == 0) : -1, (int64_t)rd};
}
// the distinct predictions: a direction whose phase is 0 on every reference does not see its filter
IFS_HD bool x_filtered(const Job& J) { return J.subpel0_x != 0 || (two_refs(J) && J.subpel1_x != 0); }
IFS_HD bool y_filtered(const Job& J) { return J.subpel0_y != 0 || (two_refs(J) && J.subpel1_y != 0); }
// the pair whose prediction pair i shares (itself when both directions are filtered)
IFS_HD int distinct_of(const Job& J, int i) { return (y_filtered(J) ? filter_y(i) : 0) * FILTERS + (x_filtered(J) ? filter_x(i) : 0); }

// ------------------------------------------------------------------------------------------------------------------ jobs
IFS_HD bool size_ok(int bsize) { return bsize_ok(bsize) && block_w(bsize) >= 8 && block_h(bsize) >= 8; }   // 17 shapes
IFS_HD bool job_ok(const Job& j, int width, int height, bool have_ref1) {
    if (!size_ok(j.bsize)) return false;
    const int bw = block_w(j.bsize), bh = block_h(j.bsize);
    if (j.x < 0 || j.y < 0 || j.x > width - bw || j.y > height - bh) return false;
    if (j.type < -1 || j.type > 1 || (j.type >= 0 && !have_ref1)) return false;
    if (j.subpel0_x < 0 || j.subpel0_x > 15 || j.subpel0_y < 0 || j.subpel0_y > 15) return false;
    if (j.type >= 0 && (j.subpel1_x < 0 || j.subpel1_x > 15 || j.subpel1_y < 0 || j.subpel1_y > 15)) return false;
    if (j.type == 1 && (j.fwd_offset < 0 || j.bck_offset < 0 || j.fwd_offset + j.bck_offset != 16)) return false;
    if (j.order < 0 || j.order > 1) return false;
    if (j.quantizer < 1 || j.quantizer > INT16_MAX) return false;
    return true;
}
// everything svt_hip_ifs_search_batch_dev and _host refuse; `jobs` is host memory on both.  A job's (dst_x, dst_y) is the caller's, like the reference positions
inline bool search_args_ok(int pix_bytes, int bd, const void* src, int src_stride, int width, int height, const void* ref0, int ref0_stride, const void* ref1, int ref1_stride,
                           const void* dst, int dst_stride, const Job* jobs, int njobs, const Result* results) {
    if (!fmt_ok(pix_bytes, bd) || !src || !ref0 || !jobs || !results || njobs < 0 || njobs > MAX_JOBS || width < 1 || height < 1 || src_stride < width || ref0_stride < 1 ||
        (ref1 && ref1_stride < 1) || (dst && dst_stride < 1))
        return false;
    for (int i = 0; i < njobs; ++i)
        if (!job_ok(jobs[i], width, height, ref1 != nullptr)) return false;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------ the device's strips
// ifs_search.hip walks a block in strips of rows: 2048 samples a strip with one reference, 1024 with two.  One reference's window and three horizontal intermediates of a
// strip take slot_elems int16 elements of LDS; LDS_ELEMS_MAX is the largest need of any shape
constexpr int REACH = REACH_LO + REACH_HI;
constexpr int STRIP_SAMPLES_1 = 2048, STRIP_SAMPLES_2 = 1024;
IFS_HD constexpr int strip_rows(int bw, int bh, bool two) { return (two ? STRIP_SAMPLES_2 : STRIP_SAMPLES_1) / bw < bh ? (two ? STRIP_SAMPLES_2 : STRIP_SAMPLES_1) / bw : bh; }
IFS_HD constexpr int slot_elems(int bw, int rows) { return (rows + REACH) * ((bw + REACH) + FILTERS * bw); }
IFS_HD constexpr int job_lds_elems(int bsize, bool two) {
    return (two ? 2 : 1) * slot_elems(cs::kBlockW[bsize], strip_rows(cs::kBlockW[bsize], cs::kBlockH[bsize], two));
}
constexpr int lds_elems_max() {
    int m = 0;
    for (int b = 0; b < cs::BLOCK_SIZES; ++b)
        if (cs::kBlockW[b] >= 8 && cs::kBlockH[b] >= 8)
            for (int two = 0; two < 2; ++two) m = job_lds_elems(b, two != 0) > m ? job_lds_elems(b, two != 0) : m;
    return m;
}
constexpr int LDS_ELEMS_MAX = lds_elems_max();

// ------------------------------------------------------------------------------------------------------------------ the serial form
// sample (r, c) of one reference's block under the pair (fy, fx): the pixel (COMP = false) or the 16-bit value (COMP = true)
template <bool COMP, class PIX> int ref_sample(const PIX* p, int stride, int sx, int sy, int fy, int fx, int r, int c, int bd) {
    const PIX*     q = p + (ptrdiff_t)r * stride + c;
    const int16_t *xf = kTaps[fx][sx], *yf = kTaps[fy][sy];
    if (!sx && !sy) return COMP ? d16_copy(*q, bd) : (int)*q;
    if (!sy) {
        int res = 0;
        for (int k = 0; k < TAPS; ++k) res += xf[k] * q[k - REACH_LO];
        return COMP ? d16_x(res, bd) : sr_x(res, bd);
    }
    if (!sx) {
        int res = 0;
        for (int k = 0; k < TAPS; ++k) res += yf[k] * q[(ptrdiff_t)(k - REACH_LO) * stride];
        return COMP ? d16_y(res, bd) : sr_y(res, bd);
    }
    int sum = 0;
    for (int k = 0; k < TAPS; ++k) {
        const PIX* row = q + (ptrdiff_t)(k - REACH_LO) * stride;
        int        res = 0;
        for (int t = 0; t < TAPS; ++t) res += xf[t] * row[t - REACH_LO];
        sum += yf[k] * im_sample(res, bd);
    }
    return COMP ? d16_2d(sum, bd) : sr_2d(sum, bd, sizeof(PIX) == 1);
}
template <class PIX> int predict_sample(const Job& J, const PIX* ref0, int ref0_stride, const PIX* ref1, int ref1_stride, int i, int r, int c, int bd) {
    const PIX* p0 = ref0 + (ptrdiff_t)J.ref0_y * ref0_stride + J.ref0_x;
    if (!two_refs(J)) return ref_sample<false>(p0, ref0_stride, J.subpel0_x, J.subpel0_y, filter_y(i), filter_x(i), r, c, bd);
    const PIX* p1 = ref1 + (ptrdiff_t)J.ref1_y * ref1_stride + J.ref1_x;
    const int  d0 = ref_sample<true>(p0, ref0_stride, J.subpel0_x, J.subpel0_y, filter_y(i), filter_x(i), r, c, bd);
    const int  d1 = ref_sample<true>(p1, ref1_stride, J.subpel1_x, J.subpel1_y, filter_y(i), filter_x(i), r, c, bd);
    return comp_pixel(d0, d1, J.type, J.fwd_offset, J.bck_offset, bd);
}
// one job: every evaluated pair predicted whole and compared with the source, as the reference does; cands: NCAND records, or NULL
template <class PIX> void search_job(int bd, const PIX* src, int src_stride, const PIX* ref0, int ref0_stride, const PIX* ref1, int ref1_stride, PIX* dst, int dst_stride,
                                     const Job& J, Result* res, Cand* cands) {
    const int  bw = block_w(J.bsize), bh = block_h(J.bsize);
    const PIX* s = src + (size_t)J.y * src_stride + J.x;
    Cand       c[NCAND];
    for (int i = 0; i < NCAND; ++i) {
        uint64_t sse = 0;
        if (evaluated(J, i))
            for (int r = 0; r < bh; ++r)
                for (int x = 0; x < bw; ++x) {
                    const int d = (int)s[(size_t)r * src_stride + x] - predict_sample(J, ref0, ref0_stride, ref1, ref1_stride, i, r, x, bd);
                    sse += (uint32_t)(d * d);
                }
        c[i] = candidate(J, bd, i, sse);
    }
    const Result R = decide(J, c);
    *res = R;
    if (cands)
        for (int i = 0; i < NCAND; ++i) cands[i] = c[i];
    if (dst)
        for (int r = 0; r < bh; ++r)
            for (int x = 0; x < bw; ++x)
                dst[(ptrdiff_t)(J.dst_y + r) * dst_stride + J.dst_x + x] = (PIX)predict_sample(J, ref0, ref0_stride, ref1, ref1_stride, R.best, r, x, bd);
}
// the arguments have passed search_args_ok
inline void search_host(int pix_bytes, int bd, const void* src, int src_stride, const void* ref0, int ref0_stride, const void* ref1, int ref1_stride, void* dst, int dst_stride,
                        const Job* jobs, int njobs, Result* results, Cand* cands) {
    for (int i = 0; i < njobs; ++i) {
        Cand* c = cands ? cands + (size_t)i * NCAND : nullptr;
        if (pix_bytes == 1)
            search_job<uint8_t>(bd, (const uint8_t*)src, src_stride, (const uint8_t*)ref0, ref0_stride, (const uint8_t*)ref1, ref1_stride, (uint8_t*)dst, dst_stride, jobs[i],
                                results + i, c);
        else
            search_job<uint16_t>(bd, (const uint16_t*)src, src_stride, (const uint16_t*)ref0, ref0_stride, (const uint16_t*)ref1, ref1_stride, (uint16_t*)dst, dst_stride, jobs[i],
                                 results + i, c);
    }
}

}  // namespace ifs
