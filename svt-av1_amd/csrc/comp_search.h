// comp_search.h — the arithmetic of the masked-compound and inter-intra searches that is the same on the host and on the device, written once: the wedge
// mask set and the smooth inter-intra masks from the AV1 specification, the curve-fit rate/distortion model, and the three searches of
// svt_hip_compound_search_batch_dev.  comp_search.hip runs the sums across a workgroup, svt_hip_compound_search_host (svt_hip_host.cpp) and
// tests/comp_search_host_test.cpp run search_host serially.  Plain C++17, no HIP.  File:line under Source/Lib of the reference:
//   Common/Codec/EbInterPrediction.c:1550-1615   the wedge codebooks and wedge_params_lookup          (specification: Wedge_Codebook, 9.3 "Conversion tables")
//   Common/Codec/EbInterPrediction.c:1672-1734   init_wedge_primary_masks                             (specification 7.11.3.11 "Wedge mask process", MasterMask)
//   Common/Codec/EbInterPrediction.c:1737-1767   init_wedge_signs                                     (7.11.3.11: the flip sign from the first row and column)
//   Common/Codec/EbInterPrediction.c:1770-1809   get_wedge_mask_inplace, init_wedge_masks: the contiguous copies av1_get_contiguous_soft_mask returns
//   Common/Codec/EbInterPrediction.c:1823-1875   ii_weights1d, ii_size_scales, build_smooth_interintra_mask (7.11.3.13 "Intra mode variant mask process", Ii_Weights_1d)
//   Common/Codec/EbInterPrediction.c:78-175      svt_av1_build_compound_diffwtd_mask[_highbd]_c
//   Common/Codec/EbInterPrediction.c:2141-2151   svt_av1_wedge_sse_from_residuals_c
//   Encoder/Codec/EbEncInterPrediction.c:432-503 av1_model_rd_curvfit, model_rd_with_curvfit          Encoder/Codec/EbRateDistortionCost.h:106  RDCOST
//   Encoder/Codec/EbEncInterPrediction.c:517-521, :554-560   svt_av1_wedge_compute_delta_squares_c, svt_av1_wedge_sign_from_residuals_c
//   Encoder/Codec/EbEncInterPrediction.c:562-631, :635-675, :700-756   pick_wedge, pick_wedge_fixed_sign, pick_interinter_seg
//   Encoder/Codec/EbEncInterPrediction.c:819-869, :6120-6162           model_rd_for_sb_with_curvfit (luma), the residual1 / diff10 set-up of calc_pred_masked_compound
//   Encoder/Codec/EbModeDecision.c:214-242, :387-475                   pick_interintra_wedge, the decision part of inter_intra_search
//
// Two things are NOT constants of this file: the grids interp_rgrid_curv[4][65] / interp_dgrid_curv[2][65] and bsize_curvfit_model_cat_lookup[22] of the model
// are the caller's data (svt_hip_set_rd_curvfit_grids); they are not in the specification.
//
// The model's abscissa is svt_log2f((uint32_t)sse_norm / (qstep * qstep)), on the C path (uint32_t)log2(x) (Common/Codec/EbUtility.c:251).  Its argument is 0 whenever
// sse_norm < qstep^2, the common case, and the conversion of -inf to uint32_t is undefined in C.  LOG2_OF_ZERO below pins that case to what the reference's C build
// gives (0, at -O0 and -O2 alike); tests/golden/comp_search.npz, recorded from the running reference, decides it.  docs/kernels/comp_search.md.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/svt_hip.h"

#if defined(__HIPCC__)
#define CS_HD __host__ __device__ inline
#else
#define CS_HD inline
#endif

namespace cs {

using Job = SvtHipCompSearchJob;
using Result = SvtHipCompSearchResult;
using Cand = SvtHipCompSearchCand;

constexpr int KIND_WEDGE = SVT_HIP_COMP_SEARCH_WEDGE, KIND_DIFFWTD = SVT_HIP_COMP_SEARCH_DIFFWTD, KIND_INTERINTRA = SVT_HIP_COMP_SEARCH_INTERINTRA;
constexpr int MAX_CANDS = SVT_HIP_COMP_SEARCH_MAX_CANDS;   // records per job in d_cand: 16 | 2 | 4 + 16
constexpr int BLOCK_SIZES = 22, WEDGE_TYPES = 16, II_MODES = 4, MAX_WEDGE_N = 32 * 32;
constexpr int MAX_JOBS = 1 << 24;
constexpr int GRID_COLS = 65, RATE_CATS = 4, DIST_CATS = 2;
constexpr uint32_t LOG2_OF_ZERO = 0;   // svt_log2f(0) as the reference's C build computes it: see the head of this file

// BlockSize of the reference (Common/Codec/EbDefinitions.h): 4x4 4x8 8x4 8x8 8x16 16x8 16x16 16x32 32x16 32x32 32x64 64x32 64x64 64x128 128x64 128x128 4x16 16x4 8x32 32x8
// 16x64 64x16
constexpr uint8_t kBlockW[BLOCK_SIZES] = {4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64};
constexpr uint8_t kBlockH[BLOCK_SIZES] = {4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16};
CS_HD bool bsize_ok(int b) { return b >= 0 && b < BLOCK_SIZES; }
CS_HD int  block_w(int b) { return kBlockW[b]; }
CS_HD int  block_h(int b) { return kBlockH[b]; }
// the nine sizes with wedges (wedge_params_lookup: bits = 4), in the order init_wedge_masks lays them out; -1 for every other size
CS_HD int wedge_slot(int b) { return b >= 3 && b <= 9 ? b - 3 : (b == 18 ? 7 : (b == 19 ? 8 : -1)); }
CS_HD int imin(int a, int b) { return a < b ? a : b; }
CS_HD int imax(int a, int b) { return a > b ? a : b; }
CS_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------------------------------ wedge masks (specification 7.11.3.11)
// Wedge_Master_Oblique_Odd / _Even / _Vertical
constexpr uint8_t kMasterObliqueOdd[64] = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  1,  2,  6,  18,
                                           37, 53, 60, 63, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64};
constexpr uint8_t kMasterObliqueEven[64] = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  1,  4,  11, 27,
                                            46, 58, 62, 63, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64};
constexpr uint8_t kMasterVertical[64] = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  2,  7,  21,
                                         43, 57, 62, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64};
enum { WEDGE_HORIZONTAL = 0, WEDGE_VERTICAL, WEDGE_OBLIQUE27, WEDGE_OBLIQUE63, WEDGE_OBLIQUE117, WEDGE_OBLIQUE153 };
// Wedge_Codebook: {direction, x offset, y offset} in eighths of the block; [0] blocks taller than wide, [1] wider than tall, [2] square
constexpr uint8_t kWedgeCodebook[3][WEDGE_TYPES][3] = {
    {{WEDGE_OBLIQUE27, 4, 4}, {WEDGE_OBLIQUE63, 4, 4}, {WEDGE_OBLIQUE117, 4, 4}, {WEDGE_OBLIQUE153, 4, 4}, {WEDGE_HORIZONTAL, 4, 2}, {WEDGE_HORIZONTAL, 4, 4},
     {WEDGE_HORIZONTAL, 4, 6}, {WEDGE_VERTICAL, 4, 4}, {WEDGE_OBLIQUE27, 4, 2}, {WEDGE_OBLIQUE27, 4, 6}, {WEDGE_OBLIQUE153, 4, 2}, {WEDGE_OBLIQUE153, 4, 6},
     {WEDGE_OBLIQUE63, 2, 4}, {WEDGE_OBLIQUE63, 6, 4}, {WEDGE_OBLIQUE117, 2, 4}, {WEDGE_OBLIQUE117, 6, 4}},
    {{WEDGE_OBLIQUE27, 4, 4}, {WEDGE_OBLIQUE63, 4, 4}, {WEDGE_OBLIQUE117, 4, 4}, {WEDGE_OBLIQUE153, 4, 4}, {WEDGE_VERTICAL, 2, 4}, {WEDGE_VERTICAL, 4, 4},
     {WEDGE_VERTICAL, 6, 4}, {WEDGE_HORIZONTAL, 4, 4}, {WEDGE_OBLIQUE27, 4, 2}, {WEDGE_OBLIQUE27, 4, 6}, {WEDGE_OBLIQUE153, 4, 2}, {WEDGE_OBLIQUE153, 4, 6},
     {WEDGE_OBLIQUE63, 2, 4}, {WEDGE_OBLIQUE63, 6, 4}, {WEDGE_OBLIQUE117, 2, 4}, {WEDGE_OBLIQUE117, 6, 4}},
    {{WEDGE_OBLIQUE27, 4, 4}, {WEDGE_OBLIQUE63, 4, 4}, {WEDGE_OBLIQUE117, 4, 4}, {WEDGE_OBLIQUE153, 4, 4}, {WEDGE_HORIZONTAL, 4, 2}, {WEDGE_HORIZONTAL, 4, 6},
     {WEDGE_VERTICAL, 2, 4}, {WEDGE_VERTICAL, 6, 4}, {WEDGE_OBLIQUE27, 4, 2}, {WEDGE_OBLIQUE27, 4, 6}, {WEDGE_OBLIQUE153, 4, 2}, {WEDGE_OBLIQUE153, 4, 6},
     {WEDGE_OBLIQUE63, 2, 4}, {WEDGE_OBLIQUE63, 6, 4}, {WEDGE_OBLIQUE117, 2, 4}, {WEDGE_OBLIQUE117, 6, 4}}};

// MasterMask[0][dir][row][col]: WEDGE_OBLIQUE63 is the even / odd row tables shifted a sample every row (16, 15, 15, 14, 14, ...), WEDGE_VERTICAL the vertical table in
// every row; the other four are their transposes, mirrors and complements
inline int master_oblique63(int row, int col) {
    const int shift = 16 - (row >> 1) - (row & 1);
    return (row & 1 ? kMasterObliqueOdd : kMasterObliqueEven)[clampi(col - shift, 0, 63)];
}
inline int master_mask(int dir, int neg, int row, int col) {
    int v;
    switch (dir) {
        case WEDGE_OBLIQUE63: v = master_oblique63(row, col); break;
        case WEDGE_OBLIQUE27: v = master_oblique63(col, row); break;
        case WEDGE_OBLIQUE117: v = 64 - master_oblique63(row, 63 - col); break;
        case WEDGE_OBLIQUE153: v = 64 - master_oblique63(col, 63 - row); break;
        case WEDGE_VERTICAL: v = kMasterVertical[col]; break;
        default: v = kMasterVertical[row]; break;   // WEDGE_HORIZONTAL
    }
    return neg ? 64 - v : v;
}
// sample (y, x) of get_wedge_mask_inplace(index, neg, bsize) before the sign flip is applied
inline int wedge_inplace(int bsize, int index, int neg, int y, int x) {
    const int      bw = block_w(bsize), bh = block_h(bsize);
    const uint8_t* a = kWedgeCodebook[bh > bw ? 0 : (bh < bw ? 1 : 2)][index];
    return master_mask(a[0], neg, 32 - ((a[2] * bh) >> 3) + y, 32 - ((a[1] * bw) >> 3) + x);
}
// the flip sign: 1 when the average of the first row and first column of the primary is below 32
inline int wedge_signflip(int bsize, int index) {
    const int bw = block_w(bsize), bh = block_h(bsize);
    int       avg = 0;
    for (int i = 0; i < bw; ++i) avg += wedge_inplace(bsize, index, 0, 0, i);
    for (int i = 1; i < bh; ++i) avg += wedge_inplace(bsize, index, 0, i, 0);
    avg = (avg + (bw + bh - 1) / 2) / (bw + bh - 1);
    return avg < 32;
}
// the contiguous table: for each wedge size in BlockSize order, for each index, the sign-0 mask then the sign-1 mask, bw * bh bytes each with stride bw
constexpr int WEDGE_TABLE_BYTES = 2 * WEDGE_TYPES * (64 + 128 + 128 + 256 + 512 + 512 + 1024 + 256 + 256);
static_assert(WEDGE_TABLE_BYTES == 100352, "16 indices x 2 signs of the nine sizes");
CS_HD int wedge_offset(int bsize, int sign, int index) {
    if (!bsize_ok(bsize) || wedge_slot(bsize) < 0 || sign < 0 || sign > 1 || index < 0 || index >= WEDGE_TYPES) return -1;
    constexpr int kBase[9] = {0, 64 * 32, 192 * 32, 320 * 32, 576 * 32, 1088 * 32, 1600 * 32, 2624 * 32, 2880 * 32};
    return kBase[wedge_slot(bsize)] + (2 * index + sign) * block_w(bsize) * block_h(bsize);
}
inline void wedge_table_build(uint8_t* dst) {
    for (int bsize = 0; bsize < BLOCK_SIZES; ++bsize) {
        if (wedge_slot(bsize) < 0) continue;
        const int bw = block_w(bsize), bh = block_h(bsize);
        for (int index = 0; index < WEDGE_TYPES; ++index) {
            const int flip = wedge_signflip(bsize, index);
            for (int sign = 0; sign < 2; ++sign) {
                uint8_t* m = dst + wedge_offset(bsize, sign, index);
                for (int y = 0; y < bh; ++y)
                    for (int x = 0; x < bw; ++x) m[y * bw + x] = (uint8_t)wedge_inplace(bsize, index, sign ^ flip, y, x);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ smooth inter-intra masks (7.11.3.13)
// Ii_Weights_1d
constexpr uint8_t kIiWeights1d[128] = {60, 58, 56, 54, 52, 50, 48, 47, 45, 44, 42, 41, 39, 38, 37, 35, 34, 33, 32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 22, 21, 20,
                                       19, 19, 18, 18, 17, 16, 16, 15, 15, 14, 14, 13, 13, 12, 12, 12, 11, 11, 10, 10, 10, 9,  9,  9,  8,  8,  8,  8,  7,  7,  7,  7,
                                       6,  6,  6,  6,  6,  5,  5,  5,  5,  5,  4,  4,  4,  4,  4,  4,  4,  4,  3,  3,  3,  3,  3,  3,  3,  3,  3,  2,  2,  2,  2,  2,
                                       2,  2,  2,  2,  2,  2,  2,  2,  2,  2,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1};
// mode: II_DC_PRED 0, II_V_PRED 1, II_H_PRED 2, II_SMOOTH_PRED 3.  sizeScale = MAX_SB_SIZE / Max(bw, bh)
CS_HD int ii_size_scale(int bsize) { return 128 / imax(block_w(bsize), block_h(bsize)); }
CS_HD int ii_smooth_mask(int mode, int size_scale, int y, int x) {
    if (mode == 1) return kIiWeights1d[y * size_scale];
    if (mode == 2) return kIiWeights1d[x * size_scale];
    if (mode == 3) return kIiWeights1d[imin(y, x) * size_scale];
    return 32;
}
// AOM_BLEND_A64(m, v0, v1) of svt_aom_[highbd_]blend_a64_mask; combine_interintra: v0 = the intra prediction, v1 = the inter prediction
CS_HD int blend_a64(int m, int v0, int v1) { return (m * v0 + (64 - m) * v1 + 32) >> 6; }

// ------------------------------------------------------------------------------------------------------------------ the leaves
// diffwtd_mask[_highbd] with mask_base 38: DIFFWTD_38; DIFFWTD_38_INV is 64 - this
CS_HD int diffwtd_38(int a, int b, int bd) {
    const int diff = (a > b ? a - b : b - a) >> (bd - 8);
    return imin(38 + diff / 16, 64);
}
// svt_av1_wedge_compute_delta_squares_c: r0^2 - r1^2 saturated to int16
CS_HD int delta_square(int r0, int r1) { return clampi(r0 * r0 - r1 * r1, INT16_MIN, INT16_MAX); }
// one term of svt_av1_wedge_sse_from_residuals_c: (64 * r1 + m * d) clamped to int16, squared: at most 2^30
CS_HD uint32_t wedge_sse_term(int r1, int d, int m) {
    const int t = clampi(64 * r1 + m * d, INT16_MIN, INT16_MAX);
    return (uint32_t)(t * t);
}
CS_HD uint64_t wedge_sse_round(uint64_t csse) { return (csse + 2048) >> 12; }   // ROUND_POWER_OF_TWO(csse, 2 * WEDGE_WEIGHT_BITS)
// pick_wedge's sign_limit
CS_HD int64_t sign_limit(uint64_t ss0, uint64_t ss1) { return ((int64_t)ss0 - (int64_t)ss1) * 64 / 2; }

// ------------------------------------------------------------------------------------------------------------------ the model
struct RdTables {
    const double*  rate;   // [4][65]  interp_rgrid_curv
    const double*  dist;   // [2][65]  interp_dgrid_curv
    const int32_t* cat;    // [22]     bsize_curvfit_model_cat_lookup
};
inline bool rd_tables_ok(const double* rate, const double* dist, const int32_t* cat) {
    if (!rate || !dist || !cat) return false;
    for (int i = 0; i < BLOCK_SIZES; ++i)
        if (cat[i] < 0 || cat[i] >= RATE_CATS) return false;
    return true;
}
CS_HD uint32_t log2f_32(uint32_t x) {
    if (!x) return LOG2_OF_ZERO;
    uint32_t n = 0;
    while (x >>= 1) ++n;
    return n;
}
// RDCOST: unsigned 64-bit arithmetic, as the macro's operands make it
CS_HD uint64_t rdcost(uint32_t rm, int rate, int64_t dist) { return (((uint64_t)(int64_t)rate * rm + 256) >> 9) + (uint64_t)dist * 128; }
// model_rd_with_curvfit.  IEEE double throughout, no contraction (-ffp-contract=off on every compile line)
CS_HD void model_rd(const RdTables& T, int bsize, int64_t sse, int n, int quantizer, uint32_t rdmult, int* rate, int64_t* dist) {
    const int qstep = imax(quantizer >> 3, 1);
    if (sse == 0) {
        *rate = 0;
        *dist = 0;
        return;
    }
    const double sse_norm = (double)sse / n;
    double       xqr = (double)log2f_32((uint32_t)sse_norm / (uint32_t)(qstep * qstep));
    // av1_model_rd_curvfit
    const double x_start = -15.5, x_end = 16.5, x_step = 0.5, epsilon = 1e-6;
    const int    rcat = T.cat[bsize], dcat = sse_norm > 16.0;
    xqr = xqr > x_start + x_step + epsilon ? xqr : x_start + x_step + epsilon;
    xqr = xqr < x_end - x_step - epsilon ? xqr : x_end - x_step - epsilon;
    const int    xi = (int)((xqr - x_start) / x_step);   // floor of a positive value
    const double rate_f = T.rate[rcat * GRID_COLS + xi], dist_by_sse_norm_f = T.dist[dcat * GRID_COLS + xi];
    const double dist_f = dist_by_sse_norm_f * sse_norm;
    int          rate_i = (int)((rate_f * n) + 0.5);
    int64_t      dist_i = (int64_t)((dist_f * n) + 0.5);
    // check if skip is better
    if (rate_i == 0) {
        dist_i = sse << 4;
    } else if (rdcost(rdmult, rate_i, dist_i) >= rdcost(rdmult, 0, sse << 4)) {
        rate_i = 0;
        dist_i = sse << 4;
    }
    *rate = rate_i;
    *dist = dist_i;
}
// a candidate from its sse: the model, the extra rate of the caller (0 for the inter-inter kinds), RDCOST
CS_HD Cand candidate(const RdTables& T, const Job& J, int n, int sign, int64_t sse, int extra_rate) {
    int     rate;
    int64_t dist;
    model_rd(T, J.bsize, sse, n, J.quantizer, J.full_lambda, &rate, &dist);
    rate += extra_rate;
    return Cand{sign, rate, sse, dist, (int64_t)rdcost(J.full_lambda, rate, dist)};
}
CS_HD Cand   no_candidate() { return Cand{-1, 0, 0, 0, 0}; }
CS_HD Result empty_result() { return Result{-1, -1, -1, -1, -1, 0, 0, 0}; }
// `rd < best_rd` from INT64_MAX over cands[0 .. n): the first minimum; -1 when nothing is below INT64_MAX
CS_HD int first_min(const Cand* cands, int n, int64_t* best_rd) {
    int     best = -1;
    int64_t rd = INT64_MAX;
    for (int i = 0; i < n; ++i)
        if (cands[i].rd < rd) {
            rd = cands[i].rd;
            best = i;
        }
    *best_rd = best < 0 ? 0 : rd;
    return best;
}

// ------------------------------------------------------------------------------------------------------------------ jobs
// what a job reads: pred0 / pred1 are sample offsets into the predictor pool, blocks stored with stride bw.  Kind 2 reads the four intra predictions II_DC, II_V,
// II_H, II_SMOOTH back to back at pred0 and the inter prediction at pred1, and 16 + 4 rates
CS_HD bool job_ok(const Job& j, int width, int height, int64_t pred_samples, int nrates) {
    if (j.kind < KIND_WEDGE || j.kind > KIND_INTERINTRA || !bsize_ok(j.bsize)) return false;
    const int bw = block_w(j.bsize), bh = block_h(j.bsize), n = bw * bh;
    if (j.kind == KIND_DIFFWTD ? imin(bw, bh) < 8 : wedge_slot(j.bsize) < 0) return false;
    if (j.x < 0 || j.y < 0 || j.x > width - bw || j.y > height - bh) return false;
    if (j.quantizer <= 0 || j.quantizer > INT16_MAX) return false;
    const int64_t n0 = j.kind == KIND_INTERINTRA ? (int64_t)II_MODES * n : n;
    if (j.pred0 < 0 || j.pred1 < 0 || j.pred0 + n0 > pred_samples || (int64_t)j.pred1 + n > pred_samples) return false;
    if (j.kind == KIND_INTERINTRA && (j.wedge_rate < 0 || j.mode_rate < 0 || (int64_t)j.wedge_rate + WEDGE_TYPES > nrates || (int64_t)j.mode_rate + II_MODES > nrates)) return false;
    return true;
}
inline bool fmt_ok(int pix_bytes, int bd) { return (pix_bytes == 1 && bd == 8) || (pix_bytes == 2 && (bd == 8 || bd == 10)); }
// everything svt_hip_compound_search_batch_dev and _host refuse that does not need the context; `jobs` is host memory on both
inline bool search_args_ok(int pix_bytes, int bd, const void* src, int stride, int width, int height, const void* pred, int64_t pred_samples, const int32_t* rates, int nrates,
                           const Job* jobs, int njobs, const Result* results) {
    if (!fmt_ok(pix_bytes, bd) || !src || !pred || !jobs || !results || njobs < 0 || njobs > MAX_JOBS || width < 1 || height < 1 || stride < width || pred_samples < 0 ||
        pred_samples > INT32_MAX || nrates < 0 || (nrates && !rates))
        return false;
    for (int i = 0; i < njobs; ++i)
        if (!job_ok(jobs[i], width, height, pred_samples, nrates)) return false;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------ the serial form
// one job, sample by sample in the reference's order.  cands: MAX_CANDS records, or NULL
template <class PIX> void search_job(int bd, const PIX* src, int stride, const PIX* pred, const int32_t* rates, const uint8_t* masks, const RdTables& T, const Job& J, Result* res,
                                     Cand* cands) {
    const int  bw = block_w(J.bsize), bh = block_h(J.bsize), n = bw * bh;
    const PIX* s = src + (size_t)J.y * stride + J.x;
    Cand       c[MAX_CANDS];
    for (int i = 0; i < MAX_CANDS; ++i) c[i] = no_candidate();
    Result R = empty_result();
    auto   at = [&](int k) { return (int)s[(size_t)(k / bw) * stride + (k % bw)]; };
    if (J.kind == KIND_DIFFWTD) {   // pick_interinter_seg
        const PIX *p0 = pred + J.pred0, *p1 = pred + J.pred1;
        uint64_t   csse[2] = {0, 0};
        for (int k = 0; k < n; ++k) {
            const int r1 = at(k) - p1[k], d = p1[k] - p0[k], m = diffwtd_38(p0[k], p1[k], bd);
            csse[0] += wedge_sse_term(r1, d, m);
            csse[1] += wedge_sse_term(r1, d, 64 - m);
        }
        for (int t = 0; t < 2; ++t) c[t] = candidate(T, J, n, 0, (int64_t)wedge_sse_round(csse[t]), 0);
        R.mask_type = first_min(c, 2, &R.rd);
    } else {
        int16_t r1[MAX_WEDGE_N], d10[MAX_WEDGE_N], ds[MAX_WEDGE_N];
        int     sign_of[WEDGE_TYPES] = {0};
        int     first = 0;
        const PIX* p1 = pred + J.pred1;
        if (J.kind == KIND_WEDGE) {   // pick_wedge
            const PIX* p0 = pred + J.pred0;
            uint64_t   ss0 = 0, ss1 = 0;
            for (int k = 0; k < n; ++k) {
                const int r0 = at(k) - p0[k];
                r1[k] = (int16_t)(at(k) - p1[k]);
                d10[k] = (int16_t)(p1[k] - p0[k]);
                ds[k] = (int16_t)delta_square(r0, r1[k]);
                ss0 += (uint32_t)(r0 * r0);
                ss1 += (uint32_t)(r1[k] * r1[k]);
            }
            const int64_t limit = sign_limit(ss0, ss1);
            for (int w = 0; w < WEDGE_TYPES; ++w) {
                const uint8_t* m = masks + wedge_offset(J.bsize, 0, w);
                int64_t        acc = 0;
                for (int k = 0; k < n; ++k) acc += ds[k] * m[k];
                sign_of[w] = acc > limit;
            }
        } else {   // inter_intra_search: the four smooth blends, then pick_interintra_wedge on the winner's intra prediction
            const int scale = ii_size_scale(J.bsize);
            for (int mode = 0; mode < II_MODES; ++mode) {
                const PIX* intra = pred + J.pred0 + (size_t)mode * n;
                int64_t    sse = 0;
                for (int k = 0; k < n; ++k) {
                    const int diff = at(k) - blend_a64(ii_smooth_mask(mode, scale, k / bw, k % bw), intra[k], p1[k]);
                    sse += diff * diff;
                }
                c[mode] = candidate(T, J, n, 0, sse, rates[J.mode_rate + mode]);
            }
            R.interintra_mode = first_min(c, II_MODES, &R.rd);
            first = II_MODES;
            if (R.interintra_mode >= 0) {
                const PIX* p0 = pred + J.pred0 + (size_t)R.interintra_mode * n;
                for (int k = 0; k < n; ++k) {
                    r1[k] = (int16_t)(at(k) - p1[k]);
                    d10[k] = (int16_t)(p1[k] - p0[k]);
                }
            }
        }
        if (J.kind == KIND_WEDGE || R.interintra_mode >= 0) {
            for (int w = 0; w < WEDGE_TYPES; ++w) {
                const uint8_t* m = masks + wedge_offset(J.bsize, sign_of[w], w);
                uint64_t       csse = 0;
                for (int k = 0; k < n; ++k) csse += wedge_sse_term(r1[k], d10[k], m[k]);
                c[first + w] = candidate(T, J, n, sign_of[w], (int64_t)wedge_sse_round(csse), J.kind == KIND_WEDGE ? 0 : rates[J.wedge_rate + w]);
            }
            if (J.kind == KIND_WEDGE) {
                R.wedge_index = first_min(c, WEDGE_TYPES, &R.rd);
                R.wedge_sign = R.wedge_index < 0 ? -1 : c[R.wedge_index].sign;
            } else {
                R.interintra_wedge_index = first_min(c + first, WEDGE_TYPES, &R.rd_wedge);
            }
        }
    }
    *res = R;
    if (cands)
        for (int i = 0; i < MAX_CANDS; ++i) cands[i] = c[i];
}
// the arguments have passed search_args_ok and rd_tables_ok; masks = the table of wedge_table_build
inline void search_host(int pix_bytes, int bd, const void* src, int stride, const void* pred, const int32_t* rates, const uint8_t* masks, const RdTables& T, const Job* jobs,
                        int njobs, Result* results, Cand* cands) {
    for (int i = 0; i < njobs; ++i) {
        Cand* c = cands ? cands + (size_t)i * MAX_CANDS : nullptr;
        if (pix_bytes == 1) search_job<uint8_t>(bd, (const uint8_t*)src, stride, (const uint8_t*)pred, rates, masks, T, jobs[i], results + i, c);
        else search_job<uint16_t>(bd, (const uint16_t*)src, stride, (const uint16_t*)pred, rates, masks, T, jobs[i], results + i, c);
    }
}

}  // namespace cs
