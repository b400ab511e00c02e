// intra_dev.h — the AV1 luma intra predictors and the three edge operations as __device__ functions, one call per predicted sample.
//
// Written from the AV1 specification (7.11.2 "Intra prediction process": recursive / DC / smooth / Paeth / directional predictors, the
// intra edge filter, corner filter and up-sampling) and checked bit for bit against the reference's C functions (tests/test_intra_predict_gpu.py):
//   Common/Codec/EbIntraPrediction.c:863-968    dc / v / h / smooth / smooth_v / smooth_h predictors, :246-345 dr_prediction_z1 / z2 / z3
//   Common/Codec/EbIntraPrediction.c:88-110     svt_av1_filter_intra_edge_c, :2288 filter_intra_edge_corner, :78 / :112 the up-sampling and strength rules
//   Common/C_DEFAULT/EbIntraPrediction_c.c:14-55 svt_av1_upsample_intra_edge[_high]_c
// Every function is parametric in the block width / height and in the edge container E (uint8_t, or uint16_t at bit depth 10); an edge pointer
// addresses sample 0, sample -1 is the corner (and -2 exists after up-sampling).  A caller predicts sample (r, c) with predict_sample(); how
// samples are spread over lanes is the caller's business (intra.hip: one lane per column in the picture search, a grid-stride loop in the batch form).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace intra {

#define IPD __device__ __forceinline__

enum { DC_PRED = 0, V_PRED, H_PRED, D45_PRED, D135_PRED, D113_PRED, D157_PRED, D203_PRED, D67_PRED, SMOOTH_PRED, SMOOTH_V_PRED, SMOOTH_H_PRED, PAETH_PRED, N_MODES };
enum { N_TX_SIZES = 19 };

// TxSize -> width / height (AV1 specification, Tx_Width / Tx_Height)
static __device__ const uint8_t kTxW[N_TX_SIZES] = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64};
static __device__ const uint8_t kTxH[N_TX_SIZES] = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16};
// Mode_To_Angle for V_PRED .. D67_PRED
static __device__ const uint8_t kModeAngle[9] = {0, 90, 180, 45, 135, 113, 157, 203, 67};
// Dr_Intra_Derivative[angle >> 1] (AV1 specification 9.3; zero = an angle the codec never produces)
static __device__ const uint16_t kDrDerivative[44] = {0, 1023, 0, 547, 372, 0, 0, 273, 215, 0, 178, 151, 0, 132, 116, 0, 102, 0, 90, 80, 0, 71,
                                                      64, 0, 57, 51, 0, 45, 0, 40, 35, 0, 31, 27, 0, 23, 19, 0, 15, 0, 11, 0, 7, 3};
// Sm_Weights_Tx_4x4 .. Sm_Weights_Tx_64x64 (AV1 specification 9.3), the table of size N starts at N - 4
static __device__ const uint8_t kSmWeights[124] = {
    255, 149, 85, 64,
    255, 197, 146, 105, 73, 50, 37, 32,
    255, 225, 196, 170, 145, 123, 102, 84, 68, 54, 43, 33, 26, 20, 17, 16,
    255, 240, 225, 210, 196, 182, 169, 157, 145, 133, 122, 111, 101, 92, 83, 74, 66, 59, 52, 45, 39, 34, 29, 25, 21, 17, 14, 12, 10, 9, 8, 8,
    255, 248, 240, 233, 225, 218, 210, 203, 196, 189, 182, 176, 169, 163, 156, 150, 144, 138, 133, 127, 121, 116, 111, 106, 101, 96, 91, 86, 82, 77, 73, 69,
    65, 61, 57, 54, 50, 47, 44, 41, 38, 35, 32, 29, 27, 25, 22, 20, 18, 16, 15, 13, 12, 10, 9, 8, 7, 6, 6, 5, 5, 4, 4, 4};

IPD int sm_weight(int n, int i) { return kSmWeights[n - 4 + i]; }
IPD int dr_derivative(int angle) { return kDrDerivative[angle >> 1]; }
IPD int clip_px(int v, int bd) { return min(max(v, 0), (1 << bd) - 1); }

// ------------------------------------------------------------------------------------------------ edge operations
// filter_intra_edge_corner: the value both corners take
template <typename E> IPD int corner_filter(const E* above, const E* left) { return (5 * (int)left[0] + 6 * (int)above[-1] + 5 * (int)above[0] + 8) >> 4; }

// svt_av1_filter_intra_edge(p, sz, strength): sample k of the filtered run; p(k) reads sample k of the UNFILTERED run (0 <= k < sz).
// Sample 0 and a strength of 0 pass through.  Kernels: {0,4,8,4,0} {0,5,6,5,0} {2,4,4,4,2}.
template <typename F> IPD int edge_filter_at(F p, int sz, int strength, int k) {
    if (!strength || k < 1 || k >= sz) return p(k);
    const int k0 = strength == 3 ? 2 : 0, k1 = strength == 2 ? 5 : 4, k2 = strength == 1 ? 8 : (strength == 2 ? 6 : 4);
    const int last = sz - 1;
    const int s = k0 * (p(max(k - 2, 0)) + p(min(k + 2, last))) + k1 * (p(k - 1) + p(min(k + 1, last))) + k2 * p(k);
    return (s + 8) >> 4;
}

// svt_av1_upsample_intra_edge(p, sz): sample idx (-2 <= idx <= 2 * sz - 2) of the up-sampled edge; p(i) reads sample i (-1 <= i < sz) of the input.
template <typename F> IPD int edge_upsample_at(F p, int sz, int idx, int bd) {
    if (idx == -2) return p(-1);
    if (!(idx & 1)) return p(idx >> 1);
    const int i = (idx + 1) >> 1;   // in[] of the specification is p shifted by two, its ends replicated
    const int s = -p(max(i - 2, -1)) + 9 * p(i - 1) + 9 * p(i) - p(min(i + 1, sz - 1));
    return clip_px((s + 8) >> 4, bd);
}

// ------------------------------------------------------------------------------------------------ open-loop macroblock neighbours
// Sample `idx` (-1 .. 31) of the above (which = 0) or left (which = 1) edge of the macroblock at (x, y): update_neighbor_samples_array_open_loop_mb in
// closed form, every quirk kept (EbEncIntraPrediction.c:1201-1280); update_neighbor_samples_array_open_loop_mb_recon (:1282) is the same body on a
// reconstruction plane (tpl.hip).  Reads nothing left of column 0, above row 0, right of column w - 1 or below row h - 1.
IPD int ois_neighbor(const uint8_t* __restrict__ src, int stride, int w, int h, int x, int y, int which, int idx) {
    const int cnt_l = min(32, h - y), cnt_a = min(32, w - x);
    const ptrdiff_t st = stride;
    const uint8_t* p = src + (ptrdiff_t)y * st + x;
    // the left column as the x != 0 branch leaves it: rows beyond the picture keep the 129 fill, the lower half repeats sample 15
    auto left_col = [&](int i) -> int { i = min(i, 15); return i < cnt_l ? (int)p[i * st - 1] : 129; };
    if (x != 0 && y != 0) {
        if (idx < 0) return p[-st - 1];
        if (which) return left_col(idx);
        const int i = min(idx, 15);   // the unknown top-right half repeats sample 15
        return i < cnt_a ? (int)p[i - st] : 127;
    }
    if (x != 0) {   // y == 0: the above row (corner included) is one replicated sample of the left column
        if (which) return idx < 0 ? (int)p[-1] : left_col(idx);
        return idx < cnt_a ? left_col(32 - cnt_a) : 127;
    }
    if (y != 0) {   // x == 0: the left column (corner included) is the sample above the block, the above row is read over its clipped length
        const int v = p[-st];
        if (which) return idx < cnt_l ? v : 129;
        return idx < 0 ? v : (idx < cnt_a ? (int)p[idx - st] : 127);
    }
    return idx < 0 ? 128 : (which ? 129 : 127);
}

// intra_edge_filter_strength(16, 16, delta, 0): block width + height = 32
IPD int ois_strength(int delta) { const int d = abs(delta); return d >= 32 ? 3 : (d >= 4 ? 2 : (d >= 1 ? 1 : 0)); }

// ------------------------------------------------------------------------------------------------ predictors
// What one block's prediction needs besides the edges; uniform over the block.
struct PredParams {
    int mode;      // PredictionMode 0..12
    int bw, bh;
    int p_angle;   // directional modes: base angle + 3 * angle_delta
    int dx, dy;    // directional: dr_derivative of the zone's angles
    int up_above, up_left;
    int dc;        // DC_PRED: the block's value (dc_value())
    int bd;
};

IPD void set_angle(PredParams& P, int p_angle) {
    P.p_angle = p_angle;
    P.dx = p_angle < 90 ? dr_derivative(p_angle) : (p_angle > 90 && p_angle < 180 ? dr_derivative(180 - p_angle) : 1);
    P.dy = p_angle > 90 && p_angle < 180 ? dr_derivative(p_angle - 90) : (p_angle > 180 && p_angle < 270 ? dr_derivative(270 - p_angle) : 1);
}

// dc_pred[have_left][have_above]: DC, DC-left, DC-top, DC-128 from the sums of the two edges
IPD int dc_value(int sum_above, int sum_left, int bw, int bh, int have_left, int have_above, int bd) {
    if (have_left && have_above) return (sum_above + sum_left + ((bw + bh) >> 1)) / (bw + bh);
    if (have_above) return (sum_above + (bw >> 1)) / bw;
    if (have_left) return (sum_left + (bh >> 1)) / bh;
    return 128 << (bd - 8);
}

template <typename E> IPD int pred_paeth(const E* a, const E* l, int r, int c) {
    const int top = a[c], left = l[r], tl = a[-1];
    const int base = top + left - tl;
    const int pl = abs(base - left), pt = abs(base - top), ptl = abs(base - tl);
    return (pl <= pt && pl <= ptl) ? left : (pt <= ptl ? top : tl);
}
template <typename E> IPD int pred_smooth(const E* a, const E* l, int r, int c, int bw, int bh) {
    const int wh = sm_weight(bh, r), ww = sm_weight(bw, c);
    return (wh * (int)a[c] + (256 - wh) * (int)l[bh - 1] + ww * (int)l[r] + (256 - ww) * (int)a[bw - 1] + 256) >> 9;
}
template <typename E> IPD int pred_smooth_v(const E* a, const E* l, int r, int c, int bh) {
    const int wh = sm_weight(bh, r);
    return (wh * (int)a[c] + (256 - wh) * (int)l[bh - 1] + 128) >> 8;
}
template <typename E> IPD int pred_smooth_h(const E* a, const E* l, int r, int c, int bw) {
    const int ww = sm_weight(bw, c);
    return (ww * (int)l[r] + (256 - ww) * (int)a[bw - 1] + 128) >> 8;
}
// zone 1 (0 < angle < 90): along the above edge.  zone 3 (180 < angle < 270) is the same walk along the left edge with rows and columns swapped.
template <typename E> IPD int pred_z1(const E* a, int r, int c, int bw, int bh, int dx, int up, int bd) {
    const int max_base = (bw + bh - 1) << up;
    const int x = dx * (r + 1);
    const int base = (x >> (6 - up)) + (c << up), shift = ((x << up) & 63) >> 1;
    if (base >= max_base) return a[max_base];
    return clip_px(((int)a[base] * (32 - shift) + (int)a[base + 1] * shift + 16) >> 5, bd);
}
// zone 2 (90 < angle < 180): above edge where the projection stays right of the corner, left edge otherwise
template <typename E> IPD int pred_z2(const E* a, const E* l, int r, int c, int dx, int dy, int up_a, int up_l, int bd) {
    const int x = -dx * (r + 1);
    const int base1 = (x >> (6 - up_a)) + (c << up_a);
    int v;
    if (base1 >= -(1 << up_a)) {
        const int shift = ((x * (1 << up_a)) & 63) >> 1;
        v = (int)a[base1] * (32 - shift) + (int)a[base1 + 1] * shift;
    } else {
        const int y = (r << 6) - dy * (c + 1);
        const int base2 = max(y >> (6 - up_l), -(1 << up_l)), shift = ((y * (1 << up_l)) & 63) >> 1;
        v = (int)l[base2] * (32 - shift) + (int)l[base2 + 1] * shift;
    }
    return clip_px((v + 16) >> 5, bd);
}

// Sample (r, c) of the block; `a` / `l` are the conditioned edges.
template <typename E> IPD int predict_sample(const PredParams& P, const E* a, const E* l, int r, int c) {
    switch (P.mode) {
    case DC_PRED: return P.dc;
    case SMOOTH_PRED: return pred_smooth(a, l, r, c, P.bw, P.bh);
    case SMOOTH_V_PRED: return pred_smooth_v(a, l, r, c, P.bh);
    case SMOOTH_H_PRED: return pred_smooth_h(a, l, r, c, P.bw);
    case PAETH_PRED: return pred_paeth(a, l, r, c);
    default: break;
    }
    if (P.p_angle == 90) return a[c];
    if (P.p_angle == 180) return l[r];
    if (P.p_angle < 90) return pred_z1(a, r, c, P.bw, P.bh, P.dx, P.up_above, P.bd);
    if (P.p_angle > 180) return pred_z1(l, c, r, P.bh, P.bw, P.dy, P.up_left, P.bd);
    return pred_z2(a, l, r, c, P.dx, P.dy, P.up_above, P.up_left, P.bd);
}

}  // namespace intra
