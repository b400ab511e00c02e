// tpl.hip — the look-ahead's TPL flow dispenser for one picture; gfx950 (wave64).
//
// Replaces (file:line under Source/Lib of the reference):
//   Encoder/Codec/EbRateControlProcess.c:344-816     tpl_mc_flow_dispenser, with :86 get_quantize_error, :114 rate_estimator, :130 result_model_store,
//                                                    :287 get_best_reference
//   Encoder/Codec/EbEncIntraPrediction.c:1282        update_neighbor_samples_array_open_loop_mb_recon (intra_dev.h: ois_neighbor on the reconstruction)
//   Common/Codec/EbIntraPrediction.c:2545-2632       filter_intra_edge, intra_prediction_open_loop_mb
//   Encoder/Codec/EbTransforms.c:3827                svt_av1_wht_fwd_txfm (16x16 DCT_DCT) + svt_aom_satd, EbFullLoop.c:314 svt_av1_quantize_fp,
//   Common/Codec/EbInvTransforms.c:2455              the 16x16 inverse transform + reconstruction (av1_inv_transform_recon8bit)
//
// The reference walks the macroblocks one at a time.  Only an INTRA macroblock reads this picture's reconstruction (left, above, above-left, and in column 0
// the above-right macroblock); an inter macroblock copies from another frame.  So:
//   phase A, one launch: every macroblock's inter search and decision; inter macroblocks are finished (reconstruction and statistics) here.
//   phase B, one launch per step d = x + 2y (macroblock coordinates): the intra macroblocks of the step.  Left is step d - 1, above d - 2, above-left d - 3,
//            column 0's above-right d - 1: kernel boundaries on the stream are the only ordering, no workgroup waits for another.
// Mapping: a 16-lane row = one macroblock.  Lane = column for the residual and the column transform, the 16 lanes meet through a padded 16 x 17 dword LDS tile,
// lane = row for the row transform, the quantiser and the row pass of the inverse, lane = column again for the reconstruction.  The winning reference's
// coefficients stay in registers (one row of 16 per lane).  Control flow is uniform over a workgroup wherever a barrier follows: a row without work computes
// on addresses that are always readable and stores nothing.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "lane_reduce.h"
#include "txfm_1d.h"
#include "quant_dev.h"
#include "intra_dev.h"

namespace {

using namespace intra;

constexpr int TPL_TILE = 16 * 17;   // dwords per row: stride 17 keeps the column-wise store and the row-wise load conflict free
constexpr int TPL_EDGE = 48;        // bytes per edge: sample i at [16 + i], i = -1 .. 31
constexpr int TPL_ROWS_A = 16, TPL_ROWS_B = 4;
constexpr uint8_t TPL_INTER = 0xFF; // decision byte of an inter macroblock; an intra macroblock's byte is its mode

// Inverse of the 16x16 default scan (AV1 specification 9.3, Default_Scan_16x16): anti-diagonals, odd ones walked downwards, even ones upwards.
struct Iscan16 { uint8_t v[256]; };
constexpr Iscan16 make_iscan16() {
    Iscan16 s{};
    int k = 0;
    for (int d = 0; d < 31; d++) {
        const int lo = d > 15 ? d - 15 : 0, hi = d < 15 ? d : 15;
        for (int i = lo; i <= hi; i++) {
            const int r = (d & 1) ? i : hi + lo - i;
            s.v[r * 16 + (d - r)] = (uint8_t)k++;
        }
    }
    return s;
}
__device__ const Iscan16 kIscan16 = make_iscan16();

struct TplArgs {
    int w, h, pad, mb_cols, mb_rows;
    int use_ois, add_residual, rate, best_ref_only;
    uint32_t present;   // bit r: slot r in use
    SvtHipQuantParams q;
    const uint8_t* cur; int cur_stride;
    SvtHipTplRef refs[7];
    const uint32_t* mv; const uint8_t* mask; const uint8_t* ois_mode; const int32_t* ois_cost;
    uint8_t* recon; int recon_stride;
    SvtHipTplMbStats* stats;
    uint8_t* decision;
};

__device__ __forceinline__ int64_t row_add64(int64_t v) {   // lanes_sum<16> with the low half shuffled first: the header's order gives the kernels other code
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const uint32_t lo = lane_xor((uint32_t)v, o), hi = lane_xor((uint32_t)((uint64_t)v >> 32), o);
        v += (int64_t)(((uint64_t)hi << 32) | lo);
    }
    return v;
}

// 16x16 DCT_DCT of a residual (fwd_shift_16x16 = {2, -2, 0}, cos bits 13 / 12).  In: lane = column, res[r].  Out: lane = row, coef[c].
// Every thread of the workgroup calls it (two barriers); `tile` is the row's own 16 x 17 dwords.
__device__ __forceinline__ void fwd16(int32_t* __restrict__ tile, int lane, const int (&res)[16], int32_t (&coef)[16]) {
    int32_t in[16], out[16];
    // a residual is within +-255: the 16-bit sign extension is exact and keeps the transform's multiplies on the 24-bit path (see intra.hip)
#pragma unroll
    for (int r = 0; r < 16; r++) in[r] = (int32_t)(int16_t)res[r] * 4;
    tx1d::fwd_dct<16, 13>(in, out);
#pragma unroll
    for (int r = 0; r < 16; r++) tile[r * 17 + lane] = tx1d::rshift_round(out[r], 2);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 16; c++) in[c] = (int32_t)(int16_t)tile[lane * 17 + c];
    tx1d::fwd_dct<16, 12>(in, coef);
    __syncthreads();
}

// get_quantize_error + rate_estimator on the row-distributed coefficients: svt_av1_quantize_fp, eob by the default scan, svt_av1_block_error >> 2 clamped
// to >= 1, and 1 + the sum over scan positions below eob of (int)(log1p(|level|) / log(2.0)) + 1 = the bit length of |level| + 1 (levels are below 2^13;
// tests/test_tpl_ref_cpu.py pins the equality), << AV1_PROB_COST_SHIFT.
__device__ __forceinline__ void quant16(const SvtHipQuantParams& qp_arg, int lane, const int32_t (&coef)[16], int32_t (&dq)[16], int want_rate, int& eob, int64_t& err,
                                        int64_t& rate) {
    // the entry point admits variant 2 with log_scale 0 only: saying so here drops quant_one's other three branches and the tables they read
    SvtHipQuantParams qp = {};
    qp.variant = 2; qp.log_scale = 0;
    qp.round[0] = qp_arg.round[0]; qp.round[1] = qp_arg.round[1]; qp.quant[0] = qp_arg.quant[0]; qp.quant[1] = qp_arg.quant[1];
    qp.dequant[0] = qp_arg.dequant[0]; qp.dequant[1] = qp_arg.dequant[1];
    int32_t lv[16];
    int e = 0;
    int64_t se = 0;
#pragma unroll
    for (int c = 0; c < 16; c++) {
        const int rc = lane * 16 + c;
        int32_t dq_abs;
        lv[c] = quant_one(qp, coef[c], rc != 0, dq_abs);
        dq[c] = coef[c] < 0 ? -dq_abs : dq_abs;
        if (lv[c]) e = max(e, (int)kIscan16.v[rc] + 1);
        const int64_t d = (int64_t)coef[c] - dq[c];
        se += d * d;
    }
    e = lanes_max<16>(e);
    se = row_add64(se);
    int bits = 0;
#pragma unroll
    for (int c = 0; c < 16; c++)
        if ((int)kIscan16.v[lane * 16 + c] < e) bits += 32 - __clz(lv[c] + 1);
    bits = lanes_sum<16>(bits);
    eob = e;
    err = max(se >> 2, (int64_t)1);
    rate = want_rate ? (int64_t)(1 + bits) << 9 : 0;
}

// The inverse of fwd16 at bit depth 8 (inv_shift_16x16 = {-2, -4}, cos bit 12, stage ranges 16): in lane = row, dq[c]; out lane = column, the residual
// samples rsd[r] as inv_txfm2d_add adds them (range check of :2398 included).  Two barriers.
__device__ __forceinline__ void inv16(int32_t* __restrict__ tile, int lane, const int32_t (&dq)[16], int32_t (&rsd)[16]) {
    int32_t in[16], out[16];
#pragma unroll
    for (int c = 0; c < 16; c++) in[c] = tx1d::clampv<16>(dq[c]);
    tx1d::inv_dct<16, 12, 16>(in, out);
#pragma unroll
    for (int c = 0; c < 16; c++) tile[lane * 17 + c] = tx1d::rshift_round(out[c], 2);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; r++) in[r] = tx1d::clampv<16>(tile[r * 17 + lane]);
    tx1d::inv_dct<16, 12, 16>(in, out);
    constexpr int32_t res_max = (1 << 15) - 1 + (914 << 1), res_min = -res_max - 1;
#pragma unroll
    for (int r = 0; r < 16; r++) rsd[r] = min(max(tx1d::rshift_round(out[r], 4), res_min), res_max);
    __syncthreads();
}

// The second half of the reference's loop body (:752-785) for a macroblock whose prediction column is in registers: transform of source - prediction,
// quantiser, error, rate, and the reconstruction = prediction (+ inverse transform where eob != 0) written to dst.  Every thread of the workgroup calls it.
__device__ __forceinline__ void recon_pass(int32_t* __restrict__ tile, int lane, const TplArgs& A, const int (&cur)[16], const int (&pred)[16], bool store,
                                           uint8_t* dst, int dst_stride, int& eob, int64_t& err, int64_t& rate) {
    int res[16];
    int32_t coef[16], dq[16], rsd[16];
#pragma unroll
    for (int r = 0; r < 16; r++) { res[r] = cur[r] - pred[r]; rsd[r] = 0; }
    fwd16(tile, lane, res, coef);
    quant16(A.q, lane, coef, dq, A.rate, eob, err, rate);
    const bool add = store && A.add_residual && eob != 0;
    if (__syncthreads_or(add)) inv16(tile, lane, dq, rsd);   // workgroup-uniform
    if (store) {
#pragma unroll
        for (int r = 0; r < 16; r++) dst[(ptrdiff_t)r * dst_stride] = (uint8_t)min(max(pred[r] + (add ? rsd[r] : 0), 0), 255);
    }
}

// ================================================================================================ phase A
__global__ __launch_bounds__(TPL_ROWS_A * 16) void tpl_inter_kernel(const TplArgs A) {
    __shared__ int32_t tiles[TPL_ROWS_A * TPL_TILE];
    const int row = threadIdx.x >> 4, lane = threadIdx.x & 15;
    int32_t* tile = tiles + row * TPL_TILE;
    const int n_mb = A.mb_cols * A.mb_rows;
    const int mb0 = blockIdx.x * TPL_ROWS_A + row;
    const bool live = mb0 < n_mb;
    const int mb = live ? mb0 : 0;
    const int x = (mb % A.mb_cols) * 16, y = (mb / A.mb_cols) * 16;
    const uint8_t* curp = A.cur + (ptrdiff_t)y * A.cur_stride + x + lane;
    int cur[16];
#pragma unroll
    for (int r = 0; r < 16; r++) cur[r] = curp[(ptrdiff_t)r * A.cur_stride];
    const uint32_t mask = A.present && live ? (uint32_t)A.mask[mb] & A.present : 0u;

    // slot s of the kernel argument, read from the kernel-argument segment itself: an index into the by-value copy would move all of it to private memory,
    // and a select chain over the seven slots keeps 42 scalar registers alive through the transforms (the argument is the kernel's only one: offset 0)
    const SvtHipTplRef* slots = (const SvtHipTplRef*)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TplArgs, refs));
    auto ref_of = [&](int s, bool rec, const uint8_t*& p, int& stride) {
        const SvtHipTplRef R = slots[s];
        p = rec ? R.d_rec : R.d_src; stride = rec ? R.rec_stride : R.src_stride;
    };
    // the block position an MV word names: ((int16_t)(mv << 1)) >> 3, kept inside the padded plane
    auto block_at = [&](uint32_t word, int& bx, int& by, int& mvx, int& mvy) {
        mvx = (int16_t)((int16_t)(word & 0xffff) << 1); mvy = (int16_t)((int16_t)(word >> 16) << 1);
        bx = min(max(x + (mvx >> 3), -A.pad), A.w + A.pad - 16);
        by = min(max(y + (mvy >> 3), -A.pad), A.h + A.pad - 16);
    };

    // ---- get_best_reference: the valid slot with the smallest 16x16 SAD, the first one on ties
    int win = -1;
    if (A.best_ref_only) {
        uint32_t best_sad = 0xffffffffu;
        for (int s = 0; s < 7; s++) {
            if (!((A.present >> s) & 1)) continue;   // uniform
            const bool valid = (mask >> s) & 1;
            const uint8_t* p = curp; int stride = A.cur_stride;
            if (valid) {
                int bx, by, mvx, mvy;
                block_at(A.mv[(size_t)s * n_mb + mb], bx, by, mvx, mvy);
                ref_of(s, false, p, stride);
                p += (ptrdiff_t)by * stride + bx + lane;
            }
            int sad = 0;
#pragma unroll
            for (int r = 0; r < 16; r++) sad += abs(cur[r] - (int)p[(ptrdiff_t)r * stride]);
            sad = lanes_sum<16>(sad);
            if (valid && (uint32_t)sad < best_sad) { best_sad = (uint32_t)sad; win = s; }
        }
    }

    // ---- the inter costs: SATD of the transformed residual against the reference's source picture; the first smallest cost wins
    int best_rf = -1, best_cost = 0x7fffffff, best_bx = 0, best_by = 0, best_mvx = 0, best_mvy = 0;
    int32_t best[16];
#pragma unroll
    for (int c = 0; c < 16; c++) best[c] = 0;
    const int niter = A.best_ref_only ? 1 : 7;
    for (int it = 0; it < niter; it++) {
        if (!A.best_ref_only && !((A.present >> it) & 1)) continue;   // uniform
        const int s = A.best_ref_only ? max(win, 0) : it;
        const bool valid = A.best_ref_only ? win >= 0 : ((mask >> s) & 1) != 0;
        if (!__syncthreads_or(valid)) continue;
        const uint8_t* p = curp; int stride = A.cur_stride;
        int bx = 0, by = 0, mvx = 0, mvy = 0;
        if (valid) {
            block_at(A.mv[(size_t)s * n_mb + mb], bx, by, mvx, mvy);
            ref_of(s, false, p, stride);
            p += (ptrdiff_t)by * stride + bx + lane;
        }
        int res[16];
        int32_t coef[16];
#pragma unroll
        for (int r = 0; r < 16; r++) res[r] = cur[r] - (int)p[(ptrdiff_t)r * stride];
        fwd16(tile, lane, res, coef);
        int sum = 0;
#pragma unroll
        for (int c = 0; c < 16; c++) sum += abs(coef[c]);
        sum = lanes_sum<16>(sum);
        if (valid && sum < best_cost) {
            best_cost = sum; best_rf = s; best_bx = bx; best_by = by; best_mvx = mvx; best_mvy = mvy;
#pragma unroll
            for (int c = 0; c < 16; c++) best[c] = coef[c];
        }
    }

    // ---- the decision (:643-655): inter iff its best cost is strictly below the open-loop intra cost
    int mode = DC_PRED;
    int64_t best_intra = INT64_MAX;
    if (A.use_ois) {
        mode = A.ois_mode[mb];
        if (mode >= N_MODES) mode = DC_PRED;
        best_intra = A.ois_cost[mb];
    }
    const bool inter = live && best_rf >= 0 && (int64_t)best_cost < best_intra;

    int64_t src_err = 1, src_rate = 0, rec_err = 1, rec_rate = 0;
    int eob = 0;
    if (__syncthreads_or(inter)) {
        // :658-673 the winning residual's quantisation error and rate
        int32_t dq[16];
        int e0;
        quant16(A.q, lane, best, dq, A.rate, e0, src_err, src_rate);
        // :675-700 the prediction is the block of the reference's RECONSTRUCTION at the same vector
        const uint8_t* p = curp; int stride = A.cur_stride;
        if (inter) {
            ref_of(best_rf, true, p, stride);
            p += (ptrdiff_t)best_by * stride + best_bx + lane;
        }
        int pred[16];
#pragma unroll
        for (int r = 0; r < 16; r++) pred[r] = p[(ptrdiff_t)r * stride];
        recon_pass(tile, lane, A, cur, pred, inter, A.recon + (ptrdiff_t)y * A.recon_stride + x + lane, A.recon_stride, eob, rec_err, rec_rate);
    }
    if (live && lane == 0) {
        SvtHipTplMbStats S = {};
        S.rf_idx = (int8_t)best_rf;
        S.mv_row = (int16_t)best_mvy; S.mv_col = (int16_t)best_mvx;
        S.is_inter = inter;
        S.mode = (uint8_t)mode;
        if (inter) {   // :673, :787-794, result_model_store: (v << 4) / 16, at least 1
            const int64_t srcrf_dist = src_err << 4, srcrf_rate = src_rate << 4;
            const int64_t recrf_dist = max(srcrf_dist, rec_err << 4), recrf_rate = max(srcrf_rate, rec_rate << 4);
            S.srcrf_dist = max((int64_t)1, srcrf_dist / 16); S.recrf_dist = max((int64_t)1, recrf_dist / 16);
            S.srcrf_rate = max((int64_t)1, srcrf_rate / 16); S.recrf_rate = max((int64_t)1, recrf_rate / 16);
            S.eob = (uint16_t)eob;
        }
        A.stats[mb] = S;
        A.decision[mb] = inter ? TPL_INTER : (uint8_t)mode;
    }
}

// ================================================================================================ phase B, one step
// The intra macroblocks among (d - 2y, y), y = y_lo .. y_lo + n - 1.
__global__ __launch_bounds__(TPL_ROWS_B * 16) void tpl_intra_step_kernel(const TplArgs A, int d, int y_lo, int n) {
    __shared__ int32_t tiles[TPL_ROWS_B * TPL_TILE];
    __shared__ uint8_t raw[TPL_ROWS_B * 2 * TPL_EDGE], flt[TPL_ROWS_B * 2 * TPL_EDGE];
    const int row = threadIdx.x >> 4, lane = threadIdx.x & 15;
    int32_t* tile = tiles + row * TPL_TILE;
    const int k = blockIdx.x * TPL_ROWS_B + row;
    const int my = y_lo + k, mx = d - 2 * my;
    const bool inside = k < n && mx >= 0 && mx < A.mb_cols && my < A.mb_rows;
    const int mb = inside ? my * A.mb_cols + mx : 0;
    const int dec = inside ? (int)A.decision[mb] : (int)TPL_INTER;
    const bool live = dec != TPL_INTER;
    if (!__syncthreads_or(live)) return;
    const int x = live ? mx * 16 : 0, y = live ? my * 16 : 0;   // a row without work: macroblock (0, 0) reads no neighbour
    const int mode = live && dec < N_MODES ? dec : DC_PRED;

    // ---- neighbours from this picture's reconstruction (update_neighbor_samples_array_open_loop_mb_recon)
    uint8_t* ra = raw + (row * 2) * TPL_EDGE + 16;
    uint8_t* rl = ra + TPL_EDGE;
    uint8_t* fa = flt + (row * 2) * TPL_EDGE + 16;
    uint8_t* fl = fa + TPL_EDGE;
    for (int i = lane; i < 66; i += 16) {
        const int which = i >= 33, idx = i - which * 33 - 1;
        (which ? rl : ra)[idx] = (uint8_t)ois_neighbor(A.recon, A.recon_stride, A.w, A.h, x, y, which, idx);
    }
    __syncthreads();
    // ---- filter_intra_edge as in intra_ois_kernel: corner filter when both edges are read, edge filters over the available run, never for V / H
    const int p_angle = mode >= V_PRED && mode <= D67_PRED ? kModeAngle[mode] : 0;
    const bool dirf = mode >= D45_PRED && mode <= D67_PRED;
    const bool need_a = dirf && p_angle < 180, need_l = dirf && p_angle > 90;
    if (dirf) {
        const bool corner = need_a && need_l;
        const int cv = corner ? corner_filter(ra, rl) : 0;
        const int str_a = y > 0 ? ois_strength(p_angle - 90) : 0, npx_a = 17 + (p_angle < 90 ? 16 : 0);
        const int str_l = x > 0 ? ois_strength(p_angle - 180) : 0, npx_l = 17 + (p_angle > 180 ? 16 : 0);
        auto pa = [&](int kk) -> int { return kk == 0 && corner ? cv : (int)ra[kk - 1]; };
        auto pl = [&](int kk) -> int { return kk == 0 && corner ? cv : (int)rl[kk - 1]; };
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int kk = lane + 16 * j;
            if (j < 2 || lane == 0) {
                if (need_a) fa[kk - 1] = (uint8_t)edge_filter_at(pa, npx_a, str_a, kk);
                if (need_l) fl[kk - 1] = (uint8_t)edge_filter_at(pl, npx_l, str_l, kk);
            }
        }
    }
    int sa = ra[lane], sl = rl[lane];
    sa = lanes_sum<16>(sa); sl = lanes_sum<16>(sl);
    __syncthreads();
    const uint8_t* a = need_a ? fa : ra;
    const uint8_t* l = need_l ? fl : rl;
    PredParams P;
    P.mode = mode; P.bw = 16; P.bh = 16; P.up_above = 0; P.up_left = 0; P.bd = 8;
    P.dc = dc_value(sa, sl, 16, 16, x > 0, y > 0, 8);
    set_angle(P, p_angle);
    int pred[16], cur[16];
    const uint8_t* curp = A.cur + (ptrdiff_t)y * A.cur_stride + x + lane;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        pred[r] = predict_sample(P, a, l, r, lane);
        cur[r] = curp[(ptrdiff_t)r * A.cur_stride];
    }
    int eob;
    int64_t err, rate;
    recon_pass(tile, lane, A, cur, pred, live, A.recon + (ptrdiff_t)y * A.recon_stride + x + lane, A.recon_stride, eob, err, rate);
    if (live && lane == 0) {   // :789-794: both pairs are the reconstruction pass's
        SvtHipTplMbStats* S = A.stats + mb;
        S->srcrf_dist = S->recrf_dist = max((int64_t)1, (err << 4) / 16);
        S->srcrf_rate = S->recrf_rate = max((int64_t)1, (rate << 4) / 16);
        S->eob = (uint16_t)eob;
    }
}

}  // namespace

extern "C" int svt_hip_launch_tpl_dispenser(hipStream_t st, const SvtHipTplParams* p, const uint8_t* cur, int cur_stride, const SvtHipTplRef* refs, const uint32_t* mv,
                                            const uint8_t* ref_mask, const uint8_t* ois_mode, const int32_t* ois_cost, uint8_t* recon, int recon_stride,
                                            SvtHipTplMbStats* stats, uint8_t* decision, int phases) {
    TplArgs A = {};
    A.w = p->w; A.h = p->h; A.pad = p->pad; A.mb_cols = (p->w + 15) / 16; A.mb_rows = (p->h + 15) / 16;
    A.use_ois = p->use_ois != 0; A.add_residual = p->add_residual != 0; A.rate = p->rate != 0; A.best_ref_only = p->best_ref_only != 0;
    A.q = p->q;
    for (int r = 0; r < 7; r++) {
        A.refs[r] = refs[r];
        if (refs[r].d_src) A.present |= 1u << r;
    }
    A.cur = cur; A.cur_stride = cur_stride; A.mv = mv; A.mask = ref_mask; A.ois_mode = ois_mode; A.ois_cost = ois_cost;
    A.recon = recon; A.recon_stride = recon_stride; A.stats = stats; A.decision = decision;
    const int n_mb = A.mb_cols * A.mb_rows;
    if (n_mb <= 0) return 0;
    if (phases & 1) hipLaunchKernelGGL(tpl_inter_kernel, dim3((n_mb + TPL_ROWS_A - 1) / TPL_ROWS_A), dim3(TPL_ROWS_A * 16), 0, st, A);
    const int steps = A.mb_cols + 2 * A.mb_rows - 2;
    for (int d = 0; d < steps && (phases & 2); d++) {
        const int y_lo = d > A.mb_cols - 1 ? (d - (A.mb_cols - 1) + 1) / 2 : 0, y_hi = min(A.mb_rows - 1, d / 2);
        const int n = y_hi - y_lo + 1;
        if (n <= 0) continue;
        hipLaunchKernelGGL(tpl_intra_step_kernel, dim3((n + TPL_ROWS_B - 1) / TPL_ROWS_B), dim3(TPL_ROWS_B * 16), 0, st, A, d, y_lo, n);
    }
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(tpl)
