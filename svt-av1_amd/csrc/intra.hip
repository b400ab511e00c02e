// intra.hip — AV1 intra prediction on gfx950 (wave64): the batch form of the luma predictors and the picture-level open-loop intra search.
//
// Replaces (file:line under Source/Lib of the reference):
//   Encoder/Codec/EbMotionEstimation.c:3043-3155     open_loop_intra_search_mb, for every 16x16 macroblock of a picture in one launch
//   Encoder/Codec/EbEncIntraPrediction.c:1201-1280   update_neighbor_samples_array_open_loop_mb (neighbours taken from the source picture)
//   Common/Codec/EbIntraPrediction.c:2545-2632       filter_intra_edge, intra_prediction_open_loop_mb
//   Encoder/Codec/EbTransforms.c:3827-3838           svt_av1_wht_fwd_txfm (= svt_av1_fwd_txfm2d_16x16, DCT_DCT) + svt_aom_satd
//   Common/Codec/EbIntraPrediction.c:246-345, 863-968, 2260-2440 and the svt_aom_[highbd_]*_predictor_WxH_c family (batch form)
//
// Search kernel mapping: a 16-lane row = one (macroblock, mode) pair, lane = column.  Each lane predicts its 16-sample column from edges in LDS,
// subtracts the source column, runs the column DCT in registers (txfm_1d.h), the 16 lanes meet through a padded 16 x 17 dword LDS tile, each lane
// then runs one row DCT, sums |coefficient|, and the 16 partial sums are reduced inside the row.  A workgroup owns MB macroblocks x all modes and is
// laid out mode-major (slot = mode * MB + macroblock, MB a multiple of 4), so the four rows of a wave share one mode: the mode switch is a scalar
// branch and no lane idles.  The winner of a macroblock is the minimum of (cost << 4 | mode) over its slots: the first mode in mode order wins ties.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "txfm_1d.h"
#include "intra_dev.h"

namespace {

using namespace intra;

// ================================================================================================ picture-level open-loop intra search
// 16x16 DCT_DCT forward configuration (Encoder/Codec/EbTransforms.h:28 fwd_shift_16x16 = {2, -2, 0}; :46-57 fwd_cos_bit_col[2][2] = 13,
// fwd_cos_bit_row[2][2] = 12) -- the values txfm2d.hip's fwd_shift_of / fwd_cos_col_of / fwd_cos_row_of give for W = H = 16.
constexpr int OIS_S0 = 2, OIS_S1 = 2, OIS_CBC = 13, OIS_CBR = 12;
constexpr int OIS_TILE = 16 * 17;   // dwords per slot: row stride 17 keeps both the column-wise store and the row-wise load conflict free
constexpr int OIS_EDGE = 48;        // bytes per edge: sample i at [16 + i], i = -1 .. 31

template <int MB>
__global__ __launch_bounds__(MB == 4 ? 832 : (MB == 8 ? 384 : 256)) void intra_ois_kernel(const uint8_t* __restrict__ src, int stride, int w, int h, int nmodes,
                                                                                           int mb_cols, uint8_t* __restrict__ out_mode,
                                                                                           int32_t* __restrict__ out_cost) {
    extern __shared__ int32_t smem[];
    const int S = MB * nmodes;   // slots of this workgroup == blockDim.x / 16
    int32_t* tile = smem;                       // [S][16 x 17]
    uint32_t* keys = (uint32_t*)(smem + S * OIS_TILE);   // [S]
    uint8_t* srcblk = (uint8_t*)(keys + S);     // [MB][16 x 16]
    uint8_t* raw = srcblk + MB * 256;           // [MB][2][OIS_EDGE] unfiltered edges
    uint8_t* flt = raw + MB * 2 * OIS_EDGE;     // [S][2][OIS_EDGE] the edges as this slot's mode sees them
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int mbx0 = blockIdx.x * MB, y = blockIdx.y * 16;   // a workgroup's macroblocks are neighbours in one macroblock row

    // ---- the macroblocks and their neighbours, fetched once for all modes
    for (int i = tid; i < MB * 256; i += nthr) {
        const int mx = mbx0 + (i >> 8);
        if (mx < mb_cols) srcblk[i] = src[(size_t)(y + ((i >> 4) & 15)) * stride + mx * 16 + (i & 15)];
    }
    for (int i = tid; i < MB * 66; i += nthr) {
        const int m = i / 66, e = i - m * 66, which = e >= 33, idx = e - which * 33 - 1;
        if (mbx0 + m < mb_cols) raw[(m * 2 + which) * OIS_EDGE + 16 + idx] = (uint8_t)ois_neighbor(src, stride, w, h, (mbx0 + m) * 16, y, which, idx);
    }
    __syncthreads();

    const int slot = tid >> 4, lane = tid & 15;
    const int mode = __builtin_amdgcn_readfirstlane(slot / MB);   // uniform over the wave: 4 consecutive slots, MB % 4 == 0
    const int m = slot % MB;
    const bool live = mbx0 + m < mb_cols;   // a dead slot computes on whatever LDS holds (no index depends on data) and stores nothing
    const int x = live ? (mbx0 + m) * 16 : 0;
    const uint8_t* ra = raw + (m * 2) * OIS_EDGE + 16;
    const uint8_t* rl = ra + OIS_EDGE;
    uint8_t* fa = flt + (slot * 2) * OIS_EDGE + 16;
    uint8_t* fl = fa + OIS_EDGE;

    // ---- filter_intra_edge on this slot's copy of the edges a directional mode reads: corner filter when both are needed, edge filters over the available
    // run; never for V / H, and no up-sampling at 16 + 16.  Samples k = 0 .. 32 of a run (k = 0 is the corner): lane l conditions k = l, l + 16 and lane 0
    // also k = 32.  Every other mode, and the edge a zone-1 / zone-3 mode does not read, stays on the macroblock's unfiltered edges.
    const int p_angle = __builtin_amdgcn_readfirstlane(mode >= V_PRED && mode <= D67_PRED ? kModeAngle[mode] : 0);
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
    const uint8_t* a = need_a ? fa : ra;
    const uint8_t* l = need_l ? fl : rl;
    int dc = 0;
    if (mode == DC_PRED) {   // dc_pred[x > 0][y > 0][TX_16X16]
        int sa = ra[lane], sl = rl[lane];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) { sa += __shfl_xor(sa, o, 64); sl += __shfl_xor(sl, o, 64); }
        dc = dc_value(sa, sl, 16, 16, x > 0, y > 0, 8);
    }
    __syncthreads();

    // ---- lane = column: predict, subtract, column DCT (fwd_block of txfm2d.hip, W = H = 16, DCT_DCT).  The mode is a scalar: one switch, the 16 rows inside.
    {
        int32_t in[16], out[16];
        const uint8_t* s = srcblk + m * 256 + lane;
        auto column = [&](auto pred) {
#pragma unroll
            for (int r = 0; r < 16; r++) in[r] = (int32_t)s[r * 16] - pred(r);
        };
        const int c = lane;
        switch (mode) {
        case DC_PRED: column([&](int) { return dc; }); break;
        case V_PRED: { const int v = a[c]; column([&](int) { return v; }); break; }
        case H_PRED: column([&](int r) { return (int)l[r]; }); break;
        case SMOOTH_PRED: column([&](int r) { return pred_smooth(a, l, r, c, 16, 16); }); break;
        case SMOOTH_V_PRED: column([&](int r) { return pred_smooth_v(a, l, r, c, 16); }); break;
        case SMOOTH_H_PRED: column([&](int r) { return pred_smooth_h(a, l, r, c, 16); }); break;
        case PAETH_PRED: column([&](int r) { return pred_paeth(a, l, r, c); }); break;
        case D45_PRED:
        case D67_PRED: { const int dx = __builtin_amdgcn_readfirstlane(dr_derivative(p_angle)); column([&](int r) { return pred_z1(a, r, c, 16, 16, dx, 0, 8); }); break; }
        case D203_PRED: { const int dy = __builtin_amdgcn_readfirstlane(dr_derivative(270 - p_angle)); column([&](int r) { return pred_z1(l, c, r, 16, 16, dy, 0, 8); }); break; }
        default: {   // D135, D113, D157
            const int dx = __builtin_amdgcn_readfirstlane(dr_derivative(180 - p_angle)), dy = __builtin_amdgcn_readfirstlane(dr_derivative(p_angle - 90));
            column([&](int r) { return pred_z2(a, l, r, c, dx, dy, 0, 0, 8); });
            break;
        }
        }
        // A residual is within +-255: the 16-bit sign extension is exact, and it tells the compiler (which loses the range where the mode branches join) that
        // the operands of the transform's multiplies fit 24 bits: full-rate v_mul_i32_i24 instead of quarter-rate v_mul_lo_u32.  Same for the row pass below.
#pragma unroll
        for (int r = 0; r < 16; r++) in[r] = (int32_t)(int16_t)in[r] * (1 << OIS_S0);
        tx1d::fwd_dct<16, OIS_CBC>(in, out);
#pragma unroll
        for (int r = 0; r < 16; r++) tile[slot * OIS_TILE + r * 17 + lane] = tx1d::rshift_round(out[r], OIS_S1);
    }
    __syncthreads();
    // ---- lane = row: row DCT, sum of absolute coefficients (svt_aom_satd), reduced over the 16 rows
    {
        int32_t in[16], out[16];
#pragma unroll
        // the column pass leaves at most 16 * 1020 / 4 in magnitude: reading the low half sign-extended is exact
        for (int c = 0; c < 16; c++) in[c] = (int32_t)(int16_t)tile[slot * OIS_TILE + lane * 17 + c];
        tx1d::fwd_dct<16, OIS_CBR>(in, out);
        int32_t sum = 0;
#pragma unroll
        for (int c = 0; c < 16; c++) sum += abs(out[c]);
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o, 64);
        if (lane == 0) keys[slot] = ((uint32_t)sum << 4) | (uint32_t)mode;   // sum < 2^20 (see include/svt_hip.h)
    }
    __syncthreads();
    if (tid < MB && mbx0 + tid < mb_cols) {
        uint32_t best = keys[tid];
        for (int j = 1; j < nmodes; j++) best = min(best, keys[j * MB + tid]);
        const int k = blockIdx.y * mb_cols + mbx0 + tid;
        out_mode[k] = (uint8_t)(best & 15);
        out_cost[k] = (int32_t)(best >> 4);
    }
}

// ================================================================================================ batch form of the predictors
constexpr int EDGE_REC = 160, EDGE_ORG = 16;   // one edge of a record: MAX_TX_SIZE * 2 + 32 samples, sample 0 at element 16

template <typename PIX>
__global__ __launch_bounds__(256) void intra_predict_batch_kernel(const PIX* __restrict__ edges, const SvtHipIntraJob* __restrict__ jobs, int bd,
                                                                  PIX* __restrict__ dst, int dst_stride) {
    __shared__ uint16_t e0[2][EDGE_REC], e1[2][EDGE_REC], e2[2][EDGE_REC];
    __shared__ int sums[2];
    const SvtHipIntraJob J = jobs[blockIdx.x];
    // descriptors live in device memory: nothing indexes a table before this (workgroup-uniform) check
    if (J.tx_size >= N_TX_SIZES || J.mode >= N_MODES || J.angle_delta < -3 || J.angle_delta > 3) return;
    const int tid = threadIdx.x;
    const int bw = kTxW[J.tx_size], bh = kTxH[J.tx_size];
    const int start = J.start_m1 ? -1 : 0;
    const int npx[2] = {min((int)J.npx_above, 129), min((int)J.npx_left, 129)};
    const int str[2] = {min((int)J.strength_above, 3), min((int)J.strength_left, 3)};
    const int up[2] = {J.upsample_above != 0, J.upsample_left != 0};
    const int upn[2] = {min(max((int)J.up_npx_above, 1), 16), min(max((int)J.up_npx_left, 1), 16)};

    for (int i = tid; i < 2 * EDGE_REC; i += 256) e0[i / EDGE_REC][i % EDGE_REC] = edges[(size_t)J.edge_off + i];
    __syncthreads();
    // corner, then the edge filters: each output sample from the unfiltered record (the corner's new value substituted)
    const int cv = J.corner_filter ? corner_filter(&e0[0][EDGE_ORG], &e0[1][EDGE_ORG]) : 0;
    for (int i = tid; i < 2 * EDGE_REC; i += 256) {
        const int which = i / EDGE_REC, j = i % EDGE_REC, idx = j - EDGE_ORG;
        auto p = [&](int kk) -> int { const int t = start + kk; return t == -1 && J.corner_filter ? cv : (int)e0[which][EDGE_ORG + t]; };
        const int kk = idx - start;
        int v = idx == -1 && J.corner_filter ? cv : (int)e0[which][j];
        if (kk >= 1 && kk < npx[which]) v = edge_filter_at(p, npx[which], str[which], kk);
        e1[which][j] = (uint16_t)v;
    }
    __syncthreads();
    for (int i = tid; i < 2 * EDGE_REC; i += 256) {
        const int which = i / EDGE_REC, j = i % EDGE_REC, idx = j - EDGE_ORG;
        auto p = [&](int t) -> int { return e1[which][EDGE_ORG + t]; };
        e2[which][j] = (uint16_t)(up[which] && idx >= -2 && idx <= 2 * upn[which] - 2 ? edge_upsample_at(p, upn[which], idx, bd) : (int)e1[which][j]);
    }
    __syncthreads();
    const uint16_t* a = &e2[0][EDGE_ORG];
    const uint16_t* l = &e2[1][EDGE_ORG];
    PredParams P;
    P.mode = J.mode; P.bw = bw; P.bh = bh; P.up_above = up[0]; P.up_left = up[1]; P.bd = bd; P.dc = 0;
    set_angle(P, J.mode >= V_PRED && J.mode <= D67_PRED ? kModeAngle[J.mode] + 3 * J.angle_delta : 0);
    if (J.mode == DC_PRED) {
        if (tid < 2) {
            int s = 0;
            const int n = tid ? bh : bw;
            for (int i = 0; i < n; i++) s += e2[tid][EDGE_ORG + i];
            sums[tid] = s;
        }
        __syncthreads();
        P.dc = dc_value(sums[0], sums[1], bw, bh, J.dc_have & 1, (J.dc_have >> 1) & 1, bd);
    }
    PIX* d = dst + (size_t)J.dst_y * dst_stride + J.dst_x;
    for (int i = tid; i < bw * bh; i += 256) {
        const int r = i / bw, c = i - r * bw;
        d[(size_t)r * dst_stride + c] = (PIX)predict_sample(P, a, l, r, c);
    }
}

}  // namespace

extern "C" int svt_hip_launch_intra_ois(hipStream_t st, const uint8_t* src, int stride, int w, int h, int mode_end, uint8_t* mode, int32_t* cost) {
    const int mb_cols = (w + 15) / 16, mb_rows = (h + 15) / 16, nmodes = mode_end + 1;
    if (mb_cols <= 0 || mb_rows <= 0) return 0;
    // macroblocks per workgroup: a multiple of 4 (one mode per wave), as many as keep the workgroup within 13 waves and 64 KB of LDS
    const int mb = nmodes >= 4 ? 4 : (nmodes >= 2 ? 8 : 16), slots = mb * nmodes;
    const size_t lds = (size_t)slots * (OIS_TILE * 4 + 4 + 2 * OIS_EDGE) + (size_t)mb * (256 + 2 * OIS_EDGE);
    const dim3 grid((mb_cols + mb - 1) / mb, mb_rows), block(slots * 16);
    if (mb == 4) hipLaunchKernelGGL(intra_ois_kernel<4>, grid, block, lds, st, src, stride, w, h, nmodes, mb_cols, mode, cost);
    else if (mb == 8) hipLaunchKernelGGL(intra_ois_kernel<8>, grid, block, lds, st, src, stride, w, h, nmodes, mb_cols, mode, cost);
    else hipLaunchKernelGGL(intra_ois_kernel<16>, grid, block, lds, st, src, stride, w, h, nmodes, mb_cols, mode, cost);
    return (int)hipGetLastError();
}

extern "C" int svt_hip_launch_intra_predict(hipStream_t st, int pix_bytes, int bd, const void* edges, const SvtHipIntraJob* jobs, int njobs, void* dst,
                                            int dst_stride) {
    if (njobs <= 0) return 0;
    svt_for_pix(pix_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL(intra_predict_batch_kernel<PIX>, dim3(njobs), dim3(256), 0, st, (const PIX*)edges, jobs, bd, (PIX*)dst, dst_stride);
    });
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(intra)
