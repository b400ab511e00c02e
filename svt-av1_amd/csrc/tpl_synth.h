// tpl_synth.h — the arithmetic of the TPL flow synthesizer and of generate_r0beta, written once for the device (tpl_synth.hip) and for a host compiler
// (svt_hip_tpl_window_host in svt_hip_host.cpp, tests/tpl_synth_host_test.cpp).  Plain C++17, no HIP.  File:line under Source/Lib of the reference:
//   Encoder/Codec/EbRateControlProcess.c:887-998    tpl_mc_flow_synthesizer -> tpl_model_update -> tpl_model_update_b, :818-855 get_overlap_area, round_floor
//   Encoder/Codec/EbRateControlProcess.c:1000-1075  generate_r0beta, :39-84 generate_lambda_scaling_factor
//   Encoder/Codec/EbRateDistortionCost.h:104-107    RDCOST (RDDIV_BITS 7, AV1_PROB_COST_SHIFT 9)
//   Common/Codec/EbBlockStructures.h:41-60          GET_MV_RAWPEL, get_fullmv_from_mv
// The accumulators are int64_t and every add is an integer computed from the scattering block alone, so the device adds them with 64-bit atomics in any
// order.  The doubles are IEEE + * / and conversions in the reference's order; both builds use -ffp-contract=off and results are compared by bit pattern.
// Sums the reference forms in int64_t are formed in uint64_t here (the same bits, no undefined overflow).  docs/kernels/tpl.md.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/svt_hip.h"

#if defined(__HIPCC__)
#define TPL_HD __host__ __device__ inline
#else
#define TPL_HD inline
#endif

namespace tplsyn {

constexpr int RDDIV_BITS = 7, PROB_COST_SHIFT = 9;

// The grid of one picture.  mi_rows * 4 = h and mi_cols * 4 = w (both multiples of 8: the aligned picture is the picture); mi_cols_sr * 4 = mb_cols * 16.
struct Geom {
    int w, h, cell_log2, s;   // s = 4 - cell_log2: a macroblock is (1 << s) x (1 << s) cells
    int mb_cols, mb_rows;
    int cols, rows;           // the grid, in cells: cols is the reference's mi_cols_sr >> shift stride
};
TPL_HD Geom geom(int w, int h, int cell_log2) {
    Geom g;
    g.w = w; g.h = h; g.cell_log2 = cell_log2; g.s = 4 - cell_log2;
    g.mb_cols = (w + 15) / 16; g.mb_rows = (h + 15) / 16;
    g.cols = g.mb_cols << g.s; g.rows = g.mb_rows << g.s;
    return g;
}
TPL_HD bool size_ok(int w, int h) { return w >= 16 && h >= 16 && !(w & 7) && !(h & 7) && w <= 65536 && h <= 65536; }
TPL_HD bool params_ok(const SvtHipTplSynthParams* p) {
    return p && size_ok(p->w, p->h) && (p->cell_log2 == 3 || p->cell_log2 == 4) && (p->sb_size == 64 || p->sb_size == 128) && p->base_rdmult >= 0;
}
// 0 = fine, 1 = a pointer is missing or an index is out of range, 2 = a self-reference in entries 1..7
inline int frames_check(const SvtHipTplWindowFrame* f, int n) {
    if (!f || n < 1 || n > SVT_HIP_TPL_MAX_WINDOW) return 1;
    for (int i = 0; i < n; i++) {
        if (!f[i].d_dep || ((f[i].on || i == 0) && !f[i].d_stats)) return 1;   // picture 0's records feed generate_r0beta whether it is on or not
        for (int j = 0; j < i; j++)
            if (f[j].d_dep == f[i].d_dep) return 1;
        for (int k = 0; k < 8; k++) {
            if (f[i].ref_window[k] < -1 || f[i].ref_window[k] >= n) return 1;
            if (k && f[i].ref_window[k] == i) return 2;
        }
    }
    return 0;
}

TPL_HD int mv_rawpel(int x) { return (x + 3 + (x >= 0)) >> 3; }   // GET_MV_RAWPEL: eighth samples to whole samples
TPL_HD int round_floor(int ref_pos, int bsize_pix) {              // :847-855
    return ref_pos < 0 ? -(1 + (-ref_pos - 1) / bsize_pix) : ref_pos / bsize_pix;
}
// (int64_t)v as the project defines it where C does not: NaN -> 0, outside int64_t -> INT64_MIN
TPL_HD int64_t trunc_i64(double v) {
    if (!(v == v)) return 0;
    if (!(v < 9223372036854775808.0) || v < -9223372036854775808.0) return INT64_MIN;
    return (int64_t)v;
}
// v / (1 << log2) of C: towards zero
TPL_HD int64_t div_trunc_pow2(int64_t v, int log2) { return (int64_t)((uint64_t)v + (uint64_t)((v >> 63) & (((int64_t)1 << log2) - 1))) >> log2; }
TPL_HD int64_t rdcost(int32_t rm, int64_t rate, int64_t dist) {   // RDCOST(RM, R, D): the rate term is formed and shifted as uint64_t
    return (int64_t)((((uint64_t)rate * (uint64_t)(int64_t)rm + (uint64_t)((1 << PROB_COST_SHIFT) >> 1)) >> PROB_COST_SHIFT) + (uint64_t)dist * (uint64_t)(1 << RDDIV_BITS));
}

// ------------------------------------------------------------------------------------------------ the scatter of one source block
struct Block {
    int slot;                 // index into ref_window: rf_idx + 1, or -1 = no target
    int ref_row, ref_col;     // the moved block's top-left, in samples
    int grid_row, grid_col;   // top-left of the first of the four grid blocks it overlaps
    int64_t dist, rate;       // cur_dep_dist + mc_dep_dist', delta_rate + mc_dep_rate'
};
// tpl_model_update_b :893-921 for the block whose cell is (cell_row, cell_col) of its own picture; own_rate / own_dist are that cell's accumulators.
TPL_HD Block block_of(const Geom& g, const SvtHipTplMbStats& r, int64_t own_rate, int64_t own_dist, int cell_row, int cell_col) {
    (void)own_rate;   // delta_rate_cost's argument: the branch is not built (mc_dep_rate' = 0, the reference's tpl_opt_flag)
    Block b;
    const bool has_ref = r.rf_idx != -1;   // :795-798; without a reference ref_frame_poc and mv keep the memset's zeros (:579)
    b.slot = r.rf_idx >= -1 && r.rf_idx <= 6 ? r.rf_idx + 1 : -1;
    const int bs = 1 << g.cell_log2;
    b.ref_row = cell_row * bs + (has_ref ? (int16_t)mv_rawpel(r.mv_row) : 0);
    b.ref_col = cell_col * bs + (has_ref ? (int16_t)mv_rawpel(r.mv_col) : 0);
    b.grid_row = round_floor(b.ref_row, bs) * bs;
    b.grid_col = round_floor(b.ref_col, bs) * bs;
    const int64_t cur_dep_dist = (int64_t)((uint64_t)r.recrf_dist - (uint64_t)r.srcrf_dist);
    const int64_t mc_dep_dist = r.recrf_dist ? trunc_i64((double)own_dist * ((double)cur_dep_dist / (double)r.recrf_dist)) : 0;   // :911-914
    b.dist = (int64_t)((uint64_t)cur_dep_dist + (uint64_t)mc_dep_dist);
    b.rate = (int64_t)((uint64_t)r.recrf_rate - (uint64_t)r.srcrf_rate);   // :915-916, mc_dep_rate' = 0
    return b;
}
// Grid block k = 0..3 of the moved block (:923-948): false = not accepted.  Else the target cell's index and the two addends (either may be 0).
TPL_HD bool target_of(const Geom& g, const Block& b, int k, int* cell, int64_t* add_rate, int64_t* add_dist) {
    const int bs = 1 << g.cell_log2;
    const int row = b.grid_row + bs * (k >> 1), col = b.grid_col + bs * (k & 1);
    if (!(row >= 0 && row < g.h && col >= 0 && col < g.w)) return false;   // mi_rows * MI_SIZE, mi_cols * MI_SIZE: the aligned picture, not the mi_cols_sr grid
    // get_overlap_area :818-845
    const int width = (k & 1) ? b.ref_col + bs - col : col + bs - b.ref_col;
    const int height = (k >> 1) ? b.ref_row + bs - row : row + bs - b.ref_row;
    const uint64_t area = (uint64_t)(int64_t)(width * height);
    *cell = (row >> g.cell_log2) * g.cols + (col >> g.cell_log2);
    *add_dist = div_trunc_pow2((int64_t)((uint64_t)b.dist * area), 2 * g.cell_log2);   // :940-944, pix_num = 256 or 64
    *add_rate = div_trunc_pow2((int64_t)((uint64_t)b.rate * area), 2 * g.cell_log2);
    return true;
}

// ------------------------------------------------------------------------------------------------ generate_r0beta
// dep = the picture's grid, stats = its records; a cell's recrf_dist is its macroblock's.
TPL_HD int64_t cell_recrf(const Geom& g, const SvtHipTplMbStats* stats, int row, int col) { return stats[(row >> g.s) * g.mb_cols + (col >> g.s)].recrf_dist; }
TPL_HD int64_t cell_intra(int64_t recrf_dist) { return (int64_t)((uint64_t)recrf_dist << RDDIV_BITS); }
TPL_HD int64_t cell_delta(const Geom& g, int32_t rm, const int64_t* dep, int row, int col) {
    const int64_t* c = dep + 2 * ((size_t)row * g.cols + col);
    return rdcost(rm, c[0], c[1]);
}
// the base sums run over row < mi_rows, col < mi_cols_sr (:1009-1010): every grid column, but not the cell row past the aligned height
TPL_HD bool base_has_row(const Geom& g, int row) { return (row << g.cell_log2) < g.h; }
TPL_HD double r0_of(double r0_in, int64_t intra_cost_base, int64_t mc_dep_cost_base) {   // :1020-1022
    return mc_dep_cost_base != 0 ? (double)intra_cost_base / (double)mc_dep_cost_base : r0_in;
}
// tpl_rdmult_scaling_factors[mb_row * mb_cols + mb_col] (:53-80): double sums of one or four terms, mi_row outer, mi_col inner, `continue` past mi_rows
TPL_HD double factor_of(const Geom& g, int32_t rm, const SvtHipTplMbStats* stats, const int64_t* dep, int mb_row, int mb_col, int64_t mc_dep_cost_base, double r0) {
    double intra_cost = 0.0, mc_dep_cost = 0.0;
    const int n = 1 << g.s;
    for (int j = 0; j < n; j++)
        for (int i = 0; i < n; i++) {
            const int row = (mb_row << g.s) + j, col = (mb_col << g.s) + i;
            if (!base_has_row(g, row)) continue;   // mi_col >= mi_cols_sr never holds
            const int64_t intra = cell_intra(cell_recrf(g, stats, row, col));
            intra_cost += (double)intra;
            mc_dep_cost += (double)intra + (double)cell_delta(g, rm, dep, row, col);
        }
    double rk = 0;
    if (mc_dep_cost > 0 && intra_cost > 0) rk = intra_cost / mc_dep_cost;
    return mc_dep_cost_base ? rk / r0 + 1.2 : 1.2;
}
// tpl_beta[sb_row * sb_cols + sb_col] (:1043-1072): int64 sums over the superblock's cells whose macroblock exists
TPL_HD double beta_of(const Geom& g, int sb_size, int32_t rm, const SvtHipTplMbStats* stats, const int64_t* dep, int sb_row, int sb_col, double r0) {
    uint64_t intra_cost = 0, mc_dep_cost = 0;
    const int blks = sb_size >> g.cell_log2;
    for (int j = 0; j < blks; j++)
        for (int i = 0; i < blks; i++) {
            const int col = ((sb_col * sb_size) >> g.cell_log2) + i, row = ((sb_row * sb_size) >> g.cell_log2) + j;
            if ((col >> g.s) >= g.mb_cols || (row >> g.s) >= g.mb_rows) continue;
            const int64_t intra = cell_intra(cell_recrf(g, stats, row, col));
            intra_cost += (uint64_t)intra;
            mc_dep_cost += (uint64_t)intra + (uint64_t)cell_delta(g, rm, dep, row, col);
        }
    double beta = 1.0;
    if ((int64_t)mc_dep_cost > 0 && (int64_t)intra_cost > 0) {
        const double rk = (double)(int64_t)intra_cost / (double)(int64_t)mc_dep_cost;
        beta = r0 / rk;
    }
    return beta;
}
TPL_HD size_t dep_cells(const Geom& g) { return (size_t)g.rows * g.cols; }
TPL_HD int sb_count(int v, int sb_size) { return (v + sb_size - 1) / sb_size; }
TPL_HD size_t out_bytes(int w, int h, int sb_size) {
    return sizeof(SvtHipTplR0BetaHeader) + sizeof(double) * ((size_t)((w + 15) / 16) * ((h + 15) / 16) + (size_t)sb_count(w, sb_size) * sb_count(h, sb_size));
}

// ------------------------------------------------------------------------------------------------ the serial form (host)
// tpl_mc_flow_synthesizer(pcs_array, idx, n) in the reference's block order
inline void synth_picture_host(const Geom& g, const SvtHipTplWindowFrame* frames, int idx) {
    const SvtHipTplWindowFrame& f = frames[idx];
    for (int row = 0; row < g.rows; row++)
        for (int col = 0; col < g.cols; col++) {
            const int64_t* own = f.d_dep + 2 * ((size_t)row * g.cols + col);
            const Block b = block_of(g, f.d_stats[(row >> g.s) * g.mb_cols + (col >> g.s)], own[0], own[1], row, col);
            const int t = b.slot < 0 ? -1 : f.ref_window[b.slot];
            if (t < 0) continue;
            for (int k = 0; k < 4; k++) {
                int cell;
                int64_t add_rate, add_dist;
                if (!target_of(g, b, k, &cell, &add_rate, &add_dist)) continue;
                int64_t* c = frames[t].d_dep + 2 * (size_t)cell;
                c[0] = (int64_t)((uint64_t)c[0] + (uint64_t)add_rate);
                c[1] = (int64_t)((uint64_t)c[1] + (uint64_t)add_dist);
            }
        }
}
inline void r0beta_host(const SvtHipTplSynthParams& p, const SvtHipTplMbStats* stats, const int64_t* dep, void* out) {
    const Geom g = geom(p.w, p.h, p.cell_log2);
    uint64_t intra_base = 0, mc_base = 0;
    for (int row = 0; row < g.rows; row++) {
        if (!base_has_row(g, row)) continue;
        for (int col = 0; col < g.cols; col++) {
            const int64_t intra = cell_intra(cell_recrf(g, stats, row, col));
            intra_base += (uint64_t)intra;
            mc_base += (uint64_t)intra + (uint64_t)cell_delta(g, p.base_rdmult, dep, row, col);
        }
    }
    SvtHipTplR0BetaHeader* hd = (SvtHipTplR0BetaHeader*)out;
    hd->intra_cost_base = (int64_t)intra_base; hd->mc_dep_cost_base = (int64_t)mc_base;
    hd->r0 = r0_of(p.r0_in, hd->intra_cost_base, hd->mc_dep_cost_base);
    double* factors = (double*)(hd + 1);
    for (int r = 0; r < g.mb_rows; r++)
        for (int c = 0; c < g.mb_cols; c++) factors[r * g.mb_cols + c] = factor_of(g, p.base_rdmult, stats, dep, r, c, hd->mc_dep_cost_base, hd->r0);
    double* beta = factors + (size_t)g.mb_rows * g.mb_cols;
    const int sbc = sb_count(p.w, p.sb_size), sbr = sb_count(p.h, p.sb_size);
    for (int r = 0; r < sbr; r++)
        for (int c = 0; c < sbc; c++) beta[r * sbc + c] = beta_of(g, p.sb_size, p.base_rdmult, stats, dep, r, c, hd->r0);
}
// tpl_mc_flow :1154-1197 after the dispensers; the arguments were checked by the caller
inline void window_host(const SvtHipTplSynthParams& p, const SvtHipTplWindowFrame* frames, int n, void* out) {
    const Geom g = geom(p.w, p.h, p.cell_log2);
    for (int i = 0; i < n; i++)
        for (size_t k = 0; k < 2 * dep_cells(g); k++) frames[i].d_dep[k] = 0;
    for (int i = n - 1; i >= 0; i--)
        if (frames[i].on) synth_picture_host(g, frames, i);
    r0beta_host(p, frames[0].d_stats, frames[0].d_dep, out);
}

}  // namespace tplsyn
