// ibc_search.h — the arithmetic of the intra-block-copy full-pel search (diamond, refinement, mesh, the three-way choice with the hash search and the caller's last
// check) that is the same on the host and on the device, written once: ibc_search.hip runs the walks with every lane of a wave in step and the sums taken across
// lanes, svt_hip_ibc_full_search_host in svt_hip_host.cpp and tests/ibc_search_host_test.cpp run them serially.  Plain C++17, no HIP.  It builds on ibc_hash.h:
// mv_err_cost, the variance (here with width * height for the 22 shapes), the tile rule, the serial hash search.  File:line under Source/Lib of the reference:
//   Encoder/Codec/av1me.c:284-290      mvsad_err_cost
//   Encoder/Codec/av1me.c:292-318      svt_av1_init3smotion_compensation: 11 steps of 8 sites, len = 1024 .. 1; up, down, left, right, then the four diagonals
//   Encoder/Codec/av1me.c:437-573      svt_av1_diamond_search_sad_c (NEW_DIAMOND_SEARCH is not defined: that branch is not here)
//   Encoder/Codec/av1me.c:578-643      full_pixel_diamond
//   Encoder/Codec/av1me.c:712-775      svt_av1_refining_search_sad
//   Encoder/Codec/av1me.c:346-435      exhuastive_mesh_search
//   Encoder/Codec/av1me.c:650-710      full_pixel_exhaustive
//   Encoder/Codec/av1me.c:1306-1411    svt_av1_full_pixel_search, case NSTEP and the hash tail
//   Encoder/Codec/EbModeDecision.c:4486-4490, :4523   the caller's `continue` on empty limits, av1_is_dv_valid of the final vector
//
// Three things are restated in one form only, and why that is the reference's result:
//  * all_in (av1me.c:486-519, :723-745) is a faster way to the per-point is_mv_in branch: it holds only when the four axis sites are strictly inside the limits, and
//    then the diagonals are too, so every site passes is_mv_in and both branches take the same sites in the same order.  The per-point form is the one here.
//  * `best_address == in_what` (:569) compares addresses.  A job whose limits could take the block outside the picture is refused, so two vectors inside the limits
//    differ by less than a row in their columns and equal addresses mean equal vectors.  Vectors are compared here.
//  * the two-stage acceptance (`sad < best`, then `sad + cost < best`): mvsad_err_cost is an unsigned value shifted right by 9, never negative, so the second test
//    implies the first and a scan keeps the FIRST STRICT MINIMUM of sad + cost in scan order, the clamped centre first.  That is what makes the mesh scan parallel:
//    every candidate gets (total, scan index) and the smallest pair wins, whatever order they were computed in.  tests/test_ibc_search_ref_cpu.py proves the equality
//    against the literal loop.  The diamond and the refinement keep the literal two tests: their scans are eight and four sites long.
// x->second_best_mv is written by all of these and read by nothing on the intra-block-copy path: it is not produced.  mv_check_bounds (EbModeDecision.c:4522) cannot
// fire on a vector inside limits that are a subset of the outer ones (the assert_release lines :4479-4482): it is left out.  docs/kernels/ibc_hash.md.
#pragma once
#include "ibc_hash.h"

namespace ibcs {

using Job = SvtHipIbcFullSearchJob;
using Result = SvtHipIbcFullSearchResult;

constexpr int MAX_MVSEARCH_STEPS = 11, MAX_FIRST_STEP = 1 << (MAX_MVSEARCH_STEPS - 1);
constexpr int MIN_RANGE = 7, MAX_RANGE = 256, MIN_INTERVAL = 1, MAX_MESH_STEP = 4, REFINE_RANGE = 8;
constexpr int LIMIT_REACH = 2047;     // whole samples from ref_mv >> 3: 8 * 2047 + 7 = 16383, the last index of a cost table
constexpr int MESH_STRIPS = 64;       // partial minima per job and mesh pass in d_scratch
constexpr int MAX_JOBS = 1 << 24;     // jobs of one call: MAX_JOBS * MESH_STRIPS workgroups is a grid's size

// site j of a diamond step, in units of the step's len: {-1,0} {1,0} {0,-1} {0,1} {-1,-1} {-1,1} {1,-1} {1,1} as (row, col); two bits a site, value + 1
constexpr uint32_t SITE_ROWS = 0u | 2u << 2 | 1u << 4 | 1u << 6 | 0u << 8 | 0u << 10 | 2u << 12 | 2u << 14;
constexpr uint32_t SITE_COLS = 1u | 1u << 2 | 0u << 4 | 2u << 6 | 0u << 8 | 2u << 10 | 0u << 12 | 2u << 14;
// the refinement's neighbours {-1,0} {0,-1} {0,1} {1,0}
constexpr uint32_t NEIGH_ROWS = 0u | 1u << 2 | 1u << 4 | 2u << 6;
constexpr uint32_t NEIGH_COLS = 1u | 0u << 2 | 2u << 4 | 1u << 6;
IBC_HD int unpack(uint32_t pack, int j) { return (int)((pack >> (2 * j)) & 3) - 1; }

IBC_HD int ilog2(int v) { int n = 0; while (v > 1) { v >>= 1; ++n; } return n; }
IBC_HD int iabs(int v) { return v < 0 ? -v : v; }
IBC_HD int imin(int a, int b) { return a < b ? a : b; }
IBC_HD int imax(int a, int b) { return a > b ? a : b; }
IBC_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the 22 block sizes of AV1: powers of two 4 .. 128, 1:1 and 1:2 at every size, 1:4 up to 64
IBC_HD bool shape_ok(int w, int h) {
    if (w < 4 || h < 4 || w > 128 || h > 128 || (w & (w - 1)) || (h & (h - 1))) return false;
    const int big = imax(w, h), small = imin(w, h);
    return big == small || big == 2 * small || (big == 4 * small && big <= 64);
}
IBC_HD bool limits_empty(const Job& j) { return j.col_max < j.col_min || j.row_max < j.row_min; }
// 0: to be searched; 1: empty limits; -1: a bad job.  have_tables: the call has a hash table
IBC_HD int job_status(const Job& j, int width, int height, bool have_tables) {
    if (!shape_ok(j.block_w, j.block_h) || j.x_pos < 0 || j.y_pos < 0 || j.x_pos > width - j.block_w || j.y_pos > height - j.block_h) return -1;
    if (j.step_param < 0 || j.step_param > MAX_MVSEARCH_STEPS - 1 || j.sad_per_bit < 0 || j.error_per_bit < 0 || j.ibc_shift < 0 || j.ibc_shift > 1) return -1;
    if (j.mib_size_log2 < 0 || j.mib_size_log2 > ibc::MAX_MIB_LOG2 || !ibc::tile_ok(j.mi_row_start) || !ibc::tile_ok(j.mi_row_end) || !ibc::tile_ok(j.mi_col_start) ||
        !ibc::tile_ok(j.mi_col_end))
        return -1;
    if (j.use_hash && !have_tables) return -1;
    if (limits_empty(j)) return 1;
    // no vector inside the limits takes the block outside the picture (64-bit: the limits are anything)
    if ((int64_t)j.x_pos + j.col_min < 0 || (int64_t)j.x_pos + j.col_max > width - j.block_w || (int64_t)j.y_pos + j.row_min < 0 ||
        (int64_t)j.y_pos + j.row_max > height - j.block_h)
        return -1;
    const int fr = j.ref_mv_row >> 3, fc = j.ref_mv_col >> 3;
    if ((int64_t)j.row_min - fr < -LIMIT_REACH || (int64_t)j.row_max - fr > LIMIT_REACH || (int64_t)j.col_min - fc < -LIMIT_REACH || (int64_t)j.col_max - fc > LIMIT_REACH)
        return -1;
    return 0;
}
IBC_HD bool mv_in(const Job& j, int row, int col) { return col >= j.col_min && col <= j.col_max && row >= j.row_min && row <= j.row_max; }

// mvsad_err_cost of the whole-sample vector (row, col) against ref_mv >> 3: the difference times 8, an unsigned product, rounded by AV1_PROB_COST_SHIFT
IBC_HD uint32_t mvsad_err_cost(const Job& j, int row, int col, const int32_t* joint_cost, const int32_t* comp_cost) {
    const int     d_row = (row - (j.ref_mv_row >> 3)) * 8, d_col = (col - (j.ref_mv_col >> 3)) * 8;
    const int     joint = d_row == 0 ? (d_col == 0 ? 0 : 1) : (d_col == 0 ? 2 : 3);
    const int32_t cost = joint_cost[joint] + comp_cost[ibc::MV_MAX + d_row] + comp_cost[SVT_HIP_IBC_MV_VALS + ibc::MV_MAX + d_col];
    return ((uint32_t)cost * (uint32_t)j.sad_per_bit + 256u) >> 9;
}
// the cost svt_av1_get_mvpred_var adds: mv_err_cost of 8 * (row, col) against ref_mv
IBC_HD int mvpred_cost(const Job& j, int row, int col, const int32_t* joint_cost, const int32_t* comp_cost) {
    return ibc::mv_err_cost(row * 8 - j.ref_mv_row, col * 8 - j.ref_mv_col, joint_cost, comp_cost, j.error_per_bit);
}
// svt_aom_variance{W}x{H}_c / svt_aom_highbd_10_variance{W}x{H}_c: ibc::variance_of with width * height samples
IBC_HD uint32_t variance_wh(int64_t sum, uint64_t sse, int count, int bd) {
    if (bd == 8) return (uint32_t)sse - (uint32_t)((sum * sum) / count);
    const uint32_t sse10 = (uint32_t)((sse + 8) >> 4);
    const int64_t  sum10 = (sum + 2) >> 2;
    const int64_t  v = (int64_t)sse10 - (sum10 * sum10) / count;
    return v >= 0 ? (uint32_t)v : 0;
}
// av1_is_dv_valid of the whole-sample vector (row, col) for a block_w x block_h block: ibc::dv_rule with both sides and is_chroma_reference at 4:2:0
IBC_HD int dv_rule(const Job& j, int row, int col) {
    const int bw = j.block_w, bh = j.block_h, mi_row = j.y_pos / 4, mi_col = j.x_pos / 4;
    const int dv_row = 8 * row, dv_col = 8 * col;
    const int src_top_edge = mi_row * 4 * 8 + dv_row, tile_top_edge = j.mi_row_start * 4 * 8;
    if (src_top_edge < tile_top_edge) return 1;
    const int src_left_edge = mi_col * 4 * 8 + dv_col, tile_left_edge = j.mi_col_start * 4 * 8;
    if (src_left_edge < tile_left_edge) return 2;
    const int src_bottom_edge = (mi_row * 4 + bh) * 8 + dv_row, tile_bottom_edge = j.mi_row_end * 4 * 8;
    if (src_bottom_edge > tile_bottom_edge) return 3;
    const int src_right_edge = (mi_col * 4 + bw) * 8 + dv_col, tile_right_edge = j.mi_col_end * 4 * 8;
    if (src_right_edge > tile_right_edge) return 4;
    if (((mi_row & 1) || !((bh / 4) & 1)) && ((mi_col & 1) || !((bw / 4) & 1))) {
        if (bw < 8 && src_left_edge < tile_left_edge + 4 * 8) return 5;
        if (bh < 8 && src_top_edge < tile_top_edge + 4 * 8) return 6;
    }
    const int max_mib_size = 1 << j.mib_size_log2, active_sb_row = mi_row >> j.mib_size_log2, active_sb64_col = (mi_col * 4) >> 6, sb_size = max_mib_size * 4;
    const int src_sb_row = ((src_bottom_edge >> 3) - 1) / sb_size, src_sb64_col = ((src_right_edge >> 3) - 1) >> 6;
    const int total_sb64_per_row = ((j.mi_col_end - j.mi_col_start - 1) >> 4) + 1;
    const int active_sb64 = active_sb_row * total_sb64_per_row + active_sb64_col, src_sb64 = src_sb_row * total_sb64_per_row + src_sb64_col;
    if (src_sb64 >= active_sb64 - 4) return 7;
    const int gradient = 1 + 4 + (sb_size > 64), wf_offset = gradient * (active_sb_row - src_sb_row);
    if (src_sb_row > active_sb_row || src_sb64_col >= active_sb64_col - 4 + wf_offset) return 8;
    if (sb_size == 64) {
        if (src_sb64_col > active_sb64_col + (active_sb_row - src_sb_row)) return 9;
    } else {
        const int src_sb128_col = ((src_right_edge >> 3) - 1) >> 7, active_sb128_col = (mi_col * 4) >> 7;
        if (src_sb128_col > active_sb128_col + (active_sb_row - src_sb_row)) return 9;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the diamond
// An evaluator EV gives the walks their sums.  On the device every lane of a wave runs the walk with the same values and EV takes the sums across the lanes.
//   uint32_t sad(row, col)            the block against the block displaced by (row, col)
//   void     sads(rows, cols, n, centre_row, centre_col, len, mask, out)   sad of centre + len * site j for every j < n whose bit of mask is set
//   uint32_t var(row, col)            the variance
struct Pass {
    int32_t sad, row, col, num00, var;   // var: svt_av1_get_mvpred_var(row, col), or sad when sad is INT_MAX
};
template <class EV> IBC_HD int pred_var(const EV& ev, const Job& J, int row, int col, const int32_t* jc, const int32_t* cc) {
    return ibc::pred_cost(ev.var(row, col), mvpred_cost(J, row, col, jc, cc));
}
// svt_av1_diamond_search_sad_c at search_param, from the clamped mvp_full
template <class EV> IBC_HD Pass diamond_pass(const EV& ev, const Job& J, int search_param, const int32_t* jc, const int32_t* cc) {
    const int tot_steps = MAX_MVSEARCH_STEPS - search_param;
    const int ref_row = clampi(J.mvp_row, J.row_min, J.row_max), ref_col = clampi(J.mvp_col, J.col_min, J.col_max);
    int       br = ref_row, bc = ref_col, num00 = 0, best_site = 0, last_site = 0, i = 1;
    uint32_t  bestsad = ev.sad(br, bc) + mvsad_err_cost(J, br, bc, jc, cc);
    for (int step = 0; step < tot_steps; ++step) {
        const int len = MAX_FIRST_STEP >> (search_param + step);
        unsigned  mask = 0;
        for (int j = 0; j < 8; ++j) mask |= (unsigned)mv_in(J, br + len * unpack(SITE_ROWS, j), bc + len * unpack(SITE_COLS, j)) << j;
        uint32_t s[8];
        ev.sads(SITE_ROWS, SITE_COLS, 8, br, bc, len, mask, s);
        for (int j = 0; j < 8; ++j, ++i) {
            if (!((mask >> j) & 1) || !(s[j] < bestsad)) continue;
            const uint32_t t = s[j] + mvsad_err_cost(J, br + len * unpack(SITE_ROWS, j), bc + len * unpack(SITE_COLS, j), jc, cc);
            if (t < bestsad) {
                bestsad = t;
                best_site = i;
            }
        }
        if (best_site != last_site) {   // an absolute index: its step gives the len, its place in the step the direction
            const int k = (best_site - 1) & 7, l = MAX_FIRST_STEP >> (search_param + ((best_site - 1) >> 3));
            br += l * unpack(SITE_ROWS, k);
            bc += l * unpack(SITE_COLS, k);
            last_site = best_site;
        } else if (br == ref_row && bc == ref_col) {
            ++num00;
        }
    }
    Pass p{(int32_t)bestsad, br, bc, num00, 0};
    p.var = p.sad < INT32_MAX ? pred_var(ev, J, br, bc, jc, cc) : p.sad;
    return p;
}
// svt_av1_refining_search_sad from (*row, *col): at most REFINE_RANGE rounds of the four neighbours
template <class EV> IBC_HD int refining_search(const EV& ev, const Job& J, int* row, int* col, const int32_t* jc, const int32_t* cc) {
    uint32_t best_sad = ev.sad(*row, *col) + mvsad_err_cost(J, *row, *col, jc, cc);
    for (int i = 0; i < REFINE_RANGE; ++i) {
        int      best_site = -1;
        unsigned mask = 0;
        for (int j = 0; j < 4; ++j) mask |= (unsigned)mv_in(J, *row + unpack(NEIGH_ROWS, j), *col + unpack(NEIGH_COLS, j)) << j;
        uint32_t s[8];
        ev.sads(NEIGH_ROWS, NEIGH_COLS, 4, *row, *col, 1, mask, s);
        for (int j = 0; j < 4; ++j) {
            if (!((mask >> j) & 1) || !(s[j] < best_sad)) continue;
            const uint32_t t = s[j] + mvsad_err_cost(J, *row + unpack(NEIGH_ROWS, j), *col + unpack(NEIGH_COLS, j), jc, cc);
            if (t < best_sad) {
                best_sad = t;
                best_site = j;
            }
        }
        if (best_site == -1) break;
        *row += unpack(NEIGH_ROWS, best_site);
        *col += unpack(NEIGH_COLS, best_site);
    }
    return (int)best_sad;
}
struct Diamond {
    int32_t passes, refined, var, row, col;
};
// full_pixel_diamond with do_refine = 1.  get(n) is the pass at step_param + n: every pass starts from the same point, so they may have been walked ahead of time
// and side by side; which of them count is decided here, in the reference's order
template <class EV, class GET> IBC_HD Diamond full_pixel_diamond(const EV& ev, const Job& J, GET get, const int32_t* jc, const int32_t* cc) {
    const int further_steps = MAX_MVSEARCH_STEPS - 1 - J.step_param;
    const Pass first = get(0);
    int        n = first.num00, num00 = 0, do_refine = 1;
    Diamond    d{1, 0, first.var, first.row, first.col};
    if (n > further_steps) do_refine = 0;
    while (n < further_steps) {
        ++n;
        if (num00) {
            --num00;
        } else {
            const Pass p = get(n);
            ++d.passes;
            num00 = p.num00;
            if (num00 > further_steps - n) do_refine = 0;
            if (p.var < d.var) {
                d.var = p.var;
                d.row = p.row;
                d.col = p.col;
            }
        }
    }
    if (do_refine) {
        int row = d.row, col = d.col;
        int thissme = refining_search(ev, J, &row, &col, jc, cc);
        if (thissme < INT32_MAX) thissme = pred_var(ev, J, row, col, jc, cc);
        d.refined = 1;
        if (thissme < d.var) {
            d.var = thissme;
            d.row = row;
            d.col = col;
        }
    }
    return d;
}

// ---------------------------------------------------------------------------------------------------------------- the mesh
// exhuastive_mesh_search's scan around a clamped centre.  Row i < nrows is centre + start_row + i * step; column k < ncols is centre + start_col + k * col_stride.
// step > 1: every step-th column (the reference's col_step).  step == 1: the reference takes the columns four at a time and, in the last group when it is not
// full, `end_col - c` of them and not `end_col - c + 1`: when the number of columns is no multiple of 4 the last column of every row is never examined.
// The scan index of (i, k) is 1 + i * ncols + k; 0 is the centre, which the reference evaluates first.
struct MeshGeom {
    int32_t centre_row, centre_col, start_row, start_col, step, col_stride, nrows, ncols;
};
IBC_HD int mesh_columns(int start_col, int end_col, int step) {
    const int n = end_col - start_col + 1;
    if (n <= 0) return 0;
    return step > 1 ? (n - 1) / step + 1 : n - ((n & 3) != 0);
}
IBC_HD MeshGeom mesh_geom(const Job& J, int centre_row, int centre_col, int range, int step) {
    MeshGeom g;
    g.centre_row = clampi(centre_row, J.row_min, J.row_max);
    g.centre_col = clampi(centre_col, J.col_min, J.col_max);
    g.start_row = imax(-range, J.row_min - g.centre_row);
    g.start_col = imax(-range, J.col_min - g.centre_col);
    const int end_row = imin(range, J.row_max - g.centre_row), end_col = imin(range, J.col_max - g.centre_col);
    g.step = step;
    g.col_stride = step > 1 ? step : 1;
    g.nrows = end_row >= g.start_row ? (end_row - g.start_row) / step + 1 : 0;
    g.ncols = mesh_columns(g.start_col, end_col, step);
    return g;
}
// (total, scan index) as one key: the smallest key is the first strict minimum in scan order
IBC_HD uint64_t mesh_key(uint32_t total, uint32_t index) { return ((uint64_t)total << 32) | index; }
IBC_HD void mesh_decode(const MeshGeom& g, uint64_t key, int* row, int* col) {
    const uint32_t index = (uint32_t)key;
    if (index == 0) {
        *row = g.centre_row;
        *col = g.centre_col;
    } else {
        *row = g.centre_row + g.start_row + (int)((index - 1) / (uint32_t)g.ncols) * g.step;
        *col = g.centre_col + g.start_col + (int)((index - 1) % (uint32_t)g.ncols) * g.col_stride;
    }
}
// full_pixel_exhaustive as a walk of at most MAX_MESH_STEP scans.  run: scan `pass` is to be made at (range, step) around (row, col); after the walk (row, col)
// is its winner and best the last scan's total.  passes: scans made.  pat: range, interval x 4
struct MeshState {
    int32_t run, pass, range, step, row, col, best, progressive, passes;
};
IBC_HD bool pattern_ok(int range, int interval) { return interval >= 1 && range >= 1 && range <= MAX_RANGE; }
// the patterns a walk can reach are usable: pattern 0 may be anything (an invalid one is the reference's `return INT_MAX`); pattern i >= 1 is reached when
// pattern 0 is valid (the centre can widen its range and interval past the two thresholds) and no pattern 1 .. i - 1 has interval 1
inline bool patterns_ok(const int32_t* pat) {
    if (!pat) return false;
    const int range = pat[0], interval = pat[1];
    if (range < MIN_RANGE || range > MAX_RANGE || interval < MIN_INTERVAL || interval > range) return true;
    if (interval == 1 && 2 * range > MAX_RANGE) return true;   // interval stays max(1, range' / range) = 1: no progressive scan
    for (int i = 1; i < MAX_MESH_STEP; ++i) {
        if (!pattern_ok(pat[2 * i], pat[2 * i + 1])) return false;
        if (pat[2 * i + 1] == 1) break;
    }
    return true;
}
IBC_HD MeshState mesh_begin(const int32_t* pat, int centre_row, int centre_col) {
    MeshState s{0, 0, pat[0], pat[1], centre_row, centre_col, INT32_MAX, 0, 0};
    if (s.range < MIN_RANGE || s.range > MAX_RANGE || s.step < MIN_INTERVAL || s.step > s.range) return s;
    const int baseline_interval_divisor = s.range / s.step;
    s.range = imin(imax(s.range, (5 * imax(iabs(centre_row), iabs(centre_col))) / 4), MAX_RANGE);
    s.step = imax(s.step, s.range / baseline_interval_divisor);
    s.progressive = s.step > MIN_INTERVAL && s.range > MIN_RANGE;
    s.run = 1;
    return s;
}
// scan s.pass gave (total, row, col): the next scan, or the end
IBC_HD void mesh_advance(MeshState& s, const int32_t* pat, uint32_t total, int row, int col) {
    s.best = (int32_t)total;
    s.row = row;
    s.col = col;
    ++s.passes;
    const bool last = !s.progressive || s.pass == MAX_MESH_STEP - 1 || (s.pass >= 1 && pat[2 * s.pass + 1] == 1);
    if (last) {
        s.run = 0;
        return;
    }
    ++s.pass;
    s.range = pat[2 * s.pass];
    s.step = pat[2 * s.pass + 1];
}
// one scan, serially: the smallest key
template <class EV> inline uint64_t mesh_scan_host(const EV& ev, const Job& J, const MeshGeom& g, const int32_t* jc, const int32_t* cc) {
    uint64_t best = mesh_key(ev.sad(g.centre_row, g.centre_col) + mvsad_err_cost(J, g.centre_row, g.centre_col, jc, cc), 0);
    for (int i = 0; i < g.nrows; ++i)
        for (int k = 0; k < g.ncols; ++k) {
            const int      row = g.centre_row + g.start_row + i * g.step, col = g.centre_col + g.start_col + k * g.col_stride;
            const uint64_t key = mesh_key(ev.sad(row, col) + mvsad_err_cost(J, row, col, jc, cc), 1u + (uint32_t)(i * g.ncols + k));
            if (key < best) best = key;
        }
    return best;
}

// ---------------------------------------------------------------------------------------------------------------- the choice
IBC_HD int exhaustive_thr(const Job& J) { return ((1 << 25) >> (10 - (ilog2(J.block_w / 4) + ilog2(J.block_h / 4)))) << J.ibc_shift; }
IBC_HD bool hash_applies(const Job& J) { return J.use_hash && J.block_w == J.block_h; }
IBC_HD SvtHipIbcSearchJob hash_job(const Job& J, bool applies) {
    return SvtHipIbcSearchJob{J.x_pos,      J.y_pos,      applies ? J.block_w : 0, J.intra,        J.col_min,    J.col_max,      J.row_min,      J.row_max,
                              J.ref_mv_row, J.ref_mv_col, J.error_per_bit,         J.mi_row_start, J.mi_row_end, J.mi_col_start, J.mi_col_end, J.mib_size_log2};
}
IBC_HD Result empty_full_result(int status) {
    Result R{};
    R.status = status;
    R.dia_var = R.mesh_var = R.var = INT32_MAX;
    R.hash = ibc::empty_result(0);
    return R;
}
IBC_HD void set_diamond(Result& R, const Diamond& d) {
    R.dia_passes = d.passes;
    R.dia_refined = d.refined;
    R.dia_var = d.var;
    R.dia_row = d.row;
    R.dia_col = d.col;
}
// svt_av1_full_pixel_search's two comparisons and the caller's av1_is_dv_valid, from the stages' results already in R
IBC_HD void choose(Result& R, const Job& J) {
    R.source = 0;
    R.var = R.dia_var;
    R.best_row = R.dia_row;
    R.best_col = R.dia_col;
    if (R.mesh_ran && R.mesh_var < R.var) {
        R.source = 1;
        R.var = R.mesh_var;
        R.best_row = R.mesh_row;
        R.best_col = R.mesh_col;
    }
    if (R.hash.found && R.hash.best_cost < R.var) {
        R.source = 2;
        R.var = R.hash.best_cost;
        R.best_row = R.hash.best_row;
        R.best_col = R.hash.best_col;
    }
    R.dv_valid = dv_rule(J, R.best_row, R.best_col) == 0;
}

// ---------------------------------------------------------------------------------------------------------------- the serial host form
template <class PIX> struct HostEval {
    const PIX* luma;
    int        stride, x_pos, y_pos, bw, bh, bd;
    const PIX* at(int row, int col) const { return luma + (ptrdiff_t)(y_pos + row) * stride + (x_pos + col); }
    uint32_t   sad(int row, int col) const {
        const PIX *a = at(0, 0), *b = at(row, col);
        uint32_t   s = 0;
        for (int y = 0; y < bh; ++y)
            for (int x = 0; x < bw; ++x) s += (uint32_t)iabs((int)a[(ptrdiff_t)y * stride + x] - (int)b[(ptrdiff_t)y * stride + x]);
        return s;
    }
    void sads(uint32_t rows, uint32_t cols, int n, int centre_row, int centre_col, int len, unsigned mask, uint32_t* out) const {
        for (int j = 0; j < n; ++j) out[j] = (mask >> j) & 1 ? sad(centre_row + len * unpack(rows, j), centre_col + len * unpack(cols, j)) : 0;
    }
    uint32_t var(int row, int col) const {
        const PIX *a = at(0, 0), *b = at(row, col);
        int64_t    sum = 0;
        uint64_t   sse = 0;
        for (int y = 0; y < bh; ++y)
            for (int x = 0; x < bw; ++x) {
                const int d = (int)a[(ptrdiff_t)y * stride + x] - (int)b[(ptrdiff_t)y * stride + x];
                sum += d;
                sse += (uint64_t)(d * d);
            }
        return variance_wh(sum, sse, bw * bh, bd);
    }
};

inline bool full_search_args_ok(int pix_bytes, int bd, const void* luma, int stride, int width, int height, const void* bucket_start, const void* entries,
                                const void* joint_cost, const void* comp_cost, const int32_t* mesh_patterns, const void* jobs, int njobs, const void* results) {
    return luma && joint_cost && comp_cost && jobs && results && njobs >= 0 && njobs <= MAX_JOBS && !bucket_start == !entries && ibc::fmt_ok(pix_bytes, bd) &&
           ibc::picture_ok(stride, width, height) && patterns_ok(mesh_patterns);
}
template <class PIX> inline Result full_search_job_host(const PIX* luma, int stride, int width, int height, int bd, const int32_t* bucket_start,
                                                        const SvtHipIbcHashEntry* entries, const int32_t* jc, const int32_t* cc, const int32_t* pat, const Job& J,
                                                        uint32_t* buf) {
    const int status = job_status(J, width, height, bucket_start != nullptr);
    Result    R = empty_full_result(status);
    if (status) return R;
    const HostEval<PIX> ev{luma, stride, J.x_pos, J.y_pos, J.block_w, J.block_h, bd};
    set_diamond(R, full_pixel_diamond(ev, J, [&](int n) { return diamond_pass(ev, J, J.step_param + n, jc, cc); }, jc, cc));
    if (J.exhaustive_allowed && R.dia_var > exhaustive_thr(J)) {
        R.mesh_ran = 1;
        MeshState s = mesh_begin(pat, R.dia_row, R.dia_col);
        while (s.run) {
            const MeshGeom g = mesh_geom(J, s.row, s.col, s.range, s.step);
            const uint64_t key = mesh_scan_host(ev, J, g, jc, cc);
            int            row, col;
            mesh_decode(g, key, &row, &col);
            mesh_advance(s, pat, (uint32_t)(key >> 32), row, col);
        }
        R.mesh_passes = s.passes;
        if (s.passes) {
            R.mesh_var = s.best < INT32_MAX ? pred_var(ev, J, s.row, s.col, jc, cc) : s.best;
            R.mesh_row = s.row;
            R.mesh_col = s.col;
        }
    }
    if (hash_applies(J)) {
        R.hash = ibc::search_job_host(luma, stride, width, height, bd, bucket_start, entries, jc, cc, hash_job(J, true), buf);
        if (R.hash.count < 0) R.hash = ibc::empty_result(0);
    }
    choose(R, J);
    return R;
}
inline void full_search_host(int pix_bytes, int bd, const void* luma, int stride, int width, int height, const int32_t* bucket_start, const SvtHipIbcHashEntry* entries,
                             const int32_t* jc, const int32_t* cc, const int32_t* pat, const Job* jobs, int njobs, Result* results) {
    static thread_local uint32_t buf[2 * 64 * 64 + 2 * 32 * 32];
    for (int j = 0; j < njobs; ++j)
        results[j] = pix_bytes == 1 ? full_search_job_host((const uint8_t*)luma, stride, width, height, bd, bucket_start, entries, jc, cc, pat, jobs[j], buf)
                                    : full_search_job_host((const uint16_t*)luma, stride, width, height, bd, bucket_start, entries, jc, cc, pat, jobs[j], buf);
}

// d_scratch of the device call: the walks' states, the strips' partial minima of one scan, the hash search's derived jobs and its results; parts on multiples of 256
struct FullScratch {
    size_t state, partial, hash_jobs, hash_results, total;
};
inline FullScratch full_scratch(int njobs) {
    FullScratch L{};
    const size_t n = njobs > 0 ? (size_t)njobs : 0;
    size_t       at = 0;
    const auto   take = [&](size_t bytes) { const size_t r = at; at += (bytes + 255) & ~(size_t)255; return r; };
    L.state = take(n * sizeof(MeshState));
    L.partial = take(n * MESH_STRIPS * sizeof(uint64_t));
    L.hash_jobs = take(n * sizeof(SvtHipIbcSearchJob));
    L.hash_results = take(n * sizeof(SvtHipIbcSearchResult));
    L.total = at;
    return L;
}

}  // namespace ibcs
