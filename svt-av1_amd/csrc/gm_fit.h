// gm_fit.h — the arithmetic of the global-motion model fit, written once for the device (gm_fit.hip) and for a host compiler (tests/gm_fit_host.cpp runs it against
// the reference, no device needed): RANSAC (Encoder/Codec/ransac.c:34-542 with lcg_rand16 of random.h:20-23 and least_squares / linsolve / multiply_mat of
// mathutils.h:26-111), svt_av1_convert_model_to_params (global_motion.c:41-86) and the MIN_INLIER_PROB rule (global_motion.c:310-318).  Every operation is an IEEE
// double + - * / sqrt fabs floor in the reference's order; both builds use -ffp-contract=off, and results are compared by bit pattern.  docs/kernels/gm.md.
//
// A point list is the correspondence layout of svt_hip_gm_correspondences_batch_dev: corr[i] = x, y (source), rx, ry (reference).  A point SET is a list of indices
// into it (uint16_t: a list holds at most SVT_HIP_GM_MAX_CORNERS = 4096 points); nothing is copied or normalised in place: a normalised coordinate is recomputed
// from the point and the set's GmFitNorm wherever the reference reads its normalised copy, which gives the same bits ((x - mean) * scale, two roundings).
#pragma once
#include <math.h>
#include <stdint.h>
#include "gm_walk.h"

#define GM_FIT_TRIALS 20               // MIN_TRIALS
#define GM_FIT_MAX_DEGENERATE_ITER 10  // MAX_DEGENERATE_ITER
#define GM_FIT_MINPTS 3                // minpts of all three model types
#define GM_FIT_MIN_POINTS 15           // minpts * MINPTS_MULTIPLIER
#define GM_FIT_INLIER_THRESHOLD 1.25
#define GM_FIT_WORK 42                 // doubles of work space of one fit: at_a[n][n] then atb[n], n <= 6

struct GmFitNorm { double mean0, mean1, scale; };   // normalize_homography's T = {scale, 0, -scale mean0; 0, scale, -scale mean1; 0, 0, 1}

// ------------------------------------------------------------------------------------------------ draws
GM_HD uint32_t gm_fit_rand16(uint32_t* state) {
    *state = (uint32_t)(*state * 1103515245ULL + 12345);
    return *state / 65536 % 32768;
}

// get_rand_indices' walk `while (index) { step ptr; if ptr is not chosen: index-- }` as arithmetic: the position of the m-th not-chosen slot after ptr on the ring
// of n.  c0, c1 = the chosen slots (nchosen = 1: only c0).  The slot ptr stands on is never counted, chosen or not.  A whole turn of the ring passes n - chosen free
// slots, so only the remainder matters; of the remainder's steps, a chosen slot at ring distance d (1..n) ahead costs one extra step when it is reached.
GM_HD int gm_fit_advance(int ptr, int n, int m, int c0, int c1, int nchosen) {
    if (!m) return ptr;
    int da = c0 - ptr, db = (nchosen > 1 ? c1 : c0) - ptr;
    if (da <= 0) da += n;
    if (db <= 0) db += n;
    const int distinct = da == db ? 1 : 2;
    const int lo = da < db ? da : db, hi = da < db ? db : da;
    const int f = n - distinct;
    if (f <= 0) return ptr;   // no free slot: the reference would not return (never reached: n >= 3 here)
    int s = (m - 1) % f + 1;
    if (s >= lo) s++;
    if (distinct > 1 && s >= hi) s++;
    return (ptr + s) % n;
}

// get_rand_indices(npoints, 3, indices, seed).  ptr advances past indices[0] but not past indices[1]: a zero draw for the third index repeats the second.
GM_HD int gm_fit_rand_indices(int n, uint32_t* seed, int* i0, int* i1, int* i2) {
    int ptr = (int)(gm_fit_rand16(seed) % (uint32_t)n);
    if (GM_FIT_MINPTS > n) return 0;
    *i0 = ptr;
    ptr = ptr == n - 1 ? 0 : ptr + 1;
    ptr = gm_fit_advance(ptr, n, (int)(gm_fit_rand16(seed) % (uint32_t)n), *i0, *i0, 1);
    *i1 = ptr;
    ptr = gm_fit_advance(ptr, n, (int)(gm_fit_rand16(seed) % (uint32_t)n), *i0, *i1, 2);
    *i2 = ptr;
    return 1;
}

// is_degenerate_translation / is_degenerate_affine (is_collinear3) of the source sides of three points
GM_HD int gm_fit_degenerate(int type, const int32_t* a, const int32_t* b, const int32_t* c) {
    const double ax = a[0], ay = a[1], bx = b[0], by = b[1], cx = c[0], cy = c[1];
    if (type == 1) return (ax - bx) * (ax - bx) + (ay - by) * (ay - by) <= 2;
    const double v = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    return fabs(v) < 1e-3;
}

// The draws of all trials: one serial chain (the seed runs through the trials, a redraw depends on the points).  idx[t][0..2] = trial t's triple.
// 0 = drawn; 1 = the fit returns 1 (a draw degenerate more than MAX_DEGENERATE_ITER times, or get_rand_indices failed).  A trial whose find_transformation
// fails draws nothing else, so the draws do not depend on the fits.
GM_HD int gm_fit_draw_trials(int type, const int32_t* corr, int n, uint16_t (*idx)[4]) {
    uint32_t seed = (uint32_t)n;
    for (int t = 0; t < GM_FIT_TRIALS; t++) {
        int degenerate = 1, iter = 0;
        while (degenerate) {
            iter++;
            int i0, i1, i2;
            if (!gm_fit_rand_indices(n, &seed, &i0, &i1, &i2)) return 1;
            degenerate = gm_fit_degenerate(type, corr + 4 * i0, corr + 4 * i1, corr + 4 * i2);
            if (iter > GM_FIT_MAX_DEGENERATE_ITER) return 1;
            idx[t][0] = (uint16_t)i0; idx[t][1] = (uint16_t)i1; idx[t][2] = (uint16_t)i2; idx[t][3] = 0;
        }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ normalize_homography, as ordered sums
// comp 0, 1 = x, y of the source side, 2, 3 = of the reference side: sum of the coordinate over the set, in the set's order
GM_HD double gm_fit_sum_coord(const int32_t* corr, const uint16_t* idx, int np, int comp) {
    double s = 0;
    for (int k = 0; k < np; k++) s += (double)corr[4 * idx[k] + comp];
    return s;
}
// side 0 / 1; nm->mean0 / mean1 are set: the sum of the distances to the mean
GM_HD double gm_fit_sum_msqe(const int32_t* corr, const uint16_t* idx, int np, int side, const GmFitNorm* nm) {
    double msqe = 0;
    for (int k = 0; k < np; k++) {
        const double p0 = (double)corr[4 * idx[k] + 2 * side] - nm->mean0, p1 = (double)corr[4 * idx[k] + 2 * side + 1] - nm->mean1;
        msqe += sqrt(p0 * p0 + p1 * p1);
    }
    return msqe;
}
GM_HD void gm_fit_norm_scale(GmFitNorm* nm, double msqe, int np) {
    msqe /= np;
    nm->scale = msqe == 0 ? 1.0 : sqrt(2.0) / msqe;
}
// the normalised point: sx, sy of the source side under a, dx, dy of the reference side under b
GM_HD void gm_fit_npoint(const int32_t* c, const GmFitNorm* a, const GmFitNorm* b, double* sx, double* sy, double* dx, double* dy) {
    double v;
    v = (double)c[0] - a->mean0; *sx = v * a->scale;
    v = (double)c[1] - a->mean1; *sy = v * a->scale;
    v = (double)c[2] - b->mean0; *dx = v * b->scale;
    v = (double)c[3] - b->mean1; *dy = v * b->scale;
}

// ------------------------------------------------------------------------------------------------ the normal equations, one ordered sum per cell
// row 2p + r of find_rotzoom's / find_affine's matrix a, column c
GM_HD double gm_fit_a(int type, int r, int c, double sx, double sy) {
    if (type == 2) {
        if (!r) return c == 0 ? sx : c == 1 ? sy : c == 2 ? 1.0 : 0.0;
        return c == 0 ? sy : c == 1 ? -sx : c == 2 ? 0.0 : 1.0;
    }
    if (!r) return c == 0 ? sx : c == 1 ? sy : c == 4 ? 1.0 : 0.0;
    return c == 2 ? sx : c == 3 ? sy : c == 5 ? 1.0 : 0.0;
}
GM_HD int gm_fit_dim(int type) { return type == 1 ? 0 : type == 2 ? 4 : 6; }
// how many independent ordered sums a fit of this type has: TRANSLATION sumx, sumy; else the n (n + 1) / 2 cells of the upper triangle of at_a, then the n of atb
GM_HD int gm_fit_cells(int type) { const int n = gm_fit_dim(type); return n ? n * (n + 1) / 2 + n : 2; }

// cell q of the fit over the set, and where it goes in work (at_a[i][j] and its mirror, atb[i]; TRANSLATION: work[0], work[1])
GM_HD void gm_fit_cell(int type, int q, const int32_t* corr, const uint16_t* idx, int np, const GmFitNorm* a, const GmFitNorm* b, double* work) {
    const int n = gm_fit_dim(type);
    double sum = 0, sx, sy, dx, dy;
    if (!n) {
        for (int k = 0; k < np; k++) {
            gm_fit_npoint(corr + 4 * idx[k], a, b, &sx, &sy, &dx, &dy);
            sum += q ? dy - sy : dx - sx;
        }
        work[q] = sum;
        return;
    }
    const int tri = n * (n + 1) / 2;
    if (q >= tri) {
        const int i = q - tri;
        for (int k = 0; k < np; k++) {
            gm_fit_npoint(corr + 4 * idx[k], a, b, &sx, &sy, &dx, &dy);
            sum += gm_fit_a(type, 0, i, sx, sy) * dx;
            sum += gm_fit_a(type, 1, i, sx, sy) * dy;
        }
        work[n * n + i] = sum;
        return;
    }
    int i = 0, j = q;
    while (j >= n - i) { j -= n - i; i++; }
    j += i;
    for (int k = 0; k < np; k++) {
        gm_fit_npoint(corr + 4 * idx[k], a, b, &sx, &sy, &dx, &dy);
        sum += gm_fit_a(type, 0, i, sx, sy) * gm_fit_a(type, 0, j, sx, sy);
        sum += gm_fit_a(type, 1, i, sx, sy) * gm_fit_a(type, 1, j, sx, sy);
    }
    work[i * n + j] = sum;
    work[j * n + i] = sum;
}

// linsolve (mathutils.h:26-62), stride = n.  0 = singular: x is written as far as the back substitution got.
GM_HD int gm_fit_linsolve(int n, double* A, double* b, double* x) {
    const double tiny_near_zero = 1.0E-16;
    double c;
    for (int k = 0; k < n - 1; k++) {
        for (int i = n - 1; i > k; i--) {
            if (fabs(A[(i - 1) * n + k]) < fabs(A[i * n + k])) {
                for (int j = 0; j < n; j++) {
                    c = A[i * n + j];
                    A[i * n + j] = A[(i - 1) * n + j];
                    A[(i - 1) * n + j] = c;
                }
                c = b[i];
                b[i] = b[i - 1];
                b[i - 1] = c;
            }
        }
        for (int i = k; i < n - 1; i++) {
            if (fabs(A[k * n + k]) < tiny_near_zero) return 0;
            c = A[(i + 1) * n + k] / A[k * n + k];
            for (int j = 0; j < n; j++) A[(i + 1) * n + j] -= c * A[k * n + j];
            b[i + 1] -= c * b[k];
        }
    }
    for (int i = n - 1; i >= 0; i--) {
        if (fabs(A[i * n + i]) < tiny_near_zero) return 0;
        c = 0;
        for (int j = i + 1; j <= n - 1; j++) c += A[i * n + j] * x[j];
        x[i] = (b[i] - c) / A[i * n + i];
    }
    return 1;
}

// ------------------------------------------------------------------------------------------------ denormalize_*_reorder
GM_HD void gm_fit_mul3(const double* m1, const double* m2, double* res) {   // multiply_mat(m1, m2, res, 3, 3, 3)
    for (int row = 0; row < 3; row++)
        for (int col = 0; col < 3; col++) {
            double sum = 0;
            for (int inner = 0; inner < 3; inner++) sum += m1[row * 3 + inner] * m2[inner * 3 + col];
            res[row * 3 + col] = sum;
        }
}
GM_HD void gm_fit_denormalize(double* pd, const GmFitNorm* a, const GmFitNorm* b) {   // denormalize_homography(pd, t1, t2)
    const double t1[9] = {a->scale, 0, -a->scale * a->mean0, 0, a->scale, -a->scale * a->mean1, 0, 0, 1};
    const double t22 = -b->scale * b->mean0, t25 = -b->scale * b->mean1;
    const double is = 1.0 / b->scale;
    const double it2[9] = {is, 0, -t22 * is, 0, is, -t25 * is, 0, 0, 1};   // invnormalize_mat
    double p2[9];
    gm_fit_mul3(pd, t1, p2);
    gm_fit_mul3(it2, p2, pd);
}

// The end of find_translation / find_rotzoom / find_affine once every cell is in work: the solve and the denormalisation.  params receives x directly, as the
// reference's mat does: on a singular system (return 1) it holds what linsolve wrote and is not denormalised.
GM_HD int gm_fit_solve(int type, int np, double* work, const GmFitNorm* a, const GmFitNorm* b, double* params) {
    double pd[9];
    if (type == 1) {
        params[0] = work[0] / np;
        params[1] = work[1] / np;
        pd[0] = 1; pd[1] = 0; pd[2] = params[0]; pd[3] = 0; pd[4] = 1; pd[5] = params[1]; pd[6] = pd[7] = 0; pd[8] = 1;
        gm_fit_denormalize(pd, a, b);
        params[0] = pd[2]; params[1] = pd[5];
        params[2] = params[5] = 1;
        params[3] = params[4] = 0;
        params[6] = params[7] = 0;
        return 0;
    }
    const int n = gm_fit_dim(type);
    if (!gm_fit_linsolve(n, work, work + n * n, params)) return 1;
    if (type == 2) {
        pd[0] = params[0]; pd[1] = params[1]; pd[2] = params[2]; pd[3] = -params[1]; pd[4] = params[0]; pd[5] = params[3]; pd[6] = pd[7] = 0; pd[8] = 1;
        gm_fit_denormalize(pd, a, b);
        params[0] = pd[2]; params[1] = pd[5]; params[2] = pd[0]; params[3] = pd[1];
        params[4] = -params[3];   // -0.0 when params[3] is +0.0
        params[5] = params[2];
    } else {
        pd[0] = params[0]; pd[1] = params[1]; pd[2] = params[4]; pd[3] = params[2]; pd[4] = params[3]; pd[5] = params[5]; pd[6] = pd[7] = 0; pd[8] = 1;
        gm_fit_denormalize(pd, a, b);
        params[0] = pd[2]; params[1] = pd[5]; params[2] = pd[0]; params[3] = pd[1]; params[4] = pd[3]; params[5] = pd[4];
    }
    params[6] = params[7] = 0;
    return 0;
}

// find_transformation over a set, serially (the three-point fit of a trial; the host build's recomputation).  nm = two GmFitNorm, work = GM_FIT_WORK doubles.
GM_HD void gm_fit_norms(const int32_t* corr, const uint16_t* idx, int np, GmFitNorm* nm) {
    for (int side = 0; side < 2; side++) {
        nm[side].mean0 = gm_fit_sum_coord(corr, idx, np, 2 * side) / np;
        nm[side].mean1 = gm_fit_sum_coord(corr, idx, np, 2 * side + 1) / np;
        gm_fit_norm_scale(nm + side, gm_fit_sum_msqe(corr, idx, np, side, nm + side), np);
    }
}
GM_HD int gm_fit_find(int type, const int32_t* corr, const uint16_t* idx, int np, GmFitNorm* nm, double* work, double* params) {
    gm_fit_norms(corr, idx, np, nm);
    for (int q = 0; q < gm_fit_cells(type); q++) gm_fit_cell(type, q, corr, idx, np, nm, nm + 1, work);
    return gm_fit_solve(type, np, work, nm, nm + 1, params);
}

// ------------------------------------------------------------------------------------------------ inliers and selection
// project_points_double_* of one point, then its distance to the reference side
GM_HD double gm_fit_distance(int type, const double* mat, const int32_t* c) {
    const double x = c[0], y = c[1];
    double px, py;
    if (type == 1) { px = x + mat[0]; py = y + mat[1]; }
    else if (type == 2) { px = mat[2] * x + mat[3] * y + mat[0]; py = -mat[3] * x + mat[2] * y + mat[1]; }
    else { px = mat[2] * x + mat[3] * y + mat[0]; py = mat[4] * x + mat[5] * y + mat[1]; }
    const double dx = px - (double)c[2], dy = py - (double)c[3];
    return sqrt(dx * dx + dy * dy);
}
GM_HD double gm_fit_variance(int cnt, double sum_distance, double sum_distance_squared) {
    const double mean_distance = sum_distance / ((double)cnt);
    return sum_distance_squared / ((double)cnt - 1.0) - mean_distance * mean_distance * ((double)cnt) / ((double)cnt - 1.0);
}
// The keep rule replayed over the trials in order (one kept motion: RANSAC_NUM_MOTIONS = 1).  ok[t] = trial t's find_transformation succeeded, cnt / var = its
// inliers and variance (var is read only where cnt > 1).  -> the kept trial, -1 = none; is_better_motion is strict, so of equal motions the earlier stays.
GM_HD int gm_fit_select(const int* ok, const int* cnt, const double* var, int* num_inliers) {
    int kept = -1, kept_num = 0;
    double kept_var = 1e12;   // k_infinite_variance
    for (int t = 0; t < GM_FIT_TRIALS; t++) {
        if (!ok[t]) continue;
        if (cnt[t] >= kept_num && cnt[t] > 1) {
            if (cnt[t] > kept_num || var[t] < kept_var) { kept = t; kept_num = cnt[t]; kept_var = var[t]; }
        }
    }
    *num_inliers = kept_num;
    return kept;
}

// ------------------------------------------------------------------------------------------------ svt_av1_convert_model_to_params and what follows
// (int32_t)floor(v) with the conversion defined for every v: clamped in double first (the reference's conversion is undefined outside int32; such models are
// outside the contract).  NaN gives 0.
GM_HD int32_t gm_fit_to_i32(double v) {
    v = floor(v);
    if (!(v == v)) return 0;
    if (v < -2147483648.0) v = -2147483648.0;
    if (v > 2147483647.0) v = 2147483647.0;
    return (int32_t)v;
}
GM_HD int64_t gm_fit_clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
GM_HD void gm_fit_convert(const double* params, int32_t* model) {   // convert_to_params
    int alpha_present = 0;
    for (int i = 0; i < 2; i++) model[i] = (int32_t)gm_fit_clamp64(gm_fit_to_i32(params[i] * (1 << 6) + 0.5), -(1 << 12), 1 << 12) * (1 << 10);
    for (int i = 2; i < 6; i++) {
        const int diag_value = (i == 2 || i == 5) ? (1 << 15) : 0;
        const int32_t v = (int32_t)gm_fit_clamp64((int64_t)gm_fit_to_i32(params[i] * (1 << 15) + 0.5) - diag_value, -(1 << 12), 1 << 12);
        alpha_present |= (v != 0);
        model[i] = (v + diag_value) * 2;
    }
    for (int i = 6; i < 8; i++) {
        model[i] = (int32_t)gm_fit_clamp64(gm_fit_to_i32(params[i] * (1 << 16) + 0.5), -(1 << 11), 1 << 11);
        alpha_present |= (model[i] != 0);
    }
    if (!alpha_present) {
        const int32_t a0 = model[0] < 0 ? -model[0] : model[0], a1 = model[1] < 0 ? -model[1] : model[1];
        if (a0 < (1 << 10) && a1 < (1 << 10)) model[0] = model[1] = 0;   // MIN_TRANS_THRESH
    }
}

GM_HD void gm_fit_identity(double* params) {
    params[0] = 0; params[1] = 0; params[2] = 1; params[3] = 0; params[4] = 0; params[5] = 1; params[6] = 0; params[7] = 0;
}

// What compute_global_motion does with a fit (EbGlobalMotionEstimation.c:330-350): fit->ret / npoints / num_inliers / params are set; fills the rest, and the
// refinement job where the reference would refine (wmtype -1 = it would not: gm_job_start finishes such a job at once).
GM_HD void gm_fit_finish(SvtHipGmFit* fit, int ref, int n_refinements, SvtHipGmJob* job) {
    const int n = fit->npoints;
    fit->num_inliers_kept = ((double)fit->num_inliers < 0.1 * n || n == 0) ? 0 : fit->num_inliers;   // MIN_INLIER_PROB
    gm_fit_convert(fit->params, fit->wmmat);
    fit->wmtype = gm_get_wmtype(fit->wmmat);
    fit->reserved = 0;
    if (!job) return;
    job->ref = ref;
    job->wmtype = (fit->num_inliers_kept == 0 || fit->wmtype == 0) ? -1 : fit->wmtype;
    for (int k = 0; k < 8; k++) job->wmmat[k] = fit->wmmat[k];
    job->n_refinements = n_refinements;
    job->reserved = 0;
    job->best_frame_error = INT64_MAX;
}
