// gm_walk.h — the integer side of the global-motion refinement, written once for the device (gm.hip) and for a host compiler (tests/gm_walk_host.cpp drives it with
// the reference's own warp error, no device needed): svt_get_shear_params, add_param_offset, force_wmtype, get_wmtype, and the state machine that replays
// svt_av1_refine_integerized_param (Encoder/Codec/global_motion.c:135-259) over batches of speculated candidates.  docs/kernels/gm.md describes the mapping.
#pragma once
#include <stdint.h>
#include "../../include/svt_hip.h"

#if defined(__HIPCC__)
#define GM_HD __host__ __device__ inline
#else
#define GM_HD inline
#endif

// K: how deep both directional runs of a parameter are speculated in the batch that also holds its left / right probes.  A batch is 2 + 2 K candidates; a run that
// outlives K continues in the next round with a batch of GM_NC steps in its one direction.
#define GM_K 4
#define GM_NC (2 + 2 * GM_K)

enum { GM_PHASE_INIT = 0, GM_PHASE_FRESH = 1, GM_PHASE_RUN = 2 };

struct GmState {
    int32_t mat[8];          // the carried struct's wmmat: for ROTZOOM rows 4-5 are whatever the last valid probe left there
    int64_t best, best_frame_error;
    int32_t wmtype, n_ref, n_params, i, p, step, phase, dir, best_param, n_live, probes, rounds, invalid, done;
    int32_t cand_val[GM_NC];       // the value of parameter p in candidate c
    int32_t cand_rows[GM_NC][2];   // ROTZOOM: rows 4-5 of the carried struct once candidate c has been evaluated
    int32_t cand_valid[GM_NC];
};

// Div_Lut of the AV1 specification (7.11.3.7): entry f is 2^22 / (256 + f) rounded to nearest, f = 0..256
GM_HD int gm_div_lut(int f) { return ((1 << 22) + ((256 + f) >> 1)) / (256 + f); }
GM_HD int gm_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
GM_HD int gm_round_signed(int v, int n) { return v < 0 ? -((-v + ((1 << n) >> 1)) >> n) : ((v + ((1 << n) >> 1)) >> n); }
GM_HD int64_t gm_round_signed64(int64_t v, int n) { return v < 0 ? -((-v + (((int64_t)1 << n) >> 1)) >> n) : ((v + (((int64_t)1 << n) >> 1)) >> n); }

// svt_get_shear_params: m = wmmat[0..5] -> o->alpha .. delta, o->valid.  The 16-bit fields wrap exactly as the reference's int16_t members do.
GM_HD void gm_shear_params(const int32_t* m, SvtHipGmModel* o) {
    o->alpha = o->beta = o->gamma = o->delta = 0;
    o->valid = 0;
    if (m[2] <= 0) return;
    int16_t a = (int16_t)gm_clamp(m[2] - (1 << 16), INT16_MIN, INT16_MAX), b = (int16_t)gm_clamp(m[3], INT16_MIN, INT16_MAX);
    // resolve_divisor_32(|m[2]|)
    const uint32_t D = (uint32_t)m[2];
    int shift = 31;
    while (!(D >> shift)) shift--;
    const int32_t e = (int32_t)(D - ((uint32_t)1 << shift));
    const int32_t f = shift > 8 ? (e + ((1 << (shift - 8)) >> 1)) >> (shift - 8) : e << (8 - shift);
    shift += 14;
    const int16_t y = (int16_t)gm_div_lut(f);
    int64_t v = ((int64_t)m[4] * (1 << 16)) * y;
    int16_t g = (int16_t)gm_clamp((int)gm_round_signed64(v, shift), INT16_MIN, INT16_MAX);
    v = ((int64_t)m[3] * m[4]) * y;
    int16_t d = (int16_t)gm_clamp(m[5] - (int)gm_round_signed64(v, shift) - (1 << 16), INT16_MIN, INT16_MAX);
    a = (int16_t)(gm_round_signed(a, 6) * 64); b = (int16_t)(gm_round_signed(b, 6) * 64);
    g = (int16_t)(gm_round_signed(g, 6) * 64); d = (int16_t)(gm_round_signed(d, 6) * 64);
    o->alpha = a; o->beta = b; o->gamma = g; o->delta = d;
    const int aa = a < 0 ? -(int)a : a, ab = b < 0 ? -(int)b : b, ag = g < 0 ? -(int)g : g, ad = d < 0 ? -(int)d : d;
    o->valid = !((4 * aa + 7 * ab >= (1 << 16)) || (4 * ag + 4 * ad >= (1 << 16)));
}

// add_param_offset (global_motion.c:91-113) for the six parameters of an affine model
GM_HD int32_t gm_add_param_offset(int p, int32_t v, int32_t offset) {
    const int scale = p < 2 ? 10 : 1, lim = p < 2 ? (1 << 12) : (1 << 12), one = (p == 2 || p == 5) ? (1 << 16) : 0;
    v = (v - one) >> scale;
    v += offset;
    v = gm_clamp(v, -lim, lim);
    return v * (1 << scale) + one;
}

GM_HD void gm_force_wmtype(int32_t* m, int wmtype) {
    if (wmtype <= 0) m[0] = m[1] = 0;
    if (wmtype <= 1) { m[2] = 1 << 16; m[3] = 0; }
    if (wmtype <= 2) { m[4] = -m[3]; m[5] = m[2]; }
    m[6] = m[7] = 0;
}
GM_HD int gm_get_wmtype(const int32_t* m) {
    if (m[5] == (1 << 16) && !m[4] && m[2] == (1 << 16) && !m[3]) return (!m[1] && !m[0]) ? 0 : 1;
    return (m[2] == m[5] && m[3] == -m[4]) ? 2 : 3;
}

// Candidate c of the batch: parameter p takes `val`; rows = rows 4-5 of the carried struct when the reference would evaluate it (updated to what it leaves there).
// ROTZOOM: svt_get_shear_params sees the OLD rows, svt_warp_plane then rewrites them from wmmat[2..3] -- unless the shear parameters were invalid.
GM_HD void gm_write_cand(GmState* st, SvtHipGmModel* cands, int c, int32_t val, int32_t rows[2]) {
    int32_t m[6];
    for (int k = 0; k < 6; k++) m[k] = (st->n_params && k == st->p) ? val : st->mat[k];   // no dynamically indexed private array on the device
    SvtHipGmModel o;
    if (st->wmtype == 2) {
        m[4] = rows[0]; m[5] = rows[1];
        gm_shear_params(m, &o);
        m[4] = -m[3]; m[5] = m[2];
        if (o.valid) { rows[0] = m[4]; rows[1] = m[5]; }
    } else {
        gm_shear_params(m, &o);
    }
    for (int k = 0; k < 6; k++) o.mat[k] = m[k];
    cands[c] = o;
    st->cand_val[c] = val;
    st->cand_rows[c][0] = rows[0]; st->cand_rows[c][1] = rows[1];
    st->cand_valid[c] = o.valid;
}

GM_HD void gm_write_batch(GmState* st, SvtHipGmModel* cands) {
    int32_t rows[2] = {st->mat[4], st->mat[5]};
    if (st->phase == GM_PHASE_INIT) {
        gm_write_cand(st, cands, 0, st->mat[0], rows);
        st->n_live = 1;
    } else if (st->phase == GM_PHASE_FRESH) {
        const int p = st->p;
        const int32_t vl = gm_add_param_offset(p, st->mat[p], -st->step), vr = gm_add_param_offset(p, st->mat[p], st->step);
        gm_write_cand(st, cands, 0, vl, rows);
        gm_write_cand(st, cands, 1, vr, rows);
        for (int side = 0; side < 2; side++) {
            int32_t v = side ? vr : vl, r[2] = {rows[0], rows[1]};
            for (int t = 0; t < GM_K; t++) {
                v = gm_add_param_offset(p, v, side ? st->step : -st->step);
                gm_write_cand(st, cands, 2 + side * GM_K + t, v, r);
            }
        }
        st->n_live = GM_NC;
    } else {
        int32_t v = st->best_param;
        for (int t = 0; t < GM_NC; t++) {
            v = gm_add_param_offset(st->p, v, st->step * st->dir);
            gm_write_cand(st, cands, t, v, rows);
        }
        st->n_live = GM_NC;
    }
}

// the reference evaluates candidate c: count it, leave the rows it leaves, return its error
GM_HD int64_t gm_consume(GmState* st, const int64_t* err, int c) {
    st->probes++;
    if (!st->cand_valid[c]) st->invalid++;
    if (st->wmtype == 2) { st->mat[4] = st->cand_rows[c][0]; st->mat[5] = st->cand_rows[c][1]; }
    return err[c];
}

GM_HD void gm_next_param(GmState* st) {
    st->phase = GM_PHASE_FRESH;
    if (++st->p >= st->n_params) {
        st->p = 0;
        st->step >>= 1;
        if (++st->i >= st->n_ref) st->done = 1;
    }
}

// directional run over candidates first .. first + n - 1 (strict <, stop at the first that is not better)
GM_HD void gm_replay_run(GmState* st, const int64_t* err, int first, int n) {
    for (int t = 0; t < n; t++) {
        const int64_t e = gm_consume(st, err, first + t);
        if (e < st->best) {
            st->best = e;
            st->best_param = st->cand_val[first + t];
        } else {
            st->dir = 0;
            break;
        }
    }
    st->mat[st->p] = st->best_param;
    if (st->dir) st->phase = GM_PHASE_RUN;   // every speculated step was accepted: the run goes on in the next round
    else gm_next_param(st);
}

GM_HD void gm_finish(GmState* st, SvtHipGmResult* out) {
    gm_force_wmtype(st->mat, st->wmtype);
    for (int k = 0; k < 8; k++) out->wmmat[k] = st->mat[k];
    out->wmtype = gm_get_wmtype(st->mat);
    out->probes = st->probes;
    out->best_error = st->best;
    out->rounds = st->rounds;
    out->invalid_probes = st->invalid;
    st->done = 1;
    st->n_live = 0;
}

// First call of a job: validates it, forces the type and writes the one-candidate batch of the initial error.  ref_ok = the job's reference index names a plane.
GM_HD void gm_job_start(GmState* st, const SvtHipGmJob* job, int ref_ok, SvtHipGmModel* cands, SvtHipGmResult* out) {
    st->probes = st->rounds = st->invalid = st->done = st->n_live = 0;
    st->i = st->p = st->dir = st->best_param = 0;
    if (!ref_ok || job->wmtype < 0 || job->wmtype > 3 || job->n_refinements < 0 || job->n_refinements > SVT_HIP_GM_MAX_REFINEMENTS) {
        for (int k = 0; k < 8; k++) out->wmmat[k] = job->wmmat[k];
        out->wmtype = -1; out->probes = 0; out->best_error = -1; out->rounds = 0; out->invalid_probes = 0;
        st->done = 1;
        return;
    }
    for (int k = 0; k < 8; k++) st->mat[k] = job->wmmat[k];
    st->wmtype = job->wmtype;
    st->n_ref = job->n_refinements;
    st->n_params = 2 * job->wmtype;   // max_trans_model_params = {0, 2, 4, 6}
    st->best_frame_error = job->best_frame_error;
    st->step = st->n_ref > 0 ? 1 << (st->n_ref - 1) : 0;
    gm_force_wmtype(st->mat, st->wmtype);
    st->phase = GM_PHASE_INIT;
    gm_write_batch(st, cands);
}

// One round: err[c] = the warp error of candidate c of the batch written last; replays the reference's comparisons, then writes the next batch or the result.
GM_HD void gm_job_step(GmState* st, const int64_t* err, SvtHipGmModel* cands, SvtHipGmResult* out) {
    if (st->done) return;
    st->rounds++;
    if (st->phase == GM_PHASE_INIT) {
        const int64_t e = gm_consume(st, err, 0);
        st->best = e < st->best_frame_error ? e : st->best_frame_error;
        st->phase = GM_PHASE_FRESH;
        if (!st->n_params || !st->n_ref) st->done = 1;
    } else if (st->phase == GM_PHASE_FRESH) {
        st->best_param = st->mat[st->p];
        st->dir = 0;
        int64_t e = gm_consume(st, err, 0);
        if (e < st->best) { st->best = e; st->best_param = st->cand_val[0]; st->dir = -1; }
        e = gm_consume(st, err, 1);
        if (e < st->best) { st->best = e; st->best_param = st->cand_val[1]; st->dir = 1; }
        st->mat[st->p] = st->best_param;
        if (st->dir) gm_replay_run(st, err, st->dir < 0 ? 2 : 2 + GM_K, GM_K);
        else gm_next_param(st);
    } else {
        gm_replay_run(st, err, 0, GM_NC);
    }
    if (st->done) gm_finish(st, out);
    else gm_write_batch(st, cands);
}
