// Host build of svt-av1_amd/csrc/gm_walk.h (the refinement's state machine, the same text the device compiles) for tests/test_gm_walk_host.py: the walk is driven
// round by round with a callback that returns a candidate's warp error, so the reference's own svt_av1_warp_error can stand in for the device's error kernel.
// The callback also receives rows 4-5 of the carried struct as the reference would hold them when it evaluates the candidate (the order of evaluation: left,
// right, then one of the two runs), so the test can hand the reference exactly that struct and compare the shear parameters the state machine wrote.
#include "../svt-av1_amd/csrc/gm_walk.h"

typedef int64_t (*gm_probe_fn)(void* user, const SvtHipGmModel* model, const int32_t pre_rows[2], int wmtype);

extern "C" int gm_walk_host_k(void) { return GM_K; }

extern "C" void gm_shear_params_host(const int32_t* wmmat, int n, SvtHipGmModel* out) {
    for (int i = 0; i < n; i++) {
        gm_shear_params(wmmat + 6 * i, out + i);
        for (int k = 0; k < 6; k++) out[i].mat[k] = wmmat[6 * i + k];
    }
}

extern "C" int gm_walk_host(const SvtHipGmJob* job, gm_probe_fn probe, void* user, SvtHipGmResult* out, int* evaluated) {
    GmState st;
    SvtHipGmModel cands[GM_NC];
    int64_t err[GM_NC];
    int n_eval = 0;
    gm_job_start(&st, job, 1, cands, out);
    while (!st.done) {
        for (int c = 0; c < st.n_live; c++) {
            int prev = c - 1;                                                      // the candidate evaluated just before c
            if (st.phase == GM_PHASE_FRESH && c == 2 + GM_K) prev = 1;             // the right run follows left, right
            const int32_t* pre = prev < 0 ? st.mat + 4 : st.cand_rows[prev];
            err[c] = probe(user, cands + c, pre, st.wmtype);
            n_eval++;
        }
        gm_job_step(&st, err, cands, out);
        if (st.rounds > 100000) return -1;
    }
    if (evaluated) *evaluated = n_eval;
    return 0;
}
