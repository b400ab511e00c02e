// Host build of svt-av1_amd/csrc/gm_fit.h (the model fit's arithmetic, the same text the device compiles) for tests/test_gm_fit_host.py: the pieces are put
// together serially, in the order the device's workgroup runs them, so the reference's fit functions can be compared bit for bit without a device.  Also the
// literal walk of get_rand_indices next to its arithmetic form.  Build with -ffp-contract=off, as the library is.
//
// With GM_FIT_HOST_MAIN defined the file is a stand-alone program (for a sanitizer run on the CPU): it fits a few generated lists and prints the results.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../svt-av1_amd/csrc/gm_fit.h"

// ransac() over one list: corr[n][4].  inliers (may be NULL) receives the kept motion's indices.
extern "C" void gm_fit_host(int type, const int32_t* corr, int n, int n_refinements, int ref, SvtHipGmFit* fit, int32_t* inliers, SvtHipGmJob* job) {
    memset(fit, 0, sizeof(*fit));
    fit->npoints = n;
    gm_fit_identity(fit->params);
    uint16_t idx[GM_FIT_TRIALS][4];
    int fail = n < GM_FIT_MIN_POINTS ? 1 : gm_fit_draw_trials(type, corr, n, idx);
    int num = 0;
    if (!fail) {
        int ok[GM_FIT_TRIALS], cnt[GM_FIT_TRIALS];
        double var[GM_FIT_TRIALS], params[GM_FIT_TRIALS][8], work[GM_FIT_WORK];
        GmFitNorm nm[2];
        std::vector<double> dist((size_t)n * GM_FIT_TRIALS);
        for (int t = 0; t < GM_FIT_TRIALS; t++) {
            ok[t] = !gm_fit_find(type, corr, idx[t], GM_FIT_MINPTS, nm, work, params[t]);
            int c = 0;
            double sum_distance = 0.0, sum_distance_squared = 0.0;
            for (int i = 0; i < n; i++) {
                const double distance = ok[t] ? gm_fit_distance(type, params[t], corr + 4 * i) : 2 * GM_FIT_INLIER_THRESHOLD;
                dist[(size_t)i * GM_FIT_TRIALS + t] = distance;
                if (distance < GM_FIT_INLIER_THRESHOLD) {
                    c++;
                    sum_distance += distance;
                    sum_distance_squared += distance * distance;
                }
            }
            cnt[t] = c;
            var[t] = c > 1 ? gm_fit_variance(c, sum_distance, sum_distance_squared) : 0.0;
        }
        const int best = gm_fit_select(ok, cnt, var, &num);
        std::vector<uint16_t> inl;
        if (best >= 0)
            for (int i = 0; i < n; i++)
                if (dist[(size_t)i * GM_FIT_TRIALS + best] < GM_FIT_INLIER_THRESHOLD) {
                    if (inliers) inliers[inl.size()] = i;
                    inl.push_back((uint16_t)i);
                }
        if (num >= GM_FIT_MINPTS) (void)gm_fit_find(type, corr, inl.data(), num, nm, work, fit->params);
    }
    fit->ret = fail;
    fit->num_inliers = fail ? 0 : num;
    gm_fit_finish(fit, ref, n_refinements, job);
}

extern "C" void gm_fit_convert_host(const double* params, int32_t* wmmat, int32_t* wmtype) {
    gm_fit_convert(params, wmmat);
    *wmtype = gm_get_wmtype(wmmat);
}

// get_rand_indices (Encoder/Codec/ransac.c:292-314) with its walk as the loop it is, minpts = 3
static int rand_indices_loop(int npoints, uint32_t* seed, int* indices) {
    const int minpts = GM_FIT_MINPTS;
    int i, j;
    int ptr = (int)(gm_fit_rand16(seed) % (uint32_t)npoints);
    if (minpts > npoints) return 0;
    indices[0] = ptr;
    ptr = (ptr == npoints - 1 ? 0 : ptr + 1);
    i = 1;
    while (i < minpts) {
        int index = (int)(gm_fit_rand16(seed) % (uint32_t)npoints);
        while (index) {
            ptr = (ptr == npoints - 1 ? 0 : ptr + 1);
            for (j = 0; j < i; ++j)
                if (indices[j] == ptr) break;
            if (j == i) index--;
        }
        indices[i++] = ptr;
    }
    return 1;
}

// `draws` consecutive draws from `seed` with both forms: the number of draws whose triple, return value or seed afterwards differ (0 = the forms agree);
// *zero_draws counts the draws in which the second or third index was drawn as 0 (so the test can see that they occurred).
extern "C" int gm_fit_rand_indices_compare(int npoints, uint32_t seed, int draws, int* zero_draws) {
    uint32_t sa = seed, sb = seed;
    int wrong = 0;
    for (int d = 0; d < draws; d++) {
        uint32_t probe = sa;
        (void)gm_fit_rand16(&probe);
        const int z1 = gm_fit_rand16(&probe) % (uint32_t)npoints == 0, z2 = gm_fit_rand16(&probe) % (uint32_t)npoints == 0;
        if (zero_draws && npoints >= GM_FIT_MINPTS && (z1 || z2)) ++*zero_draws;
        int a[3] = {-1, -1, -1}, b[3] = {-1, -1, -1};
        const int ra = rand_indices_loop(npoints, &sa, a);
        const int rb = gm_fit_rand_indices(npoints, &sb, &b[0], &b[1], &b[2]);
        wrong += ra != rb || sa != sb || a[0] != b[0] || a[1] != b[1] || a[2] != b[2];
    }
    return wrong;
}

#ifdef GM_FIT_HOST_MAIN
#include <stdio.h>
int main() {
    uint32_t s = 12345;
    for (int n : {0, 14, 15, 40, 300, 4096}) {
        std::vector<int32_t> corr((size_t)n * 4 + 4);
        for (int i = 0; i < n; i++) {
            const int x = (int)(gm_fit_rand16(&s) % 352), y = (int)(gm_fit_rand16(&s) % 288);
            const int out = gm_fit_rand16(&s) % 4 == 0;
            corr[4 * i] = x; corr[4 * i + 1] = y;
            corr[4 * i + 2] = out ? (int)(gm_fit_rand16(&s) % 352) : (int)(1.01 * x + 0.02 * y + 3.0 + 0.5);
            corr[4 * i + 3] = out ? (int)(gm_fit_rand16(&s) % 288) : (int)(-0.02 * x + 1.01 * y - 2.0 + 0.5);
        }
        std::vector<int32_t> inl((size_t)n + 1);
        for (int type = 1; type <= 3; type++) {
            SvtHipGmFit fit;
            SvtHipGmJob job;
            gm_fit_host(type, corr.data(), n, 5, 0, &fit, inl.data(), &job);
            printf("n %d type %d: ret %d inliers %d kept %d wmtype %d job %d params %.17g %.17g %.17g %.17g\n", n, type, fit.ret, fit.num_inliers, fit.num_inliers_kept,
                   fit.wmtype, job.wmtype, fit.params[0], fit.params[1], fit.params[2], fit.params[3]);
        }
    }
    int zeros = 0, wrong = 0;
    for (int n = 1; n <= 64; n++) wrong += gm_fit_rand_indices_compare(n, (uint32_t)n * 7919u, 2000, &zeros);
    printf("rand indices: %d wrong, %d zero draws\n", wrong, zeros);
    return wrong != 0;
}
#endif
