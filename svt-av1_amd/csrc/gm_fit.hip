// gm_fit.hip — the global-motion model fit on the device: RANSAC over a correspondence list, the conversion of the kept model to integer parameters and the job the
// refinement reads; gfx950.  The arithmetic is gm_fit.h (also built for the host: tests/gm_fit_host.cpp); this file is only how it is spread over a workgroup.
// docs/kernels/gm.md "The fit".
//
// Replaces (file:line under the reference's Source/Lib): Encoder/Codec/ransac.c:359-542 ransac() with its three model types (:34-68 projections, :70-290 the fits,
// :292-314 get_rand_indices, :728-738 the degeneracy tests), Encoder/Codec/mathutils.h:26-111, Encoder/Codec/global_motion.c:41-86
// svt_av1_convert_model_to_params and :310-318 the MIN_INLIER_PROB rule.
//
// gm_ransac_kernel: one workgroup of 256 per job.  Every sum keeps the reference's order: work is split across trials and across independent accumulators, never
// inside one sum.
//   draws      lane 0: the 20 trials' index triples are one serial chain (the walk of get_rand_indices is arithmetic, gm_fit_advance)
//   fits       lanes 0..19: the three-point fit of a trial each, matrices in LDS
//   distances  all lanes: projection and distance per (point, trial) into the call's scratch, [point][trial]
//   sums       lanes 0..19: a trial's inlier count, sum_distance and sum_distance_squared, serially over the points; then its variance
//   selection  lane 0 replays the keep rule over the 20 (count, variance) pairs
//   inliers    wave 0: the kept trial's inlier list, an ordered compaction by ballot prefix
//   recompute  4 + 2 lanes for the ordered sums of the two normalisations, one lane per cell of the normal equations (2 / 14 / 27), lane 0 for the solve (LDS)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "gm_fit.h"

namespace {

struct GmFitJobTab { SvtHipGmFitJob j[SVT_HIP_GM_FIT_MAX_JOBS]; };

__global__ void __launch_bounds__(256)
gm_ransac_kernel(const int32_t* __restrict__ d_corr, const int32_t* __restrict__ d_ncorr, int max_points, GmFitJobTab tab, int n_refinements,
                 SvtHipGmFit* __restrict__ fits, int32_t* __restrict__ d_inliers, SvtHipGmJob* __restrict__ jobs_out, double* __restrict__ scratch) {
    __shared__ uint16_t s_idx[GM_FIT_TRIALS][4];
    __shared__ double s_work[GM_FIT_TRIALS][GM_FIT_WORK];
    __shared__ double s_params[GM_FIT_TRIALS][8];
    __shared__ GmFitNorm s_tnorm[GM_FIT_TRIALS][2];
    __shared__ int s_ok[GM_FIT_TRIALS], s_cnt[GM_FIT_TRIALS];
    __shared__ double s_var[GM_FIT_TRIALS];
    __shared__ uint16_t s_inl[SVT_HIP_GM_MAX_CORNERS];
    __shared__ double s_sums[4];
    __shared__ GmFitNorm s_norm[2];
    __shared__ int s_fail, s_best, s_num;
    __shared__ SvtHipGmFit s_fit;
    __shared__ SvtHipGmJob s_job;

    const int job = blockIdx.x, tid = threadIdx.x;
    const int ref = tab.j[job].ref, type = tab.j[job].type;
    const int32_t* __restrict__ corr = d_corr + (size_t)ref * max_points * 4;
    int n = d_ncorr[ref];
    n = n < 0 ? 0 : (n > max_points ? max_points : n);
    double* __restrict__ dist = scratch + (size_t)job * GM_FIT_TRIALS * max_points;   // [point][trial]

    if (tid == 0) {
        s_fit.ret = 0; s_fit.npoints = n; s_fit.num_inliers = 0;
        gm_fit_identity(s_fit.params);
        s_best = -1; s_num = 0;
        // npoints < minpts * MINPTS_MULTIPLIER || npoints == 0
        s_fail = n < GM_FIT_MIN_POINTS ? 1 : gm_fit_draw_trials(type, corr, n, s_idx);
    }
    __syncthreads();
    if (!s_fail) {   // uniform
        if (tid < GM_FIT_TRIALS) s_ok[tid] = !gm_fit_find(type, corr, s_idx[tid], GM_FIT_MINPTS, s_tnorm[tid], s_work[tid], s_params[tid]);
        __syncthreads();
        for (int i = tid; i < GM_FIT_TRIALS * n; i += 256) {
            const int t = i % GM_FIT_TRIALS;
            dist[i] = s_ok[t] ? gm_fit_distance(type, s_params[t], corr + 4 * (i / GM_FIT_TRIALS)) : 2 * GM_FIT_INLIER_THRESHOLD;
        }
        __syncthreads();
        if (tid < GM_FIT_TRIALS) {
            int cnt = 0;
            double sum_distance = 0.0, sum_distance_squared = 0.0;
            for (int i = 0; i < n; i++) {
                const double distance = dist[i * GM_FIT_TRIALS + tid];
                if (distance < GM_FIT_INLIER_THRESHOLD) {
                    cnt++;
                    sum_distance += distance;
                    sum_distance_squared += distance * distance;
                }
            }
            s_cnt[tid] = cnt;
            s_var[tid] = cnt > 1 ? gm_fit_variance(cnt, sum_distance, sum_distance_squared) : 0.0;
        }
        __syncthreads();
        if (tid == 0) s_best = gm_fit_select(s_ok, s_cnt, s_var, &s_num);
        __syncthreads();
        const int best = s_best, num = s_num;
        if (best >= 0 && tid < 64) {
            int32_t* out = d_inliers ? d_inliers + (size_t)job * max_points : nullptr;
            int off = 0;
            for (int base = 0; base < n; base += 64) {
                const int i = base + tid;
                const bool in = i < n && dist[i * GM_FIT_TRIALS + best] < GM_FIT_INLIER_THRESHOLD;
                const unsigned long long m = __ballot(in);
                if (in) {
                    const int pos = off + __popcll(m & ((1ull << tid) - 1));
                    s_inl[pos] = (uint16_t)i;
                    if (out) out[pos] = i;
                }
                off += __popcll(m);
            }
        }
        __syncthreads();
        if (num >= GM_FIT_MINPTS) {   // uniform: the motion is recomputed from its inliers
            if (tid < 4) s_sums[tid] = gm_fit_sum_coord(corr, s_inl, num, tid);
            __syncthreads();
            if (tid < 2) {
                s_norm[tid].mean0 = s_sums[2 * tid] / num;
                s_norm[tid].mean1 = s_sums[2 * tid + 1] / num;
                gm_fit_norm_scale(s_norm + tid, gm_fit_sum_msqe(corr, s_inl, num, tid, s_norm + tid), num);
            }
            __syncthreads();
            if (tid < gm_fit_cells(type)) gm_fit_cell(type, tid, corr, s_inl, num, s_norm, s_norm + 1, s_work[0]);
            __syncthreads();
            if (tid == 0) (void)gm_fit_solve(type, num, s_work[0], s_norm, s_norm + 1, s_fit.params);   // the reference ignores the return value here
        }
    }
    if (tid == 0) {
        s_fit.ret = s_fail;
        s_fit.num_inliers = s_fail ? 0 : s_num;
        gm_fit_finish(&s_fit, ref, n_refinements, jobs_out ? &s_job : nullptr);
    }
    __syncthreads();
    static_assert(sizeof(SvtHipGmFit) % 4 == 0 && sizeof(SvtHipGmJob) % 4 == 0, "copied as dwords");
    for (int k = tid; k < (int)(sizeof(SvtHipGmFit) / 4); k += 256) ((int*)(fits + job))[k] = ((const int*)&s_fit)[k];
    if (jobs_out)
        for (int k = tid; k < (int)(sizeof(SvtHipGmJob) / 4); k += 256) ((int*)(jobs_out + job))[k] = ((const int*)&s_job)[k];
}

}  // namespace

extern "C" size_t svt_hip_gm_fit_scratch_layout_bytes(int njobs, int max_points) {
    if (njobs < 0) njobs = 0;
    if (max_points < 0) max_points = 0;
    return (size_t)njobs * GM_FIT_TRIALS * (size_t)max_points * sizeof(double);
}

extern "C" int svt_hip_launch_gm_fit(hipStream_t st, const int32_t* corr, const int32_t* ncorr, int max_points, const SvtHipGmFitJob* jobs, int njobs, int n_refinements,
                                     SvtHipGmFit* fits, int32_t* inliers, SvtHipGmJob* refine_jobs, void* scratch) {
    if (njobs <= 0) return 0;
    GmFitJobTab tab = {};
    for (int i = 0; i < njobs && i < SVT_HIP_GM_FIT_MAX_JOBS; i++) tab.j[i] = jobs[i];
    hipLaunchKernelGGL(gm_ransac_kernel, dim3(njobs), dim3(256), 0, st, corr, ncorr, max_points, tab, n_refinements, fits, inliers, refine_jobs, (double*)scratch);
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(gm_fit)
