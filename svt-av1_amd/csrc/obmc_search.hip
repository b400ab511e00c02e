// obmc_search.hip — OBMC in mode decision for a list of blocks on gfx950 (wave64): the weighted target behind svt_hip_obmc_target_batch_dev and the motion
// refinement against it behind svt_hip_obmc_search_batch_dev.  8-bit, as the reference's mode decision.
//
// Replaces (file:line under Source/Lib of the reference):
//   Encoder/Codec/EbEncInterPrediction.c:2376-2437, :2196-2256   calc_target_weighted_pred with its two visitors
//   Encoder/Codec/EbModeDecision.c:2951-3036                     single_motion_search
//   Encoder/Codec/av1me.c:836-855, :791-834, :776-790            svt_av1_obmc_full_pixel_search, obmc_refining_search_sad, get_obmc_mvpred_var
//   Encoder/Codec/av1me.c:1069-1254, :973-1035                   svt_av1_find_best_obmc_sub_pixel_tree_up, upsampled_obmc_pref_error
//   Encoder/C_DEFAULT/variance.c:212-299, sad_av1.c:18-38        svt_aom_upsampled_pred_c, svt_aom_obmc_variance{W}x{H}_c, svt_aom_obmc_sad{W}x{H}_c
// The arithmetic and both walks are obmc_search.h, the same text the host forms run serially.  Here:
//   obmc_target_kernel   one workgroup per job; a sample's wsrc / mask depend on its position alone (obmc_search.h), so the 256 threads stride over the block and
//                        write two int32 each: 1 + at most 2 bytes read and 8 written per sample, no LDS.
//   obmc_search_kernel   one workgroup of four waves per job.  Every thread runs the two walks with the same values; a step hands the evaluator its up to four
//                        probes (four refinement sites, four axis probes, two second-level probes) at once.  Blocks of at most 1024 samples take a wave per
//                        probe, so a step's probes run side by side; larger blocks put the whole workgroup on one probe after the other.  A 2-D sub-pel probe keeps
//                        svt_aom_upsampled_pred's 8-bit intermediate (rows -3 .. bh + 3) in LDS, a slice per wave or one of (128 + 7) * 128 bytes; the 1-D and
//                        whole-sample probes read the plane directly.  The job's wsrc (int32) and mask (16 bits: at most 4096) are staged in LDS once for blocks
//                        up to 64x64 (24 KB) and re-read there on every probe; the 128-wide shapes read them from global memory.  The reference window is not
//                        staged: a probe's samples come through the caches (docs/kernels/obmc.md has what that costs).  Sums are taken with lane_reduce.h and
//                        joined across waves through LDS; the winner of a step is chosen by the serial code of obmc_search.h on those sums.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "lane_reduce.h"
#include "obmc_search.h"

namespace {

#define PD __device__ __forceinline__

constexpr int WG = 256, WAVES = WG / 64;
constexpr int LDS_SAMPLES = 64 * 64;               // wsrc / mask staged up to this block area
constexpr int WAVE_SAMPLES = 1024;                 // a wave per probe up to this block area
constexpr int IM_BYTES = (128 + 7) * 128;          // the intermediate of a 128x128 probe
constexpr int IM_WAVE_BYTES = IM_BYTES / WAVES;    // a wave's slice: (32 + 7) * 32 = 1248 fits
static_assert(IM_WAVE_BYTES >= (32 + 7) * 32 && IM_WAVE_BYTES % 4 == 0, "a wave's intermediate slice");

__global__ __launch_bounds__(WG) void obmc_target_kernel(const uint8_t* __restrict__ src, int stride, const uint8_t* __restrict__ nbr, const obmc::TargetJob* __restrict__ jobs,
                                                         int32_t* __restrict__ wsrc, int32_t* __restrict__ mask) {
    const obmc::TargetJob J = jobs[blockIdx.x];   // the host has checked it (obmc::target_job_ok)
    const int             bw = obmc::block_w(J.bsize), bh = obmc::block_h(J.bsize), bw_log2 = 31 - __clz(bw), n = bw * bh;
    const uint8_t*        s = src + (size_t)J.y * stride + J.x;
    for (int k = threadIdx.x; k < n; k += WG) {
        const int r = k >> bw_log2, c = k & (bw - 1);
        int32_t   w, m;
        obmc::target_sample(J, bw, bh, r, c, s[(size_t)r * stride + c], nbr, &w, &m);
        wsrc[(size_t)J.wm_off + k] = w;
        mask[(size_t)J.wm_off + k] = m;
    }
}

// The evaluator of obmc_search.h on a workgroup.  Every thread calls every method with the same arguments and gets the same results.
template <bool IN_LDS> struct DevEv {
    const uint8_t* y;   // the block's position in the reference plane
    int            stride, bw, bh, bw_log2, n, tid;
    const int32_t *g_wsrc, *g_mask;
    const int32_t*  s_wsrc;
    const uint16_t* s_mask;
    uint8_t*        s_im;
    uint32_t (*s_acc)[WAVES][2];   // [probe][wave] {sse or sad, sum}

    PD int wsrc_at(int k) const { return IN_LDS ? s_wsrc[k] : g_wsrc[k]; }
    PD int mask_at(int k) const { return IN_LDS ? (int)s_mask[k] : g_mask[k]; }

    // one probe over the threads first, first + step, ...; im = its intermediate.  SAD: whole samples, the sad; else 1/8 sample, the sse and the sum
    template <bool SAD> PD void accumulate(int row, int col, int first, int step, const uint8_t* im, uint32_t* a, uint32_t* b) const {
        const int      sx = SAD ? 0 : col & 7, sy = SAD ? 0 : row & 7;
        const uint8_t* pre = SAD ? y + (ptrdiff_t)row * stride + col : y + (ptrdiff_t)(row >> 3) * stride + (col >> 3);
        uint32_t       acc = 0;
        int            sum = 0;
        for (int k = first; k < n; k += step) {
            const int      r = k >> bw_log2, c = k & (bw - 1);
            const uint8_t* q = pre + (ptrdiff_t)r * stride + c;
            int            v;
            if (sx && sy) v = obmc::filter8(im + (r + obmc::FILTER_REACH_LO) * bw + c, bw, sy);
            else if (sx) v = obmc::filter8(q, 1, sx);
            else if (sy) v = obmc::filter8(q, stride, sy);
            else v = *q;
            if (SAD) {
                acc += obmc::sad_term(wsrc_at(k), mask_at(k), v);
            } else {
                const int d = obmc::var_diff(wsrc_at(k), mask_at(k), v);
                sum += d;
                acc += (uint32_t)(d * d);
            }
        }
        *a = wave_sum_u32(acc);
        *b = wave_sum_u32((uint32_t)sum);
    }
    // the horizontal pass of a 2-D probe: rows -3 .. bh + 3 of the block, rounded and clipped to 8 bits
    PD void intermediate(int row, int col, int first, int step, uint8_t* im) const {
        const int sx = col & 7;
        if (!sx || !(row & 7)) return;
        const uint8_t* pre = y + (ptrdiff_t)(row >> 3) * stride + (col >> 3);
        for (int k = first; k < (bh + 7) * bw; k += step) {
            const int r = k >> bw_log2, c = k & (bw - 1);
            im[k] = (uint8_t)obmc::filter8(pre + (ptrdiff_t)(r - obmc::FILTER_REACH_LO) * stride + c, 1, sx);
        }
    }
    template <bool SAD> PD void eval(const int* rows, const int* cols, int np, unsigned live, uint32_t* out_a, uint32_t* out_b) const {
        const int lane = tid & 63, wave = tid >> 6;
        if (tid < 4 * WAVES * 2) (&s_acc[0][0][0])[tid] = 0;
        __syncthreads();
        if (n <= WAVE_SAMPLES) {   // a wave per probe; the barrier between the passes is the same for every wave
            const bool mine = wave < np && (live >> wave & 1);
            uint8_t*   im = s_im + wave * IM_WAVE_BYTES;
            if (!SAD && mine) intermediate(rows[wave], cols[wave], lane, 64, im);
            if (!SAD) __syncthreads();
            if (mine) {
                uint32_t a, b;
                accumulate<SAD>(rows[wave], cols[wave], lane, 64, im, &a, &b);
                if (lane == 0) {
                    s_acc[wave][0][0] = a;
                    s_acc[wave][0][1] = b;
                }
            }
        } else {   // the workgroup on one probe after the other; np and live are the same in every thread
            for (int p = 0; p < np; ++p) {
                if (!(live >> p & 1)) continue;
                if (!SAD) {
                    __syncthreads();   // the previous probe's intermediate has been read
                    intermediate(rows[p], cols[p], tid, WG, s_im);
                    __syncthreads();
                }
                uint32_t a, b;
                accumulate<SAD>(rows[p], cols[p], tid, WG, s_im, &a, &b);
                if (lane == 0) {
                    s_acc[p][wave][0] = a;
                    s_acc[p][wave][1] = b;
                }
            }
        }
        __syncthreads();
        for (int p = 0; p < np; ++p) {
            out_a[p] = s_acc[p][0][0] + s_acc[p][1][0] + s_acc[p][2][0] + s_acc[p][3][0];
            out_b[p] = s_acc[p][0][1] + s_acc[p][1][1] + s_acc[p][2][1] + s_acc[p][3][1];
        }
        __syncthreads();   // s_acc is cleared by the next call
    }
    PD void sads(const int* rows, const int* cols, int np, unsigned live, uint32_t* out) const {
        uint32_t unused[4];
        eval<true>(rows, cols, np, live, out, unused);
    }
    PD void probes(const int* rows, const int* cols, int np, unsigned live, uint32_t* var, uint32_t* sse) const {
        uint32_t sum[4];
        eval<false>(rows, cols, np, live, sse, sum);
        for (int p = 0; p < np; ++p) var[p] = obmc::variance_of(sse[p], (int)sum[p], n);
    }
};

__global__ __launch_bounds__(WG) void obmc_search_kernel(obmc::Plane P, const int32_t* __restrict__ wsrc, const int32_t* __restrict__ mask, int64_t wm_samples,
                                                         const int32_t* __restrict__ jc, const int32_t* __restrict__ cc, const obmc::Job* __restrict__ jobs,
                                                         obmc::Result* __restrict__ results) {
    __shared__ int32_t                                 s_wsrc[LDS_SAMPLES];
    __shared__ uint16_t                                s_mask[LDS_SAMPLES];
    __shared__ __attribute__((aligned(16))) uint8_t    s_im[IM_BYTES];
    __shared__ uint32_t                                s_acc[4][WAVES][2];
    const int       tid = threadIdx.x, job = blockIdx.x;
    const obmc::Job J = jobs[job];   // the same for every thread; the host has checked it (obmc::job_status >= 0)
    const int       status = obmc::job_status(J, P, wm_samples);
    if (status != obmc::STATUS_SEARCHED) {   // the whole workgroup leaves
        if (tid == 0) results[job] = obmc::empty_result(status);
        return;
    }
    const int      bw = obmc::block_w(J.bsize), bh = obmc::block_h(J.bsize), n = bw * bh;
    const uint8_t* y = P.ref + (ptrdiff_t)J.mi_row * obmc::MI_SIZE * P.stride + J.mi_col * obmc::MI_SIZE;
    obmc::Result   R;
    if (n <= LDS_SAMPLES) {
        for (int k = tid; k < n; k += WG) {
            s_wsrc[k] = wsrc[(size_t)J.wm_off + k];
            s_mask[k] = (uint16_t)mask[(size_t)J.wm_off + k];
        }
        __syncthreads();
        const DevEv<true> ev{y, P.stride, bw, bh, 31 - __clz(bw), n, tid, nullptr, nullptr, s_wsrc, s_mask, s_im, s_acc};
        R = obmc::search_job(ev, J, P.mi_rows, P.mi_cols, jc, cc);
    } else {
        const DevEv<false> ev{y, P.stride, bw, bh, 31 - __clz(bw), n, tid, wsrc + J.wm_off, mask + J.wm_off, nullptr, nullptr, s_im, s_acc};
        R = obmc::search_job(ev, J, P.mi_rows, P.mi_cols, jc, cc);
    }
    if (tid == 0) results[job] = R;
}

}  // namespace

int svt_hip_launch_obmc_target(hipStream_t st, const uint8_t* src, int stride, const uint8_t* nbr, const SvtHipObmcTargetJob* jobs, int njobs, int32_t* wsrc, int32_t* mask) {
    hipLaunchKernelGGL(obmc_target_kernel, dim3(njobs), dim3(WG), 0, st, src, stride, nbr, jobs, wsrc, mask);
    return (int)hipGetLastError();
}

int svt_hip_launch_obmc_search(hipStream_t st, const uint8_t* ref, int stride, int width, int height, int pad_w, int pad_h, int mi_rows, int mi_cols, const int32_t* wsrc,
                               const int32_t* mask, int64_t wm_samples, const int32_t* joint_cost, const int32_t* comp_cost, const SvtHipObmcSearchJob* jobs, int njobs,
                               SvtHipObmcSearchResult* results) {
    const obmc::Plane P{ref, stride, width, height, pad_w, pad_h, mi_rows, mi_cols};
    hipLaunchKernelGGL(obmc_search_kernel, dim3(njobs), dim3(WG), 0, st, P, wsrc, mask, wm_samples, joint_cost, comp_cost, jobs, results);
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(obmc_search)
