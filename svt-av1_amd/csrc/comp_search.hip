// comp_search.hip — the mask decisions of compound mode decision for a list of blocks on gfx950 (wave64), behind svt_hip_compound_search_batch_dev: the inter-inter
// wedge (index and sign), the diff-weighted mask type, and the inter-intra mode with its wedge.
//
// Replaces (file:line under Source/Lib of the reference):
//   Encoder/Codec/EbEncInterPrediction.c:562-631, :6120-6162   pick_wedge with the residual1 / diff10 set-up of calc_pred_masked_compound
//   Encoder/Codec/EbEncInterPrediction.c:700-756               pick_interinter_seg
//   Encoder/Codec/EbModeDecision.c:387-475, :214-242           the decision part of inter_intra_search, pick_interintra_wedge
//   Encoder/Codec/EbEncInterPrediction.c:635-675               pick_wedge_fixed_sign
//   Encoder/Codec/EbEncInterPrediction.c:432-503, :819-869     model_rd_with_curvfit, model_rd_for_sb_with_curvfit (luma)
// The arithmetic is comp_search.h, the same text the host form runs serially.  Here:
//   comp_search_kernel   one workgroup of four waves per job, one launch for a mixed list.  The wedge kinds stage residual1, diff10 and (kind 0) ds in LDS once
//                        as int16 (6 KB at 32x32); wave w then takes the wedge indices w, w + 4, w + 8, w + 12, its lanes striding over the block four samples at a
//                        time: one 8-byte LDS read per array and one 4-byte read of the mask table (100 KB, cache-resident) per lane and step.  The diff-weighted
//                        kind keeps nothing: every thread strides over the block and holds two running sums, whatever the size.  Sums are reduced with the 64-bit
//                        forms of lane_reduce.h and joined across the four waves through LDS; sixteen lanes then run the model, and one thread takes the first
//                        minimum.  No atomics, and no value leaves the workgroup before the result.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "fmt_dispatch.h"
#include "lane_reduce.h"
#include "comp_search.h"

namespace {

#define PD __device__ __forceinline__

constexpr int WG = 256, WAVES = WG / 64, MAX_SUMS = 4;

// the totals of v[0 .. K) over the workgroup, in every thread.  Every thread of the workgroup calls it
template <int K> PD void block_sums(unsigned long long (&v)[K], unsigned long long (*s_part)[WAVES], int tid) {
    static_assert(K <= MAX_SUMS, "s_part holds MAX_SUMS rows");
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = wave_sum_u64(v[k]);
        if ((tid & 63) == 0) s_part[k][tid >> 6] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = s_part[k][0] + s_part[k][1] + s_part[k][2] + s_part[k][3];
    __syncthreads();   // s_part may be written again
}

PD int lo16(uint32_t v) { return (int16_t)(v & 0xFFFF); }
PD int hi16(uint32_t v) { return (int16_t)(v >> 16); }

// The wedge indices wave, wave + 4, ... of one block: the sign (PICK_SIGN: the dot product of ds with the sign-0 mask against the limit; else 0), then
// svt_av1_wedge_sse_from_residuals with the mask of that sign.  n is a multiple of 64, so a lane's four samples are all inside the block or all outside.
// Value ranges: |ds| <= 2^15 and a mask value <= 64, so a term of the dot product is below 2^21 and the at most 16 terms of a lane (n <= 1024, 64 lanes, 4 a step)
// stay below 2^25: a 32-bit lane sum, widened for the wave sum.  A term of the sse is a clamped int16 squared, at most 2^30 (reached: -32768^2): two of them fit 32
// bits, four do not, so a step adds two 32-bit pair sums to a 64-bit lane sum.
template <bool PICK_SIGN>
PD void wedge_scan(const int16_t* s_r1, const int16_t* s_d10, const int16_t* s_ds, const uint8_t* __restrict__ masks, int bsize, int n, long long limit, int tid, int* s_sign,
                   unsigned long long* s_sse) {
    const int lane = tid & 63, wave = tid >> 6;
    for (int w = wave; w < cs::WEDGE_TYPES; w += WAVES) {
        int sign = 0;
        if (PICK_SIGN) {
            const uint8_t* m = masks + cs::wedge_offset(bsize, 0, w);
            int            acc = 0;
            for (int k = lane * 4; k < n; k += 256) {
                const uint32_t m4 = *(const uint32_t*)(m + k);
                const uint2    d4 = *(const uint2*)(s_ds + k);
                acc += lo16(d4.x) * (int)(m4 & 255) + hi16(d4.x) * (int)((m4 >> 8) & 255) + lo16(d4.y) * (int)((m4 >> 16) & 255) + hi16(d4.y) * (int)(m4 >> 24);
            }
            sign = wave_sum_i64((long long)acc) > limit;
        }
        const uint8_t*     m = masks + cs::wedge_offset(bsize, sign, w);
        unsigned long long csse = 0;
        for (int k = lane * 4; k < n; k += 256) {
            const uint32_t m4 = *(const uint32_t*)(m + k);
            const uint2    r4 = *(const uint2*)(s_r1 + k), d4 = *(const uint2*)(s_d10 + k);
            const uint32_t a = cs::wedge_sse_term(lo16(r4.x), lo16(d4.x), (int)(m4 & 255)) + cs::wedge_sse_term(hi16(r4.x), hi16(d4.x), (int)((m4 >> 8) & 255));
            const uint32_t b = cs::wedge_sse_term(lo16(r4.y), lo16(d4.y), (int)((m4 >> 16) & 255)) + cs::wedge_sse_term(hi16(r4.y), hi16(d4.y), (int)(m4 >> 24));
            csse += (unsigned long long)a + b;
        }
        csse = wave_sum_u64(csse);
        if (lane == 0) {
            s_sign[w] = sign;
            s_sse[w] = cs::wedge_sse_round(csse);
        }
    }
}

template <class PIX, int BD>
__global__ __launch_bounds__(WG) void comp_search_kernel(const PIX* __restrict__ src, int stride, const PIX* __restrict__ pred, const int32_t* __restrict__ rates,
                                                         const uint8_t* __restrict__ masks, cs::RdTables T, const cs::Job* __restrict__ jobs,
                                                         cs::Result* __restrict__ results, cs::Cand* __restrict__ cands) {
    __shared__ __attribute__((aligned(16))) int16_t s_r1[cs::MAX_WEDGE_N], s_d10[cs::MAX_WEDGE_N], s_ds[cs::MAX_WEDGE_N];
    __shared__ unsigned long long                   s_part[MAX_SUMS][WAVES], s_sse[cs::WEDGE_TYPES];
    __shared__ int                                  s_sign[cs::WEDGE_TYPES];
    __shared__ cs::Cand                             s_cand[cs::MAX_CANDS];
    const int     tid = threadIdx.x, job = blockIdx.x;
    const cs::Job J = jobs[job];   // the same for every thread; the host has checked it (cs::job_ok)
    const int     bw = cs::block_w(J.bsize), bw_log2 = 31 - __clz(bw), n = bw * cs::block_h(J.bsize);
    const PIX*    s = src + (size_t)J.y * stride + J.x;
    const PIX*    p1 = pred + J.pred1;
    auto          at = [&](int k) { return (int)s[(size_t)(k >> bw_log2) * stride + (k & (bw - 1))]; };
    if (tid < cs::MAX_CANDS) s_cand[tid] = cs::no_candidate();
    cs::Result R = cs::empty_result();
    __syncthreads();

    if (J.kind == cs::KIND_DIFFWTD) {
        // a thread sees at most 64 samples (128x128): two 64-bit sums of terms below 2^30
        const PIX*         p0 = pred + J.pred0;
        unsigned long long csse[2] = {0, 0};
        for (int k = tid; k < n; k += WG) {
            const int a = p0[k], b = p1[k], r1 = at(k) - b, d = b - a, m = cs::diffwtd_38(a, b, BD);
            csse[0] += cs::wedge_sse_term(r1, d, m);
            csse[1] += cs::wedge_sse_term(r1, d, 64 - m);
        }
        block_sums<2>(csse, s_part, tid);
        if (tid < 2) s_cand[tid] = cs::candidate(T, J, n, 0, (int64_t)cs::wedge_sse_round(csse[tid]), 0);
        __syncthreads();
        R.mask_type = cs::first_min(s_cand, 2, &R.rd);
    } else if (J.kind == cs::KIND_WEDGE) {
        // a thread sees at most 4 samples (32x32) and a squared residual is below 2^20
        const PIX*         p0 = pred + J.pred0;
        unsigned long long ss[2] = {0, 0};
        for (int k = tid; k < n; k += WG) {
            const int v = at(k), r0 = v - p0[k], r1 = v - p1[k];
            s_r1[k] = (int16_t)r1;
            s_d10[k] = (int16_t)((int)p1[k] - (int)p0[k]);
            s_ds[k] = (int16_t)cs::delta_square(r0, r1);
            ss[0] += (uint32_t)(r0 * r0);
            ss[1] += (uint32_t)(r1 * r1);
        }
        block_sums<2>(ss, s_part, tid);   // its barriers also publish the staged arrays
        wedge_scan<true>(s_r1, s_d10, s_ds, masks, J.bsize, n, cs::sign_limit(ss[0], ss[1]), tid, s_sign, s_sse);
        __syncthreads();
        if (tid < cs::WEDGE_TYPES) s_cand[tid] = cs::candidate(T, J, n, s_sign[tid], (int64_t)s_sse[tid], 0);
        __syncthreads();
        R.wedge_index = cs::first_min(s_cand, cs::WEDGE_TYPES, &R.rd);
        R.wedge_sign = R.wedge_index < 0 ? -1 : s_cand[R.wedge_index].sign;
    } else {
        // the four smooth blends: a thread sees at most 4 samples a mode, a squared difference is below 2^20
        const PIX*         intra = pred + J.pred0;
        const int          scale = cs::ii_size_scale(J.bsize);
        unsigned long long sse[cs::II_MODES] = {0, 0, 0, 0};
        for (int k = tid; k < n; k += WG) {
            const int v = at(k), inter = p1[k], y = k >> bw_log2, x = k & (bw - 1);
#pragma unroll
            for (int mode = 0; mode < cs::II_MODES; ++mode) {
                const int diff = v - cs::blend_a64(cs::ii_smooth_mask(mode, scale, y, x), intra[mode * n + k], inter);
                sse[mode] += (uint32_t)(diff * diff);
            }
        }
        block_sums<cs::II_MODES>(sse, s_part, tid);
        if (tid < cs::II_MODES) s_cand[tid] = cs::candidate(T, J, n, 0, (int64_t)sse[tid], rates[J.mode_rate + tid]);
        __syncthreads();
        R.interintra_mode = cs::first_min(s_cand, cs::II_MODES, &R.rd);   // the same in every thread
        if (R.interintra_mode >= 0) {
            const PIX* p0 = intra + R.interintra_mode * n;
            for (int k = tid; k < n; k += WG) {
                s_r1[k] = (int16_t)(at(k) - (int)p1[k]);
                s_d10[k] = (int16_t)((int)p1[k] - (int)p0[k]);
            }
            __syncthreads();
            wedge_scan<false>(s_r1, s_d10, s_ds, masks, J.bsize, n, 0, tid, s_sign, s_sse);
            __syncthreads();
            if (tid < cs::WEDGE_TYPES) s_cand[cs::II_MODES + tid] = cs::candidate(T, J, n, 0, (int64_t)s_sse[tid], rates[J.wedge_rate + tid]);
            __syncthreads();
            R.interintra_wedge_index = cs::first_min(s_cand + cs::II_MODES, cs::WEDGE_TYPES, &R.rd_wedge);
        }
    }
    if (tid == 0) results[job] = R;
    if (cands && tid < cs::MAX_CANDS) cands[(size_t)job * cs::MAX_CANDS + tid] = s_cand[tid];
}

}  // namespace

int svt_hip_launch_compound_search(hipStream_t st, int pix_bytes, int bd, const void* src, int stride, const void* pred, const int32_t* rates, const uint8_t* masks,
                                   const double* rate_grid, const double* dist_grid, const int32_t* bsize_cat, const SvtHipCompSearchJob* jobs, int njobs,
                                   SvtHipCompSearchResult* results, SvtHipCompSearchCand* cands) {
    const cs::RdTables T{rate_grid, dist_grid, bsize_cat};
    svt_for_fmt(pix_bytes, bd, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL((comp_search_kernel<PIX, decltype(f)::bd>), dim3(njobs), dim3(WG), 0, st, (const PIX*)src, stride, (const PIX*)pred, rates, masks, T, jobs, results,
                           cands);
    });
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(comp_search)
