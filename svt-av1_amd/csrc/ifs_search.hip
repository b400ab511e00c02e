// ifs_search.hip — the dual interpolation filter search of mode decision for a list of blocks on gfx950 (wave64), behind svt_hip_ifs_search_batch_dev: nine luma
// predictions per block, one for each pair of vertical and horizontal filter, each followed by an SSE against the source, the Laplacian model and RDCOST, then the
// reference's decision walk.
//
// Replaces (file:line under Source/Lib of the reference):
//   Encoder/Codec/EbEncInterPrediction.c:3047-3297   interpolation_filter_search
//   Encoder/Codec/EbEncInterPrediction.c:2903-2996, :2877-2901, :2855-2875, :2795-2853   model_rd_for_sb (luma), model_rd_from_sse, svt_av1_model_rd_from_var_lapndz, model_rd_norm
//   Common/Codec/EbInterPrediction.c:349-469, :744-866, :552-741, :944-1143             the [highbd_]convolve_*_sr and [highbd_]jnt_convolve_* leaves the search predicts with
//   Common/Codec/EbPictureOperators.c   svt_spatial_full_distortion_kernel, svt_full_distortion_kernel16_bits
// The rounding of every branch, the model and both walks are ifs_search.h, the same text the host form runs serially.  Here:
//   ifs_search_kernel   one workgroup of four waves per job, one launch for a mixed list.  A block is walked in strips of rows.  Per strip and reference the window
//                       (rows + 7) x (bw + 7) is staged in LDS as int16; where both phases of a reference are non-zero the horizontal pass is made ONCE per x filter,
//                       three int16 intermediates of (rows + 7) x bw, and each is shared by its three vertical passes.  A thread then owns samples of the strip: it
//                       forms the distinct predictions (1, 3 or 9: a direction whose phase is 0 on every reference does not see its filter) from LDS, reads the source
//                       sample once and adds up to nine squared differences in registers.  Candidates that share a prediction differ in rate only.  Sums: 32 bits in
//                       a thread (at most 64 samples of a 128x128 block, each below 2^20), 64 bits across the wave (lane_reduce.h) and through LDS across the four
//                       waves.  No atomics.  Threads 0 .. 8 then run the model for a candidate each, every thread runs the walk on the nine records in LDS, so the
//                       winner is known to all without another exchange.
//   the winner's block  written in a second walk over the strips from the same LDS data: a block of one strip still has its window and intermediates on chip and
//                       nothing is staged again; a larger block stages each strip once more and makes the one horizontal pass of the winner's x filter.  Only the winner's pair is
//                       formed (predict1), from that one intermediate.
// LDS budget.  A whole 128x128 block of 16-bit samples with three intermediates would be (135 * 135 + 3 * 135 * 128) * 2 = 140 130 bytes of the CU's 160 KB: one
// workgroup per CU.  Strips bound it: one reference 2048 samples per strip (16 rows of a 128-wide block: 23 * (135 + 3 * 128) * 2 = 23 874 bytes at most), two
// references 1024 samples per strip and both references' data side by side (2 * 15 * (135 + 384) * 2 = 31 140 bytes at most).  The kernel declares 32 768 bytes + 1 KB
// of sums and records, so five workgroups (20 waves) fit a CU by LDS; its 127 vector registers allow four (16 waves), so LDS is not what bounds residency.  Blocks of at
// most 2048 / 1024 samples, every shape up to 32x64 / 64x32 for one reference, are one strip.
// What a strip costs: its 7 extra rows are staged and filtered horizontally again, (rows + 7) / rows = 1.44 for the 16-row strips of a 128-wide block.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "fmt_dispatch.h"
#include "lane_reduce.h"
#include "interp_kernels.h"
#include "ifs_search.h"

namespace {

#define PD __device__ __forceinline__

constexpr int WG = 256, WAVES = WG / 64;
constexpr int LDS_ELEMS = 16384;                       // int16 elements of windows and intermediates
constexpr int REACH = ifs::REACH;

using ifs::strip_rows;
static_assert(ifs::LDS_ELEMS_MAX <= LDS_ELEMS, "every shape's strip fits the LDS the kernel declares");

struct RefView {   // one reference of a job as a strip sees it
    const int16_t* win;   // (rows + 7) x wp, origin (-3, -3) of the strip
    const int16_t* im;    // [3] x (rows + 7) x bw, rows from -3
    int            sx, sy;
};

// the nine values of sample (r, c) of a strip from one reference: pixels (COMP = false) or 16-bit compound values (COMP = true), out[fy * 3 + fx].  Where a phase is 0
// the three entries along that filter are equal.  Uniform control flow: the phases are per job.
template <int BD, bool COMP, bool LOWBD> PD void predict9(const RefView& V, int wp, int bw, int im_elems, int r, int c, int* out) {
    using namespace ifs;
    if (!V.sx && !V.sy) {
        const int v = V.win[(r + REACH_LO) * wp + c + REACH_LO], t = COMP ? d16_copy(v, BD) : v;
#pragma unroll
        for (int i = 0; i < NCAND; ++i) out[i] = t;
    } else if (!V.sy) {
        int a[TAPS];
#pragma unroll
        for (int k = 0; k < TAPS; ++k) a[k] = V.win[(r + REACH_LO) * wp + c + k];
#pragma unroll
        for (int fx = 0; fx < FILTERS; ++fx) {
            int res = 0;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) res += kInterp[fx][V.sx][k] * a[k];
            const int t = COMP ? d16_x(res, BD) : sr_x(res, BD);
            out[fx] = out[FILTERS + fx] = out[2 * FILTERS + fx] = t;
        }
    } else if (!V.sx) {
        int a[TAPS];
#pragma unroll
        for (int k = 0; k < TAPS; ++k) a[k] = V.win[(r + k) * wp + c + REACH_LO];
#pragma unroll
        for (int fy = 0; fy < FILTERS; ++fy) {
            int res = 0;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) res += kInterp[fy][V.sy][k] * a[k];
            const int t = COMP ? d16_y(res, BD) : sr_y(res, BD);
            out[fy * FILTERS] = out[fy * FILTERS + 1] = out[fy * FILTERS + 2] = t;
        }
    } else {
#pragma unroll
        for (int fx = 0; fx < FILTERS; ++fx) {
            int a[TAPS];
#pragma unroll
            for (int k = 0; k < TAPS; ++k) a[k] = V.im[fx * im_elems + (r + k) * bw + c];
#pragma unroll
            for (int fy = 0; fy < FILTERS; ++fy) {
                int sum = 0;
#pragma unroll
                for (int k = 0; k < TAPS; ++k) sum += kInterp[fy][V.sy][k] * a[k];
                out[fy * FILTERS + fx] = COMP ? d16_2d(sum, BD) : sr_2d(sum, BD, LOWBD);
            }
        }
    }
}

// one of those nine: sample (r, c) under the pair (fy, fx) alone, for the winner's block.  Reads the one intermediate of x filter fx
template <int BD, bool COMP, bool LOWBD> PD int predict1(const RefView& V, int wp, int bw, int im_elems, int r, int c, int fy, int fx) {
    using namespace ifs;
    if (!V.sx && !V.sy) {
        const int v = V.win[(r + REACH_LO) * wp + c + REACH_LO];
        return COMP ? d16_copy(v, BD) : v;
    }
    int res = 0;
    if (!V.sy) {
#pragma unroll
        for (int k = 0; k < TAPS; ++k) res += kInterp[fx][V.sx][k] * V.win[(r + REACH_LO) * wp + c + k];
        return COMP ? d16_x(res, BD) : sr_x(res, BD);
    }
    if (!V.sx) {
#pragma unroll
        for (int k = 0; k < TAPS; ++k) res += kInterp[fy][V.sy][k] * V.win[(r + k) * wp + c + REACH_LO];
        return COMP ? d16_y(res, BD) : sr_y(res, BD);
    }
#pragma unroll
    for (int k = 0; k < TAPS; ++k) res += kInterp[fy][V.sy][k] * V.im[fx * im_elems + (r + k) * bw + c];
    return COMP ? d16_2d(res, BD) : sr_2d(res, BD, LOWBD);
}

template <typename PIX, int BD>
__global__ __launch_bounds__(WG) void ifs_search_kernel(const PIX* __restrict__ src, int src_stride, const PIX* __restrict__ ref0, int ref0_stride, const PIX* __restrict__ ref1,
                                                        int ref1_stride, PIX* __restrict__ dst, int dst_stride, const ifs::Job* __restrict__ jobs,
                                                        ifs::Result* __restrict__ results, ifs::Cand* __restrict__ cands) {
    using namespace ifs;
    __shared__ int16_t            s_mem[LDS_ELEMS];
    __shared__ unsigned long long s_sum[WAVES][NCAND];
    __shared__ Cand               s_cand[NCAND];
    constexpr bool LOWBD = sizeof(PIX) == 1;
    const int      tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, job = blockIdx.x;
    const Job      J = jobs[job];   // the same for every thread; the host has checked it (ifs::job_ok)
    const bool     two = two_refs(J);
    const int      bw = block_w(J.bsize), bh = block_h(J.bsize), bw_log2 = 31 - __clz(bw);
    const int      rows = strip_rows(bw, bh, two), wp = bw + REACH, win_elems = (rows + REACH) * wp, im_elems = (rows + REACH) * bw;
    const int      slot = win_elems + FILTERS * im_elems, nrefs = two ? 2 : 1;
    const bool     one_strip = rows == bh;
    const int      ny = y_filtered(J) ? FILTERS : 1, nx = x_filtered(J) ? FILTERS : 1;
    const PIX*     rp[2] = {ref0 + (ptrdiff_t)J.ref0_y * ref0_stride + J.ref0_x, two ? ref1 + (ptrdiff_t)J.ref1_y * ref1_stride + J.ref1_x : nullptr};
    const int      rstride[2] = {ref0_stride, ref1_stride};
    RefView        V[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        V[r].win = s_mem + r * slot;
        V[r].im = s_mem + r * slot + win_elems;
        V[r].sx = r ? J.subpel1_x : J.subpel0_x;
        V[r].sy = r ? J.subpel1_y : J.subpel0_y;
    }
    // a strip's windows, then the horizontal passes of the x filters in `fx_mask`; barriers inside, the same for every thread
    auto stage = [&](int y0, unsigned fx_mask) {
        __syncthreads();   // the previous strip has been read
        for (int r = 0; r < nrefs; ++r) {
            int16_t*   w = s_mem + r * slot;
            const PIX* p = rp[r] + (ptrdiff_t)(y0 - REACH_LO) * rstride[r] - REACH_LO;
            for (int i = tid; i < win_elems; i += WG) {
                const int rr = i / wp, cc = i - rr * wp;
                w[i] = (int16_t)p[(ptrdiff_t)rr * rstride[r] + cc];
            }
        }
        __syncthreads();
        for (int r = 0; r < nrefs; ++r) {
            if (!V[r].sx || !V[r].sy) continue;
            const int16_t* w = s_mem + r * slot;
            int16_t*       im = s_mem + r * slot + win_elems;
            for (int i = tid; i < im_elems; i += WG) {
                const int rr = i >> bw_log2, cc = i & (bw - 1);
                int       a[TAPS];
#pragma unroll
                for (int k = 0; k < TAPS; ++k) a[k] = w[rr * wp + cc + k];
#pragma unroll
                for (int fx = 0; fx < FILTERS; ++fx) {
                    if (!(fx_mask >> fx & 1)) continue;
                    int res = 0;
#pragma unroll
                    for (int k = 0; k < TAPS; ++k) res += kInterp[fx][V[r].sx][k] * a[k];
                    im[fx * im_elems + i] = (int16_t)im_sample(res, BD);
                }
            }
        }
        __syncthreads();
    };
    // the nine predictions of sample (r, c) of the staged strip
    auto predict = [&](int r, int c, int* p) {
        if (!two) {
            predict9<BD, false, LOWBD>(V[0], wp, bw, im_elems, r, c, p);
        } else {
            int d0[NCAND], d1[NCAND];
            predict9<BD, true, LOWBD>(V[0], wp, bw, im_elems, r, c, d0);
            predict9<BD, true, LOWBD>(V[1], wp, bw, im_elems, r, c, d1);
#pragma unroll
            for (int i = 0; i < NCAND; ++i) p[i] = comp_pixel(d0[i], d1[i], J.type, J.fwd_offset, J.bck_offset, BD);
        }
    };

    uint32_t acc[NCAND];
#pragma unroll
    for (int i = 0; i < NCAND; ++i) acc[i] = 0;
    const PIX* s = src + (size_t)J.y * src_stride + J.x;
    for (int y0 = 0; y0 < bh; y0 += rows) {
        stage(y0, 7u);
        for (int k = tid; k < rows * bw; k += WG) {
            const int r = k >> bw_log2, c = k & (bw - 1);
            const int sv = s[(size_t)(y0 + r) * src_stride + c];
            int       p[NCAND];
            predict(r, c, p);
#pragma unroll
            for (int fy = 0; fy < FILTERS; ++fy)
#pragma unroll
                for (int fx = 0; fx < FILTERS; ++fx)
                    if (fy < ny && fx < nx) {
                        const int d = sv - p[fy * FILTERS + fx];
                        acc[fy * FILTERS + fx] += (uint32_t)(d * d);
                    }
        }
    }
#pragma unroll
    for (int i = 0; i < NCAND; ++i) {
        const unsigned long long t = wave_sum_u64(acc[i]);
        if (lane == 0) s_sum[wave][i] = t;
    }
    __syncthreads();
    if (tid < NCAND) {
        const int      d = distinct_of(J, tid);
        const uint64_t sse = s_sum[0][d] + s_sum[1][d] + s_sum[2][d] + s_sum[3][d];
        s_cand[tid] = candidate(J, BD, tid, sse);
        if (cands) cands[(size_t)job * NCAND + tid] = s_cand[tid];
    }
    __syncthreads();
    const Result R = decide(J, s_cand);   // every thread: the same nine records, the same walk
    if (tid == 0) results[job] = R;
    if (!dst) return;
    const int by = filter_y(R.best), bx = filter_x(R.best);
    for (int y0 = 0; y0 < bh; y0 += rows) {
        if (!one_strip) stage(y0, 1u << bx);
        for (int k = tid; k < rows * bw; k += WG) {
            const int r = k >> bw_log2, c = k & (bw - 1);
            int       v;
            if (!two) {
                v = predict1<BD, false, LOWBD>(V[0], wp, bw, im_elems, r, c, by, bx);
            } else {
                const int d0 = predict1<BD, true, LOWBD>(V[0], wp, bw, im_elems, r, c, by, bx), d1 = predict1<BD, true, LOWBD>(V[1], wp, bw, im_elems, r, c, by, bx);
                v = comp_pixel(d0, d1, J.type, J.fwd_offset, J.bck_offset, BD);
            }
            dst[(ptrdiff_t)(J.dst_y + y0 + r) * dst_stride + J.dst_x + c] = (PIX)v;
        }
    }
}

}  // namespace

int svt_hip_launch_ifs_search(hipStream_t st, int pix_bytes, int bd, const void* src, int src_stride, const void* ref0, int ref0_stride, const void* ref1, int ref1_stride,
                              void* dst, int dst_stride, const SvtHipIfsJob* jobs, int njobs, SvtHipIfsResult* results, SvtHipIfsCand* cands) {
    if (njobs <= 0) return 0;
    svt_for_fmt(pix_bytes, bd, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL((ifs_search_kernel<PIX, decltype(f)::bd>), dim3(njobs), dim3(WG), 0, st, (const PIX*)src, src_stride, (const PIX*)ref0, ref0_stride, (const PIX*)ref1,
                           ref1_stride, (PIX*)dst, dst_stride, jobs, results, cands);
    });
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(ifs_search)
