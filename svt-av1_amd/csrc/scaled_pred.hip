// scaled_pred.hip — inter prediction from a reference of another size for a list of blocks in one launch, and the job list from block records; gfx950.
//
// Replaces (file:line under the reference's Source/Lib):
//   Common/Codec/EbInterPrediction.c:471-550, :867-946   svt_av1_convolve_2d_scale_c / svt_av1_highbd_convolve_2d_scale_c (C only in the reference:
//                                                         common_dsp_rtcd.c:238-241), as svt_inter_predictor / svt_highbd_inter_predictor call them (:1368-1500)
//   Encoder/Codec/EbEncInterPrediction.c:3591-3661        compute_subpel_params, the scaled branch
// The filter phase changes per output column and row (x_qn = subpel_x + x * xs), so a block's source window is up to twice the block plus 8 each way.  One
// workgroup owns one job and walks it in 32 x 32 output tiles; x_qn / y_qn of a tile's first sample are closed forms of the tile origin (no state passes
// from tile to tile).  Per tile and reference: the source window (at most 70 x 70 samples) is staged in LDS once, the horizontal pass runs once into an
// int16 LDS tile of tile_w x im_h, the vertical pass runs from there into registers.  A compound job does that for both references and combines the two
// 16-bit values in registers: algorithmic bytes = the samples read + the pixels written, no intermediate in HBM.  Every formula is csrc/scaled_pred.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "interp_kernels.h"
#include "lds_stage.h"
#include "scaled_pred.h"

namespace {

constexpr int SP_TILE = 32;
constexpr int SP_WIN = (((SP_TILE - 1) * SP_MAX_STEP + SP_SCALE_SUBPEL_MASK) >> SP_SCALE_SUBPEL_BITS) + SP_TAPS;   // 70: the widest window of a tile
constexpr int SP_PITCH = SP_WIN + 2;
constexpr int SP_PER_THREAD = SP_TILE * SP_TILE / 256;

__device__ __forceinline__ int pow2_shift_at_least(int n, int lo) {   // smallest s >= lo with (1 << s) >= n
    int s = lo;
    while ((1 << s) < n) s++;
    return s;
}
__device__ __forceinline__ bool ref_fields_ok(int subpel_x, int subpel_y, int xs, int ys) {
    return subpel_x <= SP_SCALE_SUBPEL_MASK && subpel_y <= SP_SCALE_SUBPEL_MASK && xs >= 1 && xs <= SP_MAX_STEP && ys >= 1 && ys <= SP_MAX_STEP;
}

// One reference of one tile: d[u] = the 16-bit value of output tid + 256 * u (column = index & (cwp - 1), row = index >> cshift)
template <typename PIX, int BD>
__device__ __forceinline__ void tile_values(uint16_t* s_src, int16_t* s_im, const int16_t (*s_f)[16][8], const PIX* __restrict__ ref, int ref_stride, int pos_x,
                                            int pos_y, int X0, int Y0, int xs, int ys, int cw, int ch, int cshift, bool compound, int tid, int* d) {
    const int sx0 = X0 & SP_SCALE_SUBPEL_MASK, sy0 = Y0 & SP_SCALE_SUBPEL_MASK;
    const int cols = sp_span(sx0, xs, cw), rows = sp_span(sy0, ys, ch);          // <= SP_WIN each: cw, ch <= SP_TILE, steps <= SP_MAX_STEP
    const PIX* win = ref + (ptrdiff_t)(pos_y + (Y0 >> SP_SCALE_SUBPEL_BITS) - 3) * ref_stride + (pos_x + (X0 >> SP_SCALE_SUBPEL_BITS) - 3);
    __syncthreads();                                                             // the previous tile / reference has left s_src and s_im
    {   // the window, rows x cols, as rows x (1 << wshift) work items; a lane past the last column loads that column again and stores nothing
        const int wshift = pow2_shift_at_least(cols, 5), wmask = (1 << wshift) - 1;
        batched_stage<4, PIX>(rows << wshift, tid, 256,
            [&](int i) { return win[(ptrdiff_t)(i >> wshift) * ref_stride + min(i & wmask, cols - 1)]; },
            [&](int i, PIX v) { if ((i & wmask) < cols) s_src[(i >> wshift) * SP_PITCH + (i & wmask)] = v; });
    }
    __syncthreads();
    const int c = tid & ((1 << cshift) - 1), r0 = tid >> cshift, rstep = 256 >> cshift;
    if (c < cw) {   // horizontal: this thread's column has one filter and one first tap for every row
        int16_t f[8];
        const int idx = sp_filter_idx(sx0, xs, c), tap0 = sp_tap0(sx0, xs, c);
#pragma unroll
        for (int k = 0; k < 8; k++) f[k] = s_f[0][idx][k];
        for (int r = r0; r < rows; r += rstep) s_im[r * SP_TILE + c] = sp_horiz<BD>(f, s_src + r * SP_PITCH + tap0);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SP_PER_THREAD; u++) {   // vertical
        const int y = r0 + u * rstep;
        d[u] = 0;
        if (c < cw && y < ch) d[u] = sp_vert<BD>(s_f[1][sp_filter_idx(sy0, ys, y)], s_im + sp_tap0(sy0, ys, y) * SP_TILE + c, SP_TILE, compound);
    }
}

// 7 waves per SIMD: 72 registers without a spill (8 would spill; the plain 256 takes 80 and 6 waves, measured 0 - 5 % slower: docs/kernels/scaled_pred.md)
template <typename PIX, int BD>
__global__ void __launch_bounds__(256, 7)
scaled_predict_kernel(const PIX* __restrict__ ref0, int ref0_stride, const PIX* __restrict__ ref1, int ref1_stride, PIX* __restrict__ dst, int dst_stride,
                      const SvtHipScaledBlk* __restrict__ jobs) {
    __shared__ uint16_t s_src[SP_WIN * SP_PITCH];
    __shared__ int16_t s_im[SP_WIN * SP_TILE];
    __shared__ __attribute__((aligned(16))) int16_t s_f[2][16][8];
    const SvtHipScaledBlk b = jobs[svt_xcd_order(blockIdx.x, gridDim.x)];   // the job list is in raster order of the blocks: an XCD takes a band of them
    const int tid = threadIdx.x;
    const bool compound = b.compound != 0;
    // what keeps every LDS index inside its array; uniform over the workgroup
    if (b.w < 1 || b.w > SP_MAX_BLOCK || b.h < 1 || b.h > SP_MAX_BLOCK || b.bank_x > 5 || b.bank_y > 5 || b.compound > 2 || !ref_fields_ok(b.subpel0_x, b.subpel0_y, b.xs0, b.ys0) ||
        (compound && !ref_fields_ok(b.subpel1_x, b.subpel1_y, b.xs1, b.ys1)))
        return;
    s_f[tid >> 7][(tid >> 3) & 15][tid & 7] = kInterp[(tid >> 7) ? b.bank_y : b.bank_x][(tid >> 3) & 15][tid & 7];   // 2 banks x 16 phases x 8 taps = 256 values
    const int cshift = pow2_shift_at_least(min((int)b.w, SP_TILE), 2), rstep = 256 >> cshift;
    for (int oy = 0; oy < b.h; oy += SP_TILE)
        for (int ox = 0; ox < b.w; ox += SP_TILE) {
            const int cw = min(SP_TILE, b.w - ox), ch = min(SP_TILE, b.h - oy);
            int d0[SP_PER_THREAD], d1[SP_PER_THREAD];
            tile_values<PIX, BD>(s_src, s_im, s_f, ref0, ref0_stride, b.pos0_x, b.pos0_y, b.subpel0_x + ox * b.xs0, b.subpel0_y + oy * b.ys0, b.xs0, b.ys0, cw, ch, cshift,
                                 compound, tid, d0);
            if (compound)
                tile_values<PIX, BD>(s_src, s_im, s_f, ref1, ref1_stride, b.pos1_x, b.pos1_y, b.subpel1_x + ox * b.xs1, b.subpel1_y + oy * b.ys1, b.xs1, b.ys1, cw, ch,
                                     cshift, true, tid, d1);
            const int c = tid & ((1 << cshift) - 1), r0 = tid >> cshift;
#pragma unroll
            for (int u = 0; u < SP_PER_THREAD; u++) {
                const int y = r0 + u * rstep;
                if (c < cw && y < ch) {
                    const int res = compound ? sp_combine(d0[u], d1[u], b.compound, b.fwd_offset, b.bck_offset) : d0[u];
                    dst[(ptrdiff_t)(b.dst_y + oy + y) * dst_stride + (b.dst_x + ox + c)] = (PIX)sp_final<BD>(res, compound);
                }
            }
        }
}

__global__ void __launch_bounds__(256)
scaled_jobs_kernel(SvtHipScaleFactors sf0, SvtHipScaleFactors sf1, int fw0, int fh0, int fw1, int fh1, const SvtHipScaledRec* __restrict__ recs,
                   SvtHipScaledBlk* __restrict__ jobs, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) jobs[i] = sp_job_of_record(recs[i], sf0, sf1, fw0, fh0, fw1, fh1);
}

}  // namespace

extern "C" int svt_hip_launch_scaled_predict(hipStream_t st, int pix_bytes, int bd, const void* ref0, int ref0_stride, const void* ref1, int ref1_stride, void* dst,
                                             int dst_stride, const SvtHipScaledBlk* jobs, int n) {
    if (n <= 0) return 0;
    svt_for_fmt12(pix_bytes, bd, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL((scaled_predict_kernel<PIX, decltype(f)::bd>), dim3(n), dim3(256), 0, st, (const PIX*)ref0, ref0_stride, (const PIX*)ref1, ref1_stride, (PIX*)dst,
                           dst_stride, jobs);
    });
    return (int)hipGetLastError();
}

extern "C" int svt_hip_launch_scaled_jobs(hipStream_t st, const SvtHipScaleFactors* sf0, const SvtHipScaleFactors* sf1, const int frame_w[2], const int frame_h[2],
                                          const SvtHipScaledRec* recs, SvtHipScaledBlk* jobs, int n) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(scaled_jobs_kernel, dim3((n + 255) / 256), dim3(256), 0, st, *sf0, *sf1, frame_w[0], frame_h[0], frame_w[1], frame_h[1], recs, jobs, n);
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(scaled_pred)
