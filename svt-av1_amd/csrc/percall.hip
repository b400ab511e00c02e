// percall.hip — stand-alone forms of operations that otherwise only exist fused inside the frame kernels: the small helpers of the reference's
// dispatch table behind the per-call table of include/svt_hip_rtcd.h (quantizers, residual, the SAD ladders of the open-loop search, the means and
// variance intermediates of picture analysis, the 64-point coefficient re-packs, the stand-alone convolutions, compound masks and blends, CDEF's
// distortion of one filter block, the self-guided projection on materialised flt0 / flt1 planes, the lossless 4x4 inverse).  A kernel that takes a LIST
// of units lets a caller with many of them pay one launch; the per-call table launches it with a list of one.  CDEF's strength decision has its
// own unit (cdef_select.hip).  Bit-exact restatements of (paths under Source/Lib of the reference):
//   quantize_blocks        Encoder/Codec/EbFullLoop.c:37-93, :171-225, :314-377, :467-532
//   residual               Common/Codec/EbPictureOperators.c (svt_residual_kernel8bit_c / 16bit_c)
//   ext_all_sad            Encoder/Codec/EbMotionEstimation.c:230-388
//   ext_eight_sad_32_64    Encoder/Codec/EbMotionEstimation.c:394-458
//   ext_sad_16 / _32_64    Encoder/Codec/EbMotionEstimation.c:122-228         svt_ext_sad_calculation_8x8_16x16_c, _32x32_64x64_c
//   interm_var_four8x8     Encoder/Codec/EbPictureAnalysisProcess.c:309-381
//   block_mean             Encoder/Codec/EbPictureAnalysisProcess.c:287-326   svt_compute_mean_squared_values_c, svt_compute_sub_mean_8x8_c
//   handle_transform64     Encoder/Codec/EbTransforms.c:2750-2932
//   repack64               Encoder/Codec/EbTransforms.c:2933-2969             handle_transform*_N2_N4_c
//   upsampled_pred         Encoder/C_DEFAULT/variance.c:212-266 + Common/Codec/convolve.c:244-316
//   convolve8              Common/Codec/convolve.c:249-307                    svt_aom_convolve8_horiz_c / _vert_c
//   wiener_convolve        Common/Codec/convolve.c:57-242                     svt_av1_[highbd_]wiener_convolve_add_src_c
//   jnt_convolve           Common/Codec/EbInterPrediction.c:552-741, :868-1143  svt_av1_[highbd_]jnt_convolve_{2d,x,y,2d_copy}_c
//   diffwtd_mask           Common/Codec/EbInterPrediction.c:78-175; Common/C_DEFAULT/EbInterPrediction_c.c:15-45  svt_av1_build_compound_diffwtd_mask[_highbd|_d16]_c
//   blend_d16              Common/Codec/EbBlend_a64_mask.c:34-215             svt_aom_{lowbd,highbd}_blend_a64_d16_mask_c
//   cdef_dist              Encoder/Codec/EbEncCdef.c:25-220                   compute_cdef_dist_c / _8bit_c
//   sgr_flt_proj           Encoder/Codec/EbRestorationPick.c:174-316, :448-538  svt_av1_{lowbd,highbd}_pixel_proj_error_c, svt_get_proj_subspace_c
//   iwht4x4_add            Common/Codec/EbInvTransforms.c:2771-2864           svt_av1_highbd_iwht4x4_{16,1}_add_c
#include <hip/hip_runtime.h>
#include <cstddef>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "lane_reduce.h"
#include "interp_kernels.h"
#include "quant_dev.h"

namespace {

__constant__ int16_t kTaps[6][16][8] = SVT_HIP_INTERP_TABLE;
__device__ __forceinline__ int clip_px(int v, int bd) { const int mx = (1 << bd) - 1; return v < 0 ? 0 : (v > mx ? mx : v); }

// ------------------------------------------------------------------------------------------------ quantizers
// one workgroup per block of n coefficients; eob = 1 + the largest scan position holding a non-zero level
__global__ void __launch_bounds__(256)
quantize_blocks_kernel(const int32_t* __restrict__ coeff, int n, SvtHipQuantParams qp, const int16_t* __restrict__ iscan, int32_t* __restrict__ qcoeff,
                       int32_t* __restrict__ dqcoeff, uint16_t* __restrict__ eob) {
    __shared__ unsigned s_eob;
    const size_t base = (size_t)blockIdx.x * n;
    if (threadIdx.x == 0) s_eob = 0;
    __syncthreads();
    unsigned e = 0;
    for (int rc = threadIdx.x; rc < n; rc += 256) {
        const int32_t c = coeff[base + rc];
        int32_t dq;
        const int32_t lvl = quant_one(qp, c, rc != 0, dq);
        qcoeff[base + rc] = c < 0 ? -lvl : lvl;
        dqcoeff[base + rc] = c < 0 ? -dq : dq;
        if (lvl) e = max(e, (unsigned)iscan[rc] + 1u);
    }
    if (e) atomicMax(&s_eob, e);
    __syncthreads();
    if (threadIdx.x == 0) eob[blockIdx.x] = (uint16_t)s_eob;
}

// ------------------------------------------------------------------------------------------------ residual
template <typename PIX>
__global__ void __launch_bounds__(256)
residual_kernel(const PIX* __restrict__ src, int ss, const PIX* __restrict__ pred, int ps, int16_t* __restrict__ res, int rs, int w, int h) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x < w && y < h) res[(size_t)y * rs + x] = (int16_t)((int)src[(size_t)y * ss + x] - (int)pred[(size_t)y * ps + x]);
}

// ------------------------------------------------------------------------------------------------ 8-candidate SAD ladders
// state layout (uint32): best_sad8x8[64] best_sad16x16[16] best_mv8x8[64] best_mv16x16[16] eight_sad16x16[16][8] eight_sad8x8[64][8]
// (indices in the reference's z-order: 16x16 block (y, x) -> kZ16[4 * y + x], its 8x8 quadrant k -> 4 * that + k)
__constant__ uint8_t kZ16[16] = {0, 1, 4, 5, 2, 3, 6, 7, 8, 9, 12, 13, 10, 11, 14, 15};
__device__ __forceinline__ uint32_t step_mv(uint32_t mv, int j) {   // x advances 4 quarter-pel units per candidate
    const int16_t x = (int16_t)((int16_t)(mv & 0xffff) + (int16_t)(j * 4)), y = (int16_t)(mv >> 16);
    return ((uint32_t)(uint16_t)y << 16) | (uint16_t)x;
}
__global__ void __launch_bounds__(512)
ext_all_sad_kernel(const uint8_t* __restrict__ src, int ss, const uint8_t* __restrict__ ref, int rs, const SvtHipExtSadJob* __restrict__ jobs, uint32_t* __restrict__ state) {
    __shared__ uint32_t s8[64][8], s16[16][8];
    const SvtHipExtSadJob j = jobs[blockIdx.x];
    uint32_t* st = state + (size_t)blockIdx.x * 800;
    const int tid = threadIdx.x, b = tid >> 3, c = tid & 7, by = b >> 3, bx = b & 7;
    const uint8_t* s = src + j.src_off + (by * 8) * ss + bx * 8;
    const uint8_t* r = ref + j.ref_off + (by * 8) * rs + bx * 8 + c;
    uint32_t sad = 0;
    const int rstep = j.sub_sad ? 2 : 1;
    for (int y = 0; y < 8; y += rstep)
#pragma unroll
        for (int x = 0; x < 8; x++) sad += (uint32_t)abs((int)s[y * ss + x] - (int)r[y * rs + x]);
    if (j.sub_sad) sad <<= 1;
    const int z16 = kZ16[4 * (by >> 1) + (bx >> 1)], z8 = 4 * z16 + 2 * (by & 1) + (bx & 1);
    s8[z8][c] = sad;
    st[160 + 128 + z8 * 8 + c] = sad;
    __syncthreads();
    if (tid < 128) {
        const int k = tid >> 3;
        const uint32_t v = s8[4 * k][c] + s8[4 * k + 1][c] + s8[4 * k + 2][c] + s8[4 * k + 3][c];
        s16[k][c] = v;
        st[160 + k * 8 + c] = v;
    }
    __syncthreads();
    if (tid < 80) {   // candidates in order, strictly-smaller wins: the first smallest keeps the vector
        const bool is8 = tid < 64;
        const int k = is8 ? tid : tid - 64;
        uint32_t* bs = st + (is8 ? 0 : 64) + k;
        uint32_t* bm = st + (is8 ? 80 : 144) + k;
        uint32_t best = *bs, mv = *bm;
        for (int q = 0; q < 8; q++) {
            const uint32_t v = is8 ? s8[k][q] : s16[k][q];
            if (v < best) { best = v; mv = step_mv(j.mv, q); }
        }
        *bs = best; *bm = mv;
    }
}
// state layout (uint32): sad16x16[16][8] (in) best_sad32x32[4] best_sad64x64 best_mv32x32[4] best_mv64x64 (in/out) sad32x32[4][8] (out) = 170
__global__ void __launch_bounds__(64)
ext_eight_sad_32_64_kernel(const uint32_t* __restrict__ mvs, uint32_t* __restrict__ state) {
    __shared__ uint32_t s32[5][8];
    uint32_t* st = state + (size_t)blockIdx.x * 170;
    const int tid = threadIdx.x;
    if (tid < 32) {
        const int k = tid >> 3, c = tid & 7;
        const uint32_t v = st[(4 * k) * 8 + c] + st[(4 * k + 1) * 8 + c] + st[(4 * k + 2) * 8 + c] + st[(4 * k + 3) * 8 + c];
        s32[k][c] = v;
        st[138 + k * 8 + c] = v;
    }
    __syncthreads();
    if (tid < 8) s32[4][tid] = s32[0][tid] + s32[1][tid] + s32[2][tid] + s32[3][tid];
    __syncthreads();
    if (tid < 5) {
        uint32_t best = st[128 + tid], mv = st[133 + tid];
        for (int q = 0; q < 8; q++)
            if (s32[tid][q] < best) { best = s32[tid][q]; mv = step_mv(mvs[blockIdx.x], q); }
        st[128 + tid] = best; st[133 + tid] = mv;
    }
}

// ------------------------------------------------------------------------------------------------ single-candidate SAD ladders
// state of one 16x16 job (uint32): best_sad8x8[4] best_sad16x16 best_mv8x8[4] best_mv16x16 | sad16x16 sad8x8[4]   (15 words, the last five are outputs)
__global__ void __launch_bounds__(64)
ext_sad_16_kernel(const uint8_t* __restrict__ src, int ss, const uint8_t* __restrict__ ref, int rs, const SvtHipExtSadJob* __restrict__ jobs, uint32_t* __restrict__ state) {
    const SvtHipExtSadJob j = jobs[blockIdx.x];
    const uint8_t *s = src + j.src_off, *r = ref + j.ref_off;
    const int      lane = threadIdx.x, q = lane >> 4, l16 = lane & 15;   // quadrant q: 8x8 block (q >> 1, q & 1); 16 lanes x 4 pixels
    const int      qy = 8 * (q >> 1), qx = 8 * (q & 1);
    unsigned       acc = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int p = l16 * 4 + k, y = p >> 3, x = p & 7;
        if (!j.sub_sad || !(y & 1)) acc += (unsigned)abs((int)s[(size_t)(qy + y) * ss + qx + x] - (int)r[(size_t)(qy + y) * rs + qx + x]);
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) acc += lane_xor(acc, m);
    if (j.sub_sad) acc <<= 1;   // compute8x4_sad_kernel on every other row, doubled
    const unsigned s0 = (unsigned)__shfl((int)acc, 0, 64), s1 = (unsigned)__shfl((int)acc, 16, 64), s2 = (unsigned)__shfl((int)acc, 32, 64), s3 = (unsigned)__shfl((int)acc, 48, 64);
    if (lane == 0) {
        uint32_t*      st = state + (size_t)blockIdx.x * 15;
        const unsigned sad8[4] = {s0, s1, s2, s3};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            st[11 + k] = sad8[k];
            if (sad8[k] < st[k]) { st[k] = sad8[k]; st[5 + k] = j.mv; }
        }
        const unsigned sad16 = s0 + s1 + s2 + s3;
        if (sad16 < st[4]) { st[4] = sad16; st[9] = j.mv; }
        st[10] = sad16;
    }
}
// state of one 64x64 job (uint32): sad16x16[16] (input) best_sad32x32[4] best_sad64x64 best_mv32x32[4] best_mv64x64 | sad32x32[4]   (30 words)
__global__ void __launch_bounds__(64)
ext_sad_32_64_kernel(uint32_t* __restrict__ state, const uint32_t* __restrict__ mv, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t* st = state + (size_t)i * 30;
    uint32_t  s64 = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t s32 = st[4 * k] + st[4 * k + 1] + st[4 * k + 2] + st[4 * k + 3];
        st[26 + k] = s32;
        if (s32 < st[16 + k]) { st[16 + k] = s32; st[21 + k] = mv[i]; }
        s64 += s32;
    }
    if (s64 < st[20]) { st[20] = s64; st[25] = mv[i]; }
}

// ------------------------------------------------------------------------------------------------ variance intermediates
// four horizontally adjacent 8x8 blocks, rows 0 2 4 6 only: mean << 3 and mean of squares << 11 with the reference's scaling
__global__ void __launch_bounds__(64)
interm_var_kernel(const uint8_t* __restrict__ plane, int stride, const int32_t* __restrict__ offs, uint64_t* __restrict__ mean, uint64_t* __restrict__ mean_sq) {
    const int lane = threadIdx.x, blk = lane >> 4, col = (lane >> 1) & 7, half = lane & 1;
    const uint8_t* p = plane + offs[blockIdx.x] + blk * 8 + col;
    uint32_t s = 0, q = 0;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const uint32_t v = p[(size_t)(2 * (2 * half + k)) * stride];
        s += v; q += v * v;
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) { s += __shfl_xor(s, m); q += __shfl_xor(q, m); }
    if ((lane & 15) == 0) { mean[blockIdx.x * 4 + blk] = (uint64_t)s << 3; mean_sq[blockIdx.x * 4 + blk] = (uint64_t)q << 11; }
}

// ------------------------------------------------------------------------------------------------ picture-analysis block means
// mode 0: (sum of squares << 16) / (w * h) over a w x h area; mode 1: sum over rows 0, 2, 4, 6 of an 8 x 8 block, << 3.  One wave per block.
__global__ void __launch_bounds__(64)
block_mean_kernel(const uint8_t* __restrict__ plane, int stride, const int32_t* __restrict__ offs, int mode, int w, int h, uint64_t* __restrict__ out) {
    const uint8_t* p = plane + offs[blockIdx.x];
    unsigned long long acc = 0;
    if (mode == 0) {
        for (int i = threadIdx.x; i < w * h; i += 64) { const int y = i / w, x = i - y * w; const unsigned v = p[(size_t)y * stride + x]; acc += v * v; }
    } else if (threadIdx.x < 32) {
        const int y = 2 * (threadIdx.x >> 3), x = threadIdx.x & 7;
        acc = p[(size_t)y * stride + x];
    }
    acc = wave_sum_u64(acc);
    if (threadIdx.x == 0) out[blockIdx.x] = mode == 0 ? (acc << 16) / (unsigned long long)(w * h) : acc << 3;
}

// ------------------------------------------------------------------------------------------------ 64-point coefficient re-pack
// in place on a W x H block of coefficients: energy of everything outside the top-left 32 x 32, zero it, pack the kept rows to stride min(W, 32).
// Every thread reads all it needs before anybody writes, so the final buffer equals the reference's (including the stale middle rows it leaves).
template <int W, int H>
__global__ void __launch_bounds__(1024)
handle_transform64_kernel(int32_t* __restrict__ coeff, uint64_t* __restrict__ energy) {
    constexpr int KW = W > 32 ? 32 : W, KH = H > 32 ? 32 : H, N = W * H, NK = KW * KH, PER = (N + 1023) / 1024;
    __shared__ unsigned long long s_e;
    int32_t* c = coeff + (size_t)blockIdx.x * N;
    const int tid = threadIdx.x;
    if (tid == 0) s_e = 0;
    __syncthreads();
    int32_t nv[PER];
    unsigned long long e = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int i = tid + k * 1024;
        if (i >= N) { nv[k] = 0; continue; }
        const int r = i / W, col = i % W;
        const int32_t old = c[i];
        const bool dropped = r >= 32 || col >= 32;
        if (dropped) e += (unsigned long long)((int64_t)old * (int64_t)old);
        nv[k] = i < NK ? c[(i / KW) * W + (i % KW)] : (dropped ? 0 : old);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) e += __shfl_xor(e, m);
    if ((tid & 63) == 0 && e) atomicAdd(&s_e, e);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int i = tid + k * 1024;
        if (i < N) c[i] = nv[k];
    }
    if (tid == 0) energy[blockIdx.x] = s_e;
}

// ------------------------------------------------------------------------------------------------ 64-point re-pack of the N2 / N4 coefficient shapes
// handle_transform64x{16,32,64}_N2_N4_c (EbTransforms.c:2947-2969): rows 1 .. rows-1 move from stride 64 to stride 32, nothing is zeroed, no energy
__global__ void __launch_bounds__(1024)
repack64_kernel(int32_t* __restrict__ coeff, int rows, int per_block) {
    int32_t* c = coeff + (size_t)blockIdx.x * per_block;
    const int r = threadIdx.x >> 5, x = threadIdx.x & 31;
    const int32_t v = r < rows ? c[r * 64 + x] : 0;
    __syncthreads();
    if (r < rows) c[r * 32 + x] = v;
}

// ------------------------------------------------------------------------------------------------ up-sampled prediction
// two 8-tap passes with a round-to-8-bit clip after each (the libvpx-style convolve8, not the AV1 normative one)
__global__ void __launch_bounds__(256)
upsampled_pred_kernel(const uint8_t* __restrict__ ref, int rs, uint8_t* __restrict__ dst, const SvtHipUpsampledBlk* __restrict__ blks) {
    __shared__ uint8_t tmp[(128 + 7) * 128];
    const SvtHipUpsampledBlk b = blks[blockIdx.x];
    const int w = b.w, h = b.h, tid = threadIdx.x;
    const uint8_t* r0 = ref + b.ref_off;
    uint8_t* d = dst + b.dst_off;
    const int16_t* fx = kTaps[b.bank][(b.subpel_x_q3 << 1) & 15];
    const int16_t* fy = kTaps[b.bank][(b.subpel_y_q3 << 1) & 15];
    const int row0 = b.subpel_y_q3 ? -3 : 0, rows = b.subpel_y_q3 ? h + 7 : h;
    for (int i = tid; i < rows * w; i += 256) {
        const int y = i / w, x = i % w;
        const uint8_t* p = r0 + (ptrdiff_t)(y + row0) * rs + x;
        int v;
        if (b.subpel_x_q3) {
            int sum = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) sum += (int)p[k - 3] * (int)fx[k];
            v = clip_px((sum + 64) >> 7, 8);
        } else {
            v = p[0];
        }
        if (b.subpel_y_q3) tmp[y * 128 + x] = (uint8_t)v; else d[y * w + x] = (uint8_t)v;
    }
    if (!b.subpel_y_q3) return;
    __syncthreads();
    for (int i = tid; i < h * w; i += 256) {
        const int y = i / w, x = i % w;
        int sum = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) sum += (int)tmp[(y + k) * 128 + x] * (int)fy[k];
        d[y * w + x] = (uint8_t)clip_px((sum + 64) >> 7, 8);
    }
}

// ------------------------------------------------------------------------------------------------ 8-tap convolution with a phase table (scaling allowed)
// filters[16][8]: the 256-byte-aligned kernel table the reference derives from its filter pointer; q0 = first phase, step = phase advance per sample
template <bool VERT>
__global__ void __launch_bounds__(256)
convolve8_kernel(const uint8_t* __restrict__ src, int ss, uint8_t* __restrict__ dst, int ds, const int16_t* __restrict__ filters, int q0, int step, int w, int h) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const int      q = q0 + (VERT ? y : x) * step, base = (q >> 4) - 3;
    const int16_t* f = filters + 8 * (q & 15);
    int            sum = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) sum += (int)(VERT ? src[(ptrdiff_t)(base + k) * ss + x] : src[(ptrdiff_t)y * ss + base + k]) * f[k];
    dst[(size_t)y * ds + x] = (uint8_t)clip_px((sum + 64) >> 7, 8);
}

// ------------------------------------------------------------------------------------------------ Wiener convolution of one processing unit
// horizontal pass with the source added and the intermediate clamp, vertical pass on the clamped rows; step 16 (no scaling), taps fx / fy.
template <typename PIX>
__global__ void __launch_bounds__(256)
wiener_convolve_kernel(const PIX* __restrict__ src, int ss, PIX* __restrict__ dst, int ds, const int16_t* __restrict__ taps, int w, int h, int round0, int round1, int bd) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const int16_t *fx = taps, *fy = taps + 8;
    const int      lim = (1 << (bd + 1 + 7 - round0)) - 1;
    int            mid[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const PIX* row = src + (ptrdiff_t)(y + k - 3) * ss + x - 3;
        int        sum = ((int)row[3] << 7) + (1 << (bd + 7 - 1));
#pragma unroll
        for (int t = 0; t < 8; t++) sum += (int)row[t] * fx[t];
        const int v = (sum + ((1 << round0) >> 1)) >> round0;
        mid[k] = v < 0 ? 0 : (v > lim ? lim : v);
    }
    int sum = (mid[3] << 7) - (1 << (bd + round1 - 1));
#pragma unroll
    for (int k = 0; k < 8; k++) sum += mid[k] * fy[k];
    dst[(size_t)y * ds + x] = (PIX)clip_px((sum + ((1 << round1) >> 1)) >> round1, bd);
}

// ------------------------------------------------------------------------------------------------ one reference of a compound prediction
// variant 0 = 2d, 1 = x, 2 = y, 3 = 2d_copy.  do_average = 0: the 16-bit result goes to the compound buffer; 1: it is combined with the buffer
// (plain or distance-weighted average) and written to dst as pixels.  taps[0..7] horizontal, taps[8..15] vertical kernel.
struct JntArgs { int variant, w, h, round0, round1, do_average, use_jnt, fwd, bck, bd; };
template <typename PIX>
__global__ void __launch_bounds__(256)
jnt_convolve_kernel(const PIX* __restrict__ src, int ss, PIX* __restrict__ dst, int ds, uint16_t* __restrict__ cb, int cbs, const int16_t* __restrict__ taps, JntArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.w || y >= a.h) return;
    const int16_t *fx = taps, *fy = taps + 8;
    const int      offset_bits = a.bd + 14 - a.round0, round_offset = (1 << (offset_bits - a.round1)) + (1 << (offset_bits - a.round1 - 1));
    const int      round_bits = 14 - a.round0 - a.round1;
    int            res;
    if (a.variant == 0) {
        int sum = 1 << offset_bits;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const PIX* row = src + (ptrdiff_t)(y + k - 3) * ss + x - 3;
            int        hs = 1 << (a.bd + 6);
#pragma unroll
            for (int t = 0; t < 8; t++) hs += fx[t] * (int)row[t];
            sum += fy[k] * (int)(int16_t)((hs + ((1 << a.round0) >> 1)) >> a.round0);
        }
        res = (int)(uint16_t)((sum + ((1 << a.round1) >> 1)) >> a.round1);
    } else if (a.variant == 1) {
        int hs = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) hs += fx[t] * (int)src[(ptrdiff_t)y * ss + x - 3 + t];
        res = (1 << (7 - a.round1)) * ((hs + ((1 << a.round0) >> 1)) >> a.round0) + round_offset;
    } else if (a.variant == 2) {
        int vs = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) vs += fy[k] * (int)src[(ptrdiff_t)(y + k - 3) * ss + x];
        vs *= 1 << (7 - a.round0);
        res = ((vs + ((1 << a.round1) >> 1)) >> a.round1) + round_offset;
    } else
        res = (int)(uint16_t)(((int)src[(ptrdiff_t)y * ss + x] << round_bits) + round_offset);
    if (!a.do_average) { cb[(size_t)y * cbs + x] = (uint16_t)res; return; }
    int tmp = cb[(size_t)y * cbs + x];
    tmp = a.use_jnt ? (tmp * a.fwd + res * a.bck) >> 4 : (tmp + res) >> 1;
    tmp -= round_offset;
    dst[(size_t)y * ds + x] = (PIX)clip_px((tmp + ((1 << round_bits) >> 1)) >> round_bits, a.bd);
}

// ------------------------------------------------------------------------------------------------ difference-weighted compound mask, d16 blend
// mask[i * w + j] = 38 + (|a - b| rounded by `round`, shifted by `shift`) / 16, clamped to [0, 64], inverted for DIFFWTD_38_INV
template <typename T>
__global__ void __launch_bounds__(256)
diffwtd_mask_kernel(uint8_t* __restrict__ mask, const T* __restrict__ a, int as, const T* __restrict__ b, int bs, int w, int h, int inverse, int round, int shift) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= w * h) return;
    const int y = i / w, x = i - y * w;
    int d = abs((int)a[(size_t)y * as + x] - (int)b[(size_t)y * bs + x]);
    if (round > 0) d = (d + (1 << (round - 1))) >> round;
    d >>= shift;
    const int m = min(max(38 + d / 16, 0), 64);
    mask[i] = (uint8_t)(inverse ? 64 - m : m);
}
template <typename PIX>
__global__ void __launch_bounds__(256)
blend_d16_kernel(PIX* __restrict__ dst, int ds, const uint16_t* __restrict__ s0, int s0s, const uint16_t* __restrict__ s1, int s1s, const uint8_t* __restrict__ mask, int ms, int w,
                 int h, int subw, int subh, int round_offset, int round_bits, int bd) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    int m;
    if (!subw && !subh) m = mask[(size_t)y * ms + x];
    else if (subw && subh) m = (mask[(size_t)(2 * y) * ms + 2 * x] + mask[(size_t)(2 * y + 1) * ms + 2 * x] + mask[(size_t)(2 * y) * ms + 2 * x + 1] + mask[(size_t)(2 * y + 1) * ms + 2 * x + 1] + 2) >> 2;
    else if (subw) m = (mask[(size_t)y * ms + 2 * x] + mask[(size_t)y * ms + 2 * x + 1] + 1) >> 1;
    else m = (mask[(size_t)(2 * y) * ms + x] + mask[(size_t)(2 * y + 1) * ms + x] + 1) >> 1;
    int res = (m * (int)s0[(size_t)y * s0s + x] + (64 - m) * (int)s1[(size_t)y * s1s + x]) >> 6;
    res -= round_offset;
    dst[(size_t)y * ds + x] = (PIX)clip_px((res + ((1 << round_bits) >> 1)) >> round_bits, bd);
}

// ------------------------------------------------------------------------------------------------ CDEF: distortion of one filter block
// dst: the picture plane (source pixels), src: the filtered blocks packed one after the other (bw x bh each) — the reference's argument names.
template <typename PIX>
__global__ void __launch_bounds__(256)
cdef_dist_kernel(const PIX* __restrict__ dst, int dstride, const PIX* __restrict__ src, const uint8_t* __restrict__ list, int n, int bw_log2, int bh_log2, int cs,
                 int pli, uint64_t* __restrict__ out) {
    __shared__ unsigned long long part[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int bw = 1 << bw_log2, npx = 1 << (bw_log2 + bh_log2);
    unsigned long long acc = 0;
    for (int bi = wave; bi < n; bi += 4) {
        const int by = list[3 * bi], bx = list[3 * bi + 1];   // CdefList {by, bx, skip}
        const bool on = lane < npx;
        const int  i = lane >> bw_log2, jx = lane & (bw - 1);
        const unsigned s = on ? src[((size_t)bi << (bw_log2 + bh_log2)) + lane] : 0u;
        const unsigned d = on ? dst[(size_t)((by << bh_log2) + i) * dstride + (bx << bw_log2) + jx] : 0u;
        if (pli == 0 && bw_log2 == 3 && bh_log2 == 3) {   // dist_8x8_*: the perceptual luma metric
            const unsigned long long sum_s = wave_sum_u64(s), sum_d = wave_sum_u64(d), sum_s2 = wave_sum_u64((unsigned long long)s * s),
                                     sum_d2 = wave_sum_u64((unsigned long long)d * d), sum_sd = wave_sum_u64((unsigned long long)s * d);
            const uint64_t svar = sum_s2 - ((sum_s * sum_s + 32) >> 6);
            const uint64_t dvar = sum_d2 - ((sum_d * sum_d + 32) >> 6);
            const double   num = (double)(sum_d2 + sum_s2 - 2 * sum_sd) * .5 * (double)(svar + dvar + (uint64_t)(400 << 2 * cs));
            const double   den = sqrt((double)(20000 << 4 * cs) + (double)svar * (double)dvar);
            acc += (unsigned long long)floor(.5 + num / den);
        } else {
            const int e = (int)d - (int)s;
            acc += wave_sum_u64((unsigned long long)(unsigned)(e * e));
        }
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (part[0] + part[1] + part[2] + part[3]) >> (2 * cs);
}

// ------------------------------------------------------------------------------------------------ self-guided projection on materialised filters
// mode 0: acc[0..4] += {H00, H01, H11, C0, C1} (exact integers; the reference accumulates the same integers in doubles, exact below 2^53)
// mode 1: acc[0] += squared error of the projection with xq
template <typename PIX>
__global__ void __launch_bounds__(256)
sgr_flt_proj_kernel(const PIX* __restrict__ src, int ss, const PIX* __restrict__ dat, int ds, const int32_t* __restrict__ f0, int f0s, const int32_t* __restrict__ f1,
                    int f1s, int w, int h, int r0, int r1, int mode, int xq0, int xq1, long long* __restrict__ acc) {
    long long a[5] = {0, 0, 0, 0, 0};
    for (int y = blockIdx.x; y < h; y += gridDim.x)
        for (int x = threadIdx.x; x < w; x += 256) {
            const int d = dat[(size_t)y * ds + x], s = src[(size_t)y * ss + x];
            const int u = d << 4;
            if (mode == 0) {
                const long long sv = (long long)((s << 4) - u);
                const long long v1 = r0 > 0 ? (long long)f0[(size_t)y * f0s + x] - u : 0, v2 = r1 > 0 ? (long long)f1[(size_t)y * f1s + x] - u : 0;
                a[0] += v1 * v1; a[1] += v1 * v2; a[2] += v2 * v2; a[3] += v1 * sv; a[4] += v2 * sv;
            } else {
                int e;
                if (r0 > 0 || r1 > 0) {
                    int v = u << 7;
                    if (r0 > 0) v += xq0 * (f0[(size_t)y * f0s + x] - u);
                    if (r1 > 0) v += xq1 * (f1[(size_t)y * f1s + x] - u);
                    e = ((v + (1 << 10)) >> 11) - s;
                } else
                    e = d - s;
                a[0] += (long long)e * e;
            }
        }
    __shared__ long long part[4][5];
    const int nacc = mode == 0 ? 5 : 1;
    for (int k = 0; k < nacc; k++) {
        const long long t = wave_sum_i64(a[k]);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = t;
    }
    __syncthreads();
    if ((int)threadIdx.x < nacc)
        atomicAdd((unsigned long long*)&acc[threadIdx.x],
                  (unsigned long long)(part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]));
}
// svt_get_proj_subspace_c's solve: every operation an IEEE double operation in the reference's order (-ffp-contract=off)
__global__ void sgr_flt_solve_kernel(const long long* __restrict__ sums, int size, int r0, int r1, int32_t* __restrict__ xq) {
    double H00 = (double)sums[0], H01 = (double)sums[1], H11 = (double)sums[2], C0 = (double)sums[3], C1 = (double)sums[4];
    const double dsize = (double)size;
    H00 /= dsize; H01 /= dsize; H11 /= dsize; C0 /= dsize; C1 /= dsize;
    const double H10 = H01;
    int q0 = 0, q1 = 0;
    if (r0 == 0) { if (!(H11 < 1e-8)) q1 = (int)rint((C1 / H11) * 128.0); }
    else if (r1 == 0) { if (!(H00 < 1e-8)) q0 = (int)rint((C0 / H00) * 128.0); }
    else {
        const double det = H00 * H11 - H01 * H10;
        if (!(det < 1e-8)) {
            const double x0 = (H11 * C0 - H01 * C1) / det, x1 = (H00 * C1 - H10 * C0) / det;
            q0 = (int)rint(x0 * 128.0); q1 = (int)rint(x1 * 128.0);
        }
    }
    xq[0] = q0; xq[1] = q1;
}

// ---- the lossless 4x4 inverse: svt_av1_highbd_iwht4x4_16_add_c / svt_av1_highbd_iwht4x4_1_add_c (Common/Codec/EbInvTransforms.c:2771-2857), selected by eob like
// highbd_iwht4x4_add (:2858-2864).  One thread per block: 16 coefficients (four 16-byte loads), the reversible Walsh-Hadamard butterfly along rows then columns
// (3.5 adds and half a shift per sample, no multiplications), added to the prediction and clipped to the bit depth.  UNIT_QUANT_SHIFT = 2 (EbInvTransforms.h:23).
__device__ __forceinline__ void iwht4(int& a1, int& b1, int& c1, int& d1) {   // in: (a, c, d, b) as the reference names its inputs; out: the four outputs in order
    a1 += c1; d1 -= b1;
    const int e1 = (a1 - d1) >> 1;
    b1 = e1 - b1; c1 = e1 - c1;
    a1 -= b1; d1 += c1;
}
template <typename PIX>
__global__ void __launch_bounds__(64)
iwht4x4_add_kernel(const int32_t* __restrict__ dq, const uint16_t* __restrict__ eob, const PIX* pred, int ps, PIX* recon, int rs, const uint32_t* __restrict__ descs, int n, int bd) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    const uint32_t d = descs[b];
    const int x = d & 0x3FFF, y = (d >> 14) & 0x3FFF, mx = (1 << bd) - 1;
    const PIX* pr = pred + (size_t)y * ps + x; PIX* rc = recon + (size_t)y * rs + x;
    int o[4][4];   // [row][column] of the residual
    if (!eob || eob[b] > 1) {
        const int4* q = (const int4*)(dq + (size_t)b * 16);
#pragma unroll
        for (int i = 0; i < 4; i++) {   // rows: ip[0], ip[1], ip[2], ip[3] play a, c, d, b
            const int4 v = q[i];
            int a1 = v.x >> 2, c1 = v.y >> 2, d1 = v.z >> 2, b1 = v.w >> 2;
            iwht4(a1, b1, c1, d1);
            o[i][0] = a1; o[i][1] = b1; o[i][2] = c1; o[i][3] = d1;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {   // columns
            int a1 = o[0][i], c1 = o[1][i], d1 = o[2][i], b1 = o[3][i];
            iwht4(a1, b1, c1, d1);
            o[0][i] = a1; o[1][i] = b1; o[2][i] = c1; o[3][i] = d1;
        }
    } else {   // DC only
        int a1 = dq[(size_t)b * 16] >> 2;
        int e1 = a1 >> 1;
        a1 -= e1;
        const int t[4] = {a1, e1, e1, e1};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int e = t[i] >> 1, a = t[i] - e;
            o[0][i] = a; o[1][i] = e; o[2][i] = e; o[3][i] = e;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) rc[(size_t)r * rs + c] = (PIX)min(max((int)pr[(size_t)r * ps + c] + o[r][c], 0), mx);
}

}  // namespace

extern "C" {
int svt_hip_launch_quantize_blocks(hipStream_t st, const int32_t* coeff, int n, int nblk, const SvtHipQuantParams* qp, const int16_t* iscan, int32_t* qcoeff,
                                   int32_t* dqcoeff, uint16_t* eob) {
    if (nblk <= 0) return 0;
    hipLaunchKernelGGL(quantize_blocks_kernel, dim3(nblk), dim3(256), 0, st, coeff, n, *qp, iscan, qcoeff, dqcoeff, eob);
    return (int)hipGetLastError();
}
int svt_hip_launch_residual(hipStream_t st, int pix_bytes, const void* src, int ss, const void* pred, int ps, int16_t* res, int rs, int w, int h) {
    if (w <= 0 || h <= 0) return 0;
    dim3 grid((w + 63) / 64, (h + 3) / 4);
    svt_for_pix(pix_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL((residual_kernel<PIX>), grid, dim3(256), 0, st, (const PIX*)src, ss, (const PIX*)pred, ps, res, rs, w, h);
    });
    return (int)hipGetLastError();
}
int svt_hip_launch_ext_all_sad(hipStream_t st, const uint8_t* src, int ss, const uint8_t* ref, int rs, const void* jobs, int n, uint32_t* state) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(ext_all_sad_kernel, dim3(n), dim3(512), 0, st, src, ss, ref, rs, (const SvtHipExtSadJob*)jobs, state);
    return (int)hipGetLastError();
}
int svt_hip_launch_ext_eight_sad_32_64(hipStream_t st, const uint32_t* mvs, int n, uint32_t* state) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(ext_eight_sad_32_64_kernel, dim3(n), dim3(64), 0, st, mvs, state);
    return (int)hipGetLastError();
}
int svt_hip_launch_ext_sad_16(hipStream_t st, const uint8_t* src, int ss, const uint8_t* ref, int rs, const SvtHipExtSadJob* jobs, int n, uint32_t* state) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(ext_sad_16_kernel, dim3(n), dim3(64), 0, st, src, ss, ref, rs, jobs, state);
    return (int)hipGetLastError();
}
int svt_hip_launch_ext_sad_32_64(hipStream_t st, uint32_t* state, const uint32_t* mv, int n) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(ext_sad_32_64_kernel, dim3((n + 63) / 64), dim3(64), 0, st, state, mv, n);
    return (int)hipGetLastError();
}
int svt_hip_launch_interm_var(hipStream_t st, const uint8_t* plane, int stride, const int32_t* offs, int n, uint64_t* mean, uint64_t* mean_sq) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(interm_var_kernel, dim3(n), dim3(64), 0, st, plane, stride, offs, mean, mean_sq);
    return (int)hipGetLastError();
}
int svt_hip_launch_block_mean(hipStream_t st, const uint8_t* plane, int stride, const int32_t* offs, int n, int mode, int w, int h, uint64_t* out) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(block_mean_kernel, dim3(n), dim3(64), 0, st, plane, stride, offs, mode, w, h, out);
    return (int)hipGetLastError();
}
int svt_hip_launch_handle_transform64(hipStream_t st, int tx_size, int32_t* coeff, int nblk, uint64_t* energy) {
    if (nblk <= 0) return 0;
    switch (tx_size) {   // TxSize: 4 TX_64X64, 11 TX_32X64, 12 TX_64X32, 17 TX_16X64, 18 TX_64X16
    case 4:  hipLaunchKernelGGL((handle_transform64_kernel<64, 64>), dim3(nblk), dim3(1024), 0, st, coeff, energy); break;
    case 11: hipLaunchKernelGGL((handle_transform64_kernel<32, 64>), dim3(nblk), dim3(1024), 0, st, coeff, energy); break;
    case 12: hipLaunchKernelGGL((handle_transform64_kernel<64, 32>), dim3(nblk), dim3(1024), 0, st, coeff, energy); break;
    case 17: hipLaunchKernelGGL((handle_transform64_kernel<16, 64>), dim3(nblk), dim3(1024), 0, st, coeff, energy); break;
    case 18: hipLaunchKernelGGL((handle_transform64_kernel<64, 16>), dim3(nblk), dim3(1024), 0, st, coeff, energy); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
int svt_hip_launch_repack64(hipStream_t st, int32_t* coeff, int rows, int per_block, int nblk) {
    if (nblk <= 0) return 0;
    hipLaunchKernelGGL(repack64_kernel, dim3(nblk), dim3(1024), 0, st, coeff, rows, per_block);
    return (int)hipGetLastError();
}
int svt_hip_launch_upsampled_pred(hipStream_t st, const uint8_t* ref, int rs, uint8_t* dst, const void* blks, int n) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(upsampled_pred_kernel, dim3(n), dim3(256), 0, st, ref, rs, dst, (const SvtHipUpsampledBlk*)blks);
    return (int)hipGetLastError();
}
int svt_hip_launch_convolve8(hipStream_t st, int vert, const uint8_t* src, int ss, uint8_t* dst, int ds, const int16_t* filters, int q0, int step, int w, int h) {
    const dim3 grid((w + 63) / 64, (h + 3) / 4);
    if (vert) hipLaunchKernelGGL(convolve8_kernel<true>, grid, dim3(256), 0, st, src, ss, dst, ds, filters, q0, step, w, h);
    else hipLaunchKernelGGL(convolve8_kernel<false>, grid, dim3(256), 0, st, src, ss, dst, ds, filters, q0, step, w, h);
    return (int)hipGetLastError();
}
int svt_hip_launch_wiener_convolve(hipStream_t st, int pix_bytes, int bd, const void* src, int ss, void* dst, int ds, const int16_t* taps, int w, int h, int round0,
                                   int round1) {
    const dim3 grid((w + 63) / 64, (h + 3) / 4);
    const int b = pix_bytes == 1 ? 8 : bd;
    svt_for_pix(pix_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL(wiener_convolve_kernel<PIX>, grid, dim3(256), 0, st, (const PIX*)src, ss, (PIX*)dst, ds, taps, w, h, round0, round1, b);
    });
    return (int)hipGetLastError();
}
int svt_hip_launch_jnt_convolve(hipStream_t st, int pix_bytes, int bd, int variant, const void* src, int ss, void* dst, int ds, uint16_t* cb, int cbs,
                                const int16_t* taps, int w, int h, int round0, int round1, int do_average, int use_jnt, int fwd, int bck) {
    const dim3    grid((w + 63) / 64, (h + 3) / 4);
    const JntArgs a = {variant, w, h, round0, round1, do_average, use_jnt, fwd, bck, pix_bytes == 1 ? 8 : bd};
    svt_for_pix(pix_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL(jnt_convolve_kernel<PIX>, grid, dim3(256), 0, st, (const PIX*)src, ss, (PIX*)dst, ds, cb, cbs, taps, a);
    });
    return (int)hipGetLastError();
}
int svt_hip_launch_diffwtd_mask(hipStream_t st, int elem_bytes, uint8_t* mask, const void* a, int as, const void* b, int bs, int w, int h, int inverse, int round,
                                int shift) {
    const dim3 grid((w * h + 255) / 256);
    svt_for_pix(elem_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL(diffwtd_mask_kernel<PIX>, grid, dim3(256), 0, st, mask, (const PIX*)a, as, (const PIX*)b, bs, w, h, inverse, round, shift);
    });
    return (int)hipGetLastError();
}
int svt_hip_launch_blend_d16(hipStream_t st, int pix_bytes, int bd, void* dst, int ds, const uint16_t* s0, int s0s, const uint16_t* s1, int s1s, const uint8_t* mask,
                             int ms, int w, int h, int subw, int subh, int round0, int round1) {
    const dim3 grid((w + 63) / 64, (h + 3) / 4);
    const int  b = pix_bytes == 1 ? 8 : bd, offset_bits = b + 14 - round0, round_offset = (1 << (offset_bits - round1)) + (1 << (offset_bits - round1 - 1));
    svt_for_pix(pix_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL(blend_d16_kernel<PIX>, grid, dim3(256), 0, st, (PIX*)dst, ds, s0, s0s, s1, s1s, mask, ms, w, h, subw, subh, round_offset, 14 - round0 - round1, b);
    });
    return (int)hipGetLastError();
}
int svt_hip_launch_cdef_dist(hipStream_t st, int pix_bytes, const void* dst, int dstride, const void* src, const uint8_t* list, int n, int bw_log2, int bh_log2,
                             int cs, int pli, uint64_t* out) {
    svt_for_pix(pix_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL(cdef_dist_kernel<PIX>, dim3(1), dim3(256), 0, st, (const PIX*)dst, dstride, (const PIX*)src, list, n, bw_log2, bh_log2, cs, pli, out);
    });
    return (int)hipGetLastError();
}
int svt_hip_launch_sgr_flt_proj(hipStream_t st, int pix_bytes, const void* src, int ss, const void* dat, int ds, const int32_t* f0, int f0s, const int32_t* f1, int f1s,
                                int w, int h, int r0, int r1, int mode, int xq0, int xq1, long long* acc, int32_t* xq_out) {
    const int blocks = h < 256 ? h : 256;
    svt_for_pix(pix_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL(sgr_flt_proj_kernel<PIX>, dim3(blocks), dim3(256), 0, st, (const PIX*)src, ss, (const PIX*)dat, ds, f0, f0s, f1, f1s, w, h, r0, r1, mode, xq0, xq1, acc);
    });
    if (mode == 0) hipLaunchKernelGGL(sgr_flt_solve_kernel, dim3(1), dim3(1), 0, st, acc, w * h, r0, r1, xq_out);
    return (int)hipGetLastError();
}
int svt_hip_launch_iwht4x4_add(hipStream_t st, int pix_bytes, int bd, const int32_t* dq, const uint16_t* eob, const void* pred, int ps, void* recon, int rs, const uint32_t* descs, int n) {
    if (n <= 0) return 0;
    svt_for_pix(pix_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL((iwht4x4_add_kernel<PIX>), dim3((n + 63) / 64), dim3(64), 0, st, dq, eob, (const PIX*)pred, ps, (PIX*)recon, rs, descs, n, bd);
    });
    return (int)hipGetLastError();
}
}

SVT_HIP_TU_PROBE(percall)
