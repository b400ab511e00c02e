// warp_dev.h — the arithmetic of svt_av1_warp_affine_c / svt_av1_highbd_warp_affine_c (Common/Codec/EbWarpedMotion.c:577-694, :733-842) that does not depend on
// where the samples come from or where the result goes: the position of an 8x8 cell's filters, one horizontally filtered sample, one vertical filter sum.
// warp.hip (prediction) and gm.hip (global-motion warp error) both use this one copy of the rounding.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svt_warp {

__device__ __forceinline__ int rp2(int v, int n) { return (v + ((1 << n) >> 1)) >> n; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the filters of the 8x8 cell whose top-left output sample is (j, i): integer position (ix4, iy4) and the 1/65536 phases at the cell's centre
struct Cell { int ix4, iy4, sx4, sy4; };
__device__ __forceinline__ Cell cell_origin(const int32_t* mat, int alpha, int beta, int gamma, int delta, int j, int i, int ss_x, int ss_y) {
    const int src_x = (j + 4) << ss_x, src_y = (i + 4) << ss_y;
    const int dst_x = mat[2] * src_x + mat[3] * src_y + mat[0], dst_y = mat[4] * src_x + mat[5] * src_y + mat[1];
    const int x4 = dst_x >> ss_x, y4 = dst_y >> ss_y;
    Cell c;
    c.ix4 = x4 >> 16; c.iy4 = y4 >> 16;
    c.sx4 = x4 & 0xffff; c.sy4 = y4 & 0xffff;
    c.sx4 += alpha * (-4) + beta * (-4); c.sy4 += gamma * (-4) + delta * (-4);
    c.sx4 &= ~63; c.sy4 &= ~63;
    return c;
}

// horizontally filtered sample (k, l) of the cell, k = -7..7, l = -4..3; fetch(m) = the reference sample at row iy4 + k, column ix4 + l - 3 + m, clamped by the
// caller; filt = Warped_Filters ([193][8]); obh / rbh = offset_bits_horiz / reduce_bits_horiz
template <typename FETCH>
__device__ __forceinline__ int horiz(const Cell& c, int alpha, int beta, int k, int l, const int16_t (*filt)[8], int obh, int rbh, FETCH fetch) {
    const int sx = c.sx4 + beta * (k + 4) + alpha * (l + 4);
    const int16_t* f = filt[rp2(sx, 10) + 64];
    int sum = 1 << obh;
#pragma unroll
    for (int m = 0; m < 8; m++) sum += fetch(m) * (int)f[m];
    return rp2(sum, rbh);
}

// vertical filter sum (before its rounding) of output sample (k, l), k, l = -4..3, over the cell's 15 x 8 horizontally filtered samples
__device__ __forceinline__ int vert(const Cell& c, int gamma, int delta, int k, int l, const int16_t (*filt)[8], int obv, const int* tmp) {
    const int sy = c.sy4 + delta * (k + 4) + gamma * (l + 4);
    const int16_t* f = filt[rp2(sy, 10) + 64];
    int sum = 1 << obv;
#pragma unroll
    for (int m = 0; m < 8; m++) sum += tmp[(k + m + 4) * 8 + (l + 4)] * (int)f[m];
    return sum;
}

}  // namespace svt_warp
