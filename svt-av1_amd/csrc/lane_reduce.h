// lane_reduce.h — reductions over the lanes of a wave (64 lanes, four rows of 16) shared by the kernel units; device code only.  docs/design/kernels-overview.md,
// "Lane reductions": which one to reach for, and the sites that keep a form of their own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#if defined(__HIPCC__)
// DPP controls (the dpp_ctrl operand of a VALU instruction; a row is 16 lanes, a quad 4)
constexpr int DPP_QUAD_SWAP1      = 0xB1;    // quad_perm [1,0,3,2]: lane i reads lane i ^ 1
constexpr int DPP_QUAD_SWAP2      = 0x4E;    // quad_perm [2,3,0,1]: lane i reads lane i ^ 2
constexpr int DPP_ROW_HALF_MIRROR = 0x141;   // row_half_mirror: lane i of an 8-lane half row reads lane 7 - i of that half
constexpr int DPP_ROW_MIRROR      = 0x140;   // row_mirror: lane i of a row reads lane 15 - i of that row
constexpr int DPP_ROW_BCAST15     = 0x142;   // row_bcast:15: lane 15 of every row is read by all lanes of the next row
constexpr int DPP_ROW_BCAST31     = 0x143;   // row_bcast:31: lane 31 is read by all lanes of rows 2 and 3
constexpr int DPP_ROW_ROR4        = 0x124;   // row_ror:4: lane i of a row reads lane (i + 4) & 15 of that row
constexpr int DPP_ROW_ROR8        = 0x128;   // row_ror:8: lane i of a row reads lane (i + 8) & 15 of that row
// ---- one 16-lane row: the result in every lane of the row.  The total (wraps like any 32-bit add) takes four steps and no LDS: after the two quad swaps every
// lane holds its quad's total, after row_half_mirror its half row's, after row_mirror its row's.  A lane that is switched off counts as 0 (bound_ctrl).
__device__ __forceinline__ int row16_sum(int v) {
    v += __builtin_amdgcn_mov_dpp(v, DPP_QUAD_SWAP1, 0xF, 0xF, true);
    v += __builtin_amdgcn_mov_dpp(v, DPP_QUAD_SWAP2, 0xF, 0xF, true);
    v += __builtin_amdgcn_mov_dpp(v, DPP_ROW_HALF_MIRROR, 0xF, 0xF, true);
    v += __builtin_amdgcn_mov_dpp(v, DPP_ROW_MIRROR, 0xF, 0xF, true);
    return v;
}
__device__ __forceinline__ uint32_t row16_sum(uint32_t v) { return (uint32_t)row16_sum((int)v); }
// The row minimum.  A lane that is switched off leaves its reader's own value in place (old = v), so it never wins.
__device__ __forceinline__ uint32_t row16_min(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, DPP_QUAD_SWAP1, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, DPP_QUAD_SWAP2, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, DPP_ROW_HALF_MIRROR, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, DPP_ROW_MIRROR, 0xF, 0xF, false));
    return v;
}
// The row total of p0 + p1 as a 64-bit value, for any int32 p0, p1: the low 16 bits (32 values < 2^16) and the signed upper halves (32 values of magnitude
// <= 2^15) are reduced separately, so neither 32-bit sum can wrap.
__device__ __forceinline__ long long row16_sum_wide(int32_t p0, int32_t p1) {
    const int32_t lo = row16_sum((p0 & 0xFFFF) + (p1 & 0xFFFF));
    const int32_t hi = row16_sum((p0 >> 16) + (p1 >> 16));
    return (long long)hi * 65536 + lo;
}
// ---- the four rows of a wave: v holds a row result in every lane of its row; lanes 0, 16, 32, 48 are read through scalar registers.  Wave-uniform results. ----
__device__ __forceinline__ uint32_t rows_total(uint32_t v) {
    return (uint32_t)(__builtin_amdgcn_readlane((int)v, 0) + __builtin_amdgcn_readlane((int)v, 16) + __builtin_amdgcn_readlane((int)v, 32) + __builtin_amdgcn_readlane((int)v, 48));
}
__device__ __forceinline__ uint32_t rows_min(uint32_t v) {
    const uint32_t a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16), c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    return min(min(a, b), min(c, d));
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) { return rows_total(row16_sum(v)); }   // wraps like any 32-bit add
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return rows_min(row16_min(v)); }
// ---- xor butterflies: any group size, integers of 32 or 64 bits, the result in every lane of the group ------------------------------------------------
// v of lane (own lane ^ m).  A shuffle moves 32 bits: the halves of a 64-bit value travel apart, the high one first.
template <typename T> __device__ __forceinline__ T lane_xor(T v, int m) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "32- and 64-bit integers");
    if constexpr (sizeof(T) == 4) return (T)__shfl_xor((int)v, m, 64);
    else return (T)(((uint64_t)(uint32_t)__shfl_xor((int)((uint64_t)v >> 32), m, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64));
}
// Sum (wraps) / maximum over the aligned group of G lanes, G a power of two <= 64, that a lane belongs to.
template <int G, typename T> __device__ __forceinline__ T lanes_sum(T v) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v += lane_xor(v, m);
    return v;
}
template <int G, typename T> __device__ __forceinline__ T lanes_max(T v) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v = max(v, lane_xor(v, m));
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) { return lanes_sum<64>(v); }   // the 64-lane sum, in every lane
__device__ __forceinline__ long long wave_sum_i64(long long v) { return lanes_sum<64>(v); }
#endif
