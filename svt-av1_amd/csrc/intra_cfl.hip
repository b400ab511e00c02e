// intra_cfl.hip — chroma-from-luma and filter-intra prediction on gfx950 (wave64), batch forms behind svt_hip_cfl_predict_batch_dev and
// svt_hip_filter_intra_predict_batch_dev.
//
// Replaces (file:line under Source/Lib of the reference):
//   Common/Codec/EbIntraPrediction.c:349-402      svt_cfl_luma_subsampling_420_{lbd,hbd}_c, svt_subtract_average_c (and the CFL_SUB_AVG_FN size wrappers)
//   Common/C_DEFAULT/cfl_c.c                      svt_cfl_predict_{lbd,hbd}_c
//   Common/C_DEFAULT/filterintra_c.c              svt_av1_filter_intra_predictor_c
//   Common/Codec/EbIntraPrediction.c:2492-2539    highbd_filter_intra_predictor
// as cfl_prediction / av1_cost_calc_cfl (Encoder/Codec/EbProductCodingLoop.c:2723-3230) and build_intra_predictors call them.
//
// Mapping, both kernels: a wave owns 8 consecutive jobs and splits its 64 lanes into groups of G = 8, 16, 32 or 64 lanes, one job per group, G the smallest
// group that fits the largest of the eight jobs (read from the descriptors: the host never sees them).  64 / G jobs run side by side, G / 8 rounds finish the
// eight.  A picture tiled with one shape therefore keeps every lane busy for every shape from 16 chroma samples (CfL 4x4: half a group) up; a wave that mixes
// shapes runs at its largest job's width.  G and the round count are wave-uniform, so nothing inside a round diverges but the per-lane "is this strip mine" tests.
//
// CfL: a lane owns strips of 4 chroma samples of one row (8 luma samples of two rows: one 8- / 16-byte load each when the address allows, one 4- / 8-byte
// store).  Strip s of the job is lane s % G's, so a 32x32 block is 4 strips per lane and everything smaller is at most 2; the AC values stay in registers between
// the average (cross-lane butterfly over the group) and the two planes' outputs.  Filter-intra: 8 lanes per 4x2 patch, one lane per output sample; the patches
// of one anti-diagonal pr + pc are independent (a patch reads the patches above-left, above and left of it), at most min(H / 2, W / 4) <= 8 of them, and a job
// takes H / 2 + W / 4 - 1 steps on its (H + 1) x (W + 1) working tile in LDS.  A tile belongs to one wave: the steps are ordered by wavefront fences, no barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "lane_reduce.h"
#include "intra_dev.h"
#include "filter_intra_taps.h"

namespace {

using namespace intra;

constexpr int EDGE_REC = 160, EDGE_ORG = 16;   // one edge of a record, element of sample 0 (intra.hip)
constexpr int WAVE_JOBS = 8, WG_WAVES = 4, WG_JOBS = WAVE_JOBS * WG_WAVES;
constexpr int CFL_BUF_LINE = 32;               // row stride of pred_buf_q3, and of a d_ac slot
// Samples of LDS per wave: a group of G lanes gets FI_SLOT * G / 8 of them.  The largest tile of each group size -- G = 8: 4x16 (17 x 5 = 85), 16: 8x32
// (33 x 9 = 297), 32: 16x32 (33 x 17 = 561), 64: 32x32 (33 x 33 = 1089) -- fits 149, 298, 596, 1192.
constexpr int FI_SLOT = 149, FI_WAVE_TILE = FI_SLOT * 8;

static __device__ const int8_t kFilterIntraTaps[5][8][8] __attribute__((aligned(8))) = {SVT_FILTER_INTRA_TAPS_TABLE};

// ROUND_POWER_OF_TWO_SIGNED
IPD int round_signed(int v, int n) { return v < 0 ? -((-v + (1 << (n - 1))) >> n) : (v + (1 << (n - 1))) >> n; }

// The group size of a wave whose lanes each hold the lane count one of its jobs needs.
IPD int wave_group(int need) { return __any(need > 32) ? 64 : (__any(need > 16) ? 32 : (__any(need > 8) ? 16 : 8)); }

IPD int group_sum(int v, int G) {
    v += lane_xor(v, 1); v += lane_xor(v, 2); v += lane_xor(v, 4);
    if (G >= 16) v += lane_xor(v, 8);
    if (G >= 32) v += lane_xor(v, 16);
    if (G >= 64) v += lane_xor(v, 32);
    return v;
}

// LDS written by some lanes of this wave is read by others: keeps the compiler from moving accesses across, the hardware runs one wave's LDS operations in order
IPD void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }

// ---- n consecutive samples, as one wide access where the address allows
IPD void load8(const uint8_t* p, int v[8]) {
    if (((uintptr_t)p & 7) == 0) {
        const uint2 w = *(const uint2*)p;
#pragma unroll
        for (int i = 0; i < 4; i++) { v[i] = (w.x >> (8 * i)) & 255; v[4 + i] = (w.y >> (8 * i)) & 255; }
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = p[i];
    }
}
IPD void load8(const uint16_t* p, int v[8]) {
    if (((uintptr_t)p & 15) == 0) {
        const uint4 w = *(const uint4*)p;
        v[0] = w.x & 0xffff; v[1] = w.x >> 16; v[2] = w.y & 0xffff; v[3] = w.y >> 16; v[4] = w.z & 0xffff; v[5] = w.z >> 16; v[6] = w.w & 0xffff; v[7] = w.w >> 16;
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = p[i];
    }
}
IPD void load4(const uint8_t* p, int v[4]) {
    if (((uintptr_t)p & 3) == 0) {
        const uint32_t w = *(const uint32_t*)p;
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = (w >> (8 * i)) & 255;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = p[i];
    }
}
IPD void load4(const uint16_t* p, int v[4]) {
    if (((uintptr_t)p & 7) == 0) {
        const uint2 w = *(const uint2*)p;
        v[0] = w.x & 0xffff; v[1] = w.x >> 16; v[2] = w.y & 0xffff; v[3] = w.y >> 16;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = p[i];
    }
}
IPD void store4(uint8_t* p, const int v[4]) {
    if (((uintptr_t)p & 3) == 0) *(uint32_t*)p = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    else {
#pragma unroll
        for (int i = 0; i < 4; i++) p[i] = (uint8_t)v[i];
    }
}
IPD void store4(uint16_t* p, const int v[4]) {
    if (((uintptr_t)p & 7) == 0) *(uint2*)p = make_uint2((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16));
    else {
#pragma unroll
        for (int i = 0; i < 4; i++) p[i] = (uint16_t)v[i];
    }
}

// ================================================================================================ chroma from luma
// Strips of 4 chroma samples a job has; 0 = a job that writes nothing (descriptors live in device memory: checked before anything indexes a table)
IPD int cfl_strips(const SvtHipCflJob& J) {
    if (J.tx_size >= N_TX_SIZES || J.alpha_q3[0] < -16 || J.alpha_q3[0] > 16 || J.alpha_q3[1] < -16 || J.alpha_q3[1] > 16) return 0;
    const int bw = kTxW[J.tx_size], bh = kTxH[J.tx_size];
    return bw > 32 || bh > 32 ? 0 : (bw * bh) >> 2;
}

template <typename PIX>
__global__ __launch_bounds__(64 * WG_WAVES) void cfl_predict_batch_kernel(const PIX* __restrict__ luma, int luma_stride, const PIX* __restrict__ edges,
                                                                         const SvtHipCflJob* __restrict__ jobs, int njobs, int bd, PIX* cb, PIX* cr, int chroma_stride,
                                                                         int16_t* __restrict__ ac_out) {
    const int lane = threadIdx.x & 63;
    const int base = (blockIdx.x * WG_WAVES + (threadIdx.x >> 6)) * WAVE_JOBS;
    if (base >= njobs) return;   // the whole wave
    int need = 0;
    if (base + (lane >> 3) < njobs) need = cfl_strips(jobs[base + (lane >> 3)]);
    const int G = wave_group(need), lg = 31 - __clz(G), l = lane & (G - 1);
    const bool ac_wide = ((uintptr_t)ac_out & 7) == 0;

    for (int it = 0; it < WAVE_JOBS; it += 64 >> lg) {
        const int ji = base + it + (lane >> lg);
        const bool live = ji < njobs;
        const SvtHipCflJob J = jobs[live ? ji : base];
        const int strips = live ? cfl_strips(J) : 0;
        if (!__any(strips != 0)) continue;
        const int tx = strips ? J.tx_size : 0;   // a group without work computes on the 4x4 shape and stores nothing
        const int bw = kTxW[tx], bh = kTxH[tx];
        const int wq = bw >> 2, lq = 31 - __clz(wq);

        // ---- luma: (a + b + c + d) << 1 per chroma sample, the strips of this lane in registers
        const PIX* lp = luma + (ptrdiff_t)J.luma_y * luma_stride + J.luma_x;
        int ac[4][4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int s = k * G + l;
#pragma unroll
            for (int i = 0; i < 4; i++) ac[k][i] = 0;
            if (s < strips) {
                const int r = s >> lq, c = (s & (wq - 1)) << 2;
                int t[8], b[8];
                const PIX* p = lp + (ptrdiff_t)(2 * r) * luma_stride + 2 * c;
                load8(p, t); load8(p + luma_stride, b);
#pragma unroll
                for (int i = 0; i < 4; i++) { ac[k][i] = (t[2 * i] + t[2 * i + 1] + b[2 * i] + b[2 * i + 1]) << 1; sum += ac[k][i]; }
            }
        }
        // ---- svt_subtract_average: at most 1024 samples of at most 8184 each, the sum fits 24 bits
        const int n = bw * bh, avg = (group_sum(sum, G) + (n >> 1)) >> (31 - __clz(n));
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int s = k * G + l;
            if (s < strips) {
                const int r = s >> lq, c = (s & (wq - 1)) << 2;
#pragma unroll
                for (int i = 0; i < 4; i++) ac[k][i] -= avg;
                if (ac_out) {
                    int16_t* a = ac_out + (size_t)ji * (CFL_BUF_LINE * CFL_BUF_LINE) + r * CFL_BUF_LINE + c;
                    if (ac_wide) *(uint2*)a = make_uint2((uint32_t)(uint16_t)ac[k][0] | ((uint32_t)(uint16_t)ac[k][1] << 16), (uint32_t)(uint16_t)ac[k][2] | ((uint32_t)(uint16_t)ac[k][3] << 16));
                    else {
#pragma unroll
                        for (int i = 0; i < 4; i++) a[i] = (int16_t)ac[k][i];
                    }
                }
            }
        }
        // ---- the DC predictors of the two edge records: lane i of the group adds above[i] and left[i], both sums in one word (each at most 32 * 1023)
        int dc[2] = {0, 0};
        const bool from_edges = strips && J.dc_from_edges;
        if (__any(from_edges)) {
#pragma unroll
            for (int pl = 0; pl < 2; pl++) {
                int packed = 0;
                if (from_edges && ((J.plane_mask >> pl) & 1) && (pl ? cr : cb)) {
                    const PIX* e = edges + J.edge_off[pl];
                    if (l < bw) packed = e[EDGE_ORG + l];
                    if (l < bh) packed += (int)e[EDGE_REC + EDGE_ORG + l] << 16;
                }
                packed = group_sum(packed, G);
                dc[pl] = dc_value(packed & 0xffff, (int)((uint32_t)packed >> 16), bw, bh, J.dc_have & 1, (J.dc_have >> 1) & 1, bd);
            }
        }
        // ---- svt_cfl_predict: clip(pred + ROUND_POWER_OF_TWO_SIGNED(alpha * ac, 6))
#pragma unroll
        for (int pl = 0; pl < 2; pl++) {
            PIX* plane = pl ? cr : cb;
            if (!plane || !((J.plane_mask >> pl) & 1)) continue;
            const int alpha = J.alpha_q3[pl];
            PIX* dp = plane + (ptrdiff_t)J.dst_y * chroma_stride + J.dst_x;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int s = k * G + l;
                if (s < strips) {
                    const int r = s >> lq, c = (s & (wq - 1)) << 2;
                    PIX* d = dp + (ptrdiff_t)r * chroma_stride + c;
                    int p[4];
                    if (J.dc_from_edges) { p[0] = p[1] = p[2] = p[3] = dc[pl]; }
                    else load4(d, p);
#pragma unroll
                    for (int i = 0; i < 4; i++) p[i] = clip_px((int)(int16_t)p[i] + round_signed(alpha * ac[k][i], 6), bd);
                    store4(d, p);
                }
            }
        }
    }
}

// ================================================================================================ filter-intra
// Lanes a job needs: 8 per patch of its longest anti-diagonal; 0 = a job that writes nothing
IPD int fi_lanes(const SvtHipFilterIntraJob& J) {
    if (J.tx_size >= N_TX_SIZES || J.mode > 4) return 0;
    const int bw = kTxW[J.tx_size], bh = kTxH[J.tx_size];
    return bw > 32 || bh > 32 ? 0 : 8 * min(bh >> 1, bw >> 2);
}

template <typename PIX>
__global__ __launch_bounds__(64 * WG_WAVES) void filter_intra_batch_kernel(const PIX* __restrict__ edges, const SvtHipFilterIntraJob* __restrict__ jobs, int njobs, int bd,
                                                                          PIX* __restrict__ dst, int dst_stride) {
    __shared__ uint16_t tiles[WG_WAVES][FI_WAVE_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int base = (blockIdx.x * WG_WAVES + wave) * WAVE_JOBS;
    if (base >= njobs) return;   // the whole wave; no workgroup barrier follows
    int need = 0;
    if (base + (lane >> 3) < njobs) need = fi_lanes(jobs[base + (lane >> 3)]);
    const int G = wave_group(need), lg = 31 - __clz(G), l = lane & (G - 1);
    uint16_t* buf = tiles[wave] + (lane >> lg) * (FI_SLOT * (G >> 3));
    const int q = l >> 3, k = l & 7;   // patch of the diagonal, output sample of the patch

    for (int it = 0; it < WAVE_JOBS; it += 64 >> lg) {
        const int ji = base + it + (lane >> lg);
        const bool live = ji < njobs;
        const SvtHipFilterIntraJob J = jobs[live ? ji : base];
        const bool ok = live && fi_lanes(J) != 0;
        if (!__any(ok)) continue;
        const int tx = ok ? J.tx_size : 0;
        const int bw = kTxW[tx], bh = kTxH[tx], S = bw + 1;   // tile: row 0 = above[-1 .. bw - 1], column 0 = left, row stride S
        wave_sync();   // the previous round's tile has been copied out
        if (ok) {
            const PIX* e = edges + J.edge_off;
            for (int i = l; i < bw + 1 + bh; i += G) {
                if (i <= bw) buf[i] = e[EDGE_ORG - 1 + i];
                else buf[(i - bw) * S] = e[EDGE_REC + EDGE_ORG + i - bw - 1];
            }
        }
        int t[8];
        {
            const uint2 w = *(const uint2*)kFilterIntraTaps[ok ? J.mode : 0][k];
#pragma unroll
            for (int i = 0; i < 4; i++) { t[i] = (int8_t)(w.x >> (8 * i)); t[4 + i] = (int8_t)(w.y >> (8 * i)); }
        }
        const int PR = bh >> 1, PC = bw >> 2, steps = ok ? PR + PC - 1 : 0;
        for (int d = 0; __any(d < steps); d++) {
            wave_sync();
            const int pr = max(0, d - (PC - 1)) + q, pc = d - pr;
            if (d < steps && pr < PR && pc >= 0) {
                const int r = 1 + 2 * pr, c = 1 + 4 * pc;
                const uint16_t* up = buf + (r - 1) * S + c - 1;
                int v = t[0] * up[0] + t[1] * up[1] + t[2] * up[2] + t[3] * up[3] + t[4] * up[4] + t[5] * up[S] + t[6] * up[2 * S];
                buf[(r + (k >> 2)) * S + c + (k & 3)] = (uint16_t)clip_px(round_signed(v, 4), bd);
            }
        }
        wave_sync();
        if (ok) {
            PIX* dp = dst + (ptrdiff_t)J.dst_y * dst_stride + J.dst_x;
            const int wq = bw >> 2, lq = 31 - __clz(wq);
            for (int s = l; s < ((bw * bh) >> 2); s += G) {
                const int r = s >> lq, c = (s & (wq - 1)) << 2;
                const uint16_t* b = buf + (r + 1) * S + 1 + c;
                const int v[4] = {b[0], b[1], b[2], b[3]};
                store4(dp + (ptrdiff_t)r * dst_stride + c, v);
            }
        }
    }
}

}  // namespace

extern "C" int svt_hip_launch_cfl_predict(hipStream_t st, int pix_bytes, int bd, const void* luma, int luma_stride, const void* edges, const SvtHipCflJob* jobs,
                                          int njobs, void* cb, void* cr, int chroma_stride, int16_t* ac) {
    if (njobs <= 0) return 0;
    const dim3 grid((njobs + WG_JOBS - 1) / WG_JOBS), block(64 * WG_WAVES);
    svt_for_pix(pix_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL(cfl_predict_batch_kernel<PIX>, grid, block, 0, st, (const PIX*)luma, luma_stride, (const PIX*)edges, jobs, njobs, bd, (PIX*)cb, (PIX*)cr,
                           chroma_stride, ac);
    });
    return (int)hipGetLastError();
}

extern "C" int svt_hip_launch_filter_intra_predict(hipStream_t st, int pix_bytes, int bd, const void* edges, const SvtHipFilterIntraJob* jobs, int njobs, void* dst,
                                                   int dst_stride) {
    if (njobs <= 0) return 0;
    const dim3 grid((njobs + WG_JOBS - 1) / WG_JOBS), block(64 * WG_WAVES);
    svt_for_pix(pix_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL(filter_intra_batch_kernel<PIX>, grid, block, 0, st, (const PIX*)edges, jobs, njobs, bd, (PIX*)dst, dst_stride);
    });
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(intra_cfl)
