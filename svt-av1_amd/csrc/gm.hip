// gm.hip — global motion on the device: the warp error of integer models over a whole picture, the plain frame error, svt_get_shear_params, and the state machine of
// the parameter refinement; gfx950, 8-bit luma.  docs/kernels/gm.md.
//
// Replaces (file:line under /root/reference/Source/Lib): Encoder/Codec/EbEncWarpedMotion.c:171-211, :227-264 svt_av1_warp_error / warp_error (8-bit path) with
// svt_warp_plane + svt_av1_warp_affine_c (Common/Codec/EbWarpedMotion.c:577-728) fused into the sum; :160-169, :213-225 svt_av1_calc_frame_error_c /
// svt_av1_frame_error; Common/Codec/EbWarpedMotion.c:921-950 svt_get_shear_params; Encoder/Codec/global_motion.c:135-259 svt_av1_refine_integerized_param.
//
// gm_warp_error_kernel: one workgroup per (32x32 error block, candidate, job).  The reference window of the block (48 x 48 samples around where the block's centre
// lands, clamped to the plane as the filter's own reads are) is staged in LDS once; each of the 4 waves then takes 4 of the block's sixteen 8x8 cells: 15 x 8
// horizontally filtered samples through a per-wave LDS tile, then 64 lanes produce the 8 x 8 warped samples, look the difference to the source up in the 512-entry
// error table (LDS) and keep a u32 partial.  A block whose cells reach outside the staged window (models far beyond what the bitstream can carry, or a window of
// which only the clamp is left) reads global memory with the reference's clamps instead; the choice is uniform over the workgroup.  Nothing is written but one
// 64-bit atomic add per workgroup: integer sums are exact in any order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "warp_filter_table.h"
#include "warp_dev.h"
#include "gm_walk.h"

namespace {

using svt_warp::rp2;
using svt_warp::clampi;

__device__ const int16_t kWarpedFilterGm[193][8] = SVT_WARPED_FILTER_TABLE;

constexpr int WIN = 48;            // staged window: rows and columns of samples
constexpr int WIN_DW = 13;         // dwords per staged row (52 bytes: an unaligned 8-byte read may touch 3 dwords; odd dword stride)
constexpr int WIN_ORG = 24;        // the block centre's integer position sits at row / column WIN_ORG of the window

struct GmRefTab { SvtHipGmRef r[SVT_HIP_GM_MAX_REFS]; };

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// cands: [job][cand_stride]; jobs (may be NULL: reference 0) gives the job's reference plane; n_live (may be NULL: n_cand) its live batch size.
__global__ void __launch_bounds__(256)
gm_warp_error_kernel(const uint8_t* __restrict__ src, int src_stride, int w, int h, GmRefTab refs, const SvtHipGmModel* __restrict__ cands, int cand_stride, int cand0,
                     int n_cand, const SvtHipGmJob* __restrict__ jobs, const int* __restrict__ n_live, const uint16_t* __restrict__ lut_g,
                     unsigned long long* __restrict__ d_err) {
    constexpr int obh = 14, rbh = 3, obv = 19, rbv = 11;   // bd 8, round_0 3, not compound
    __shared__ int16_t filt[193][8];
    __shared__ uint16_t lut[512];
    __shared__ uint32_t win[WIN * WIN_DW];
    __shared__ int tmp[4][15 * 8];
    __shared__ unsigned wg_sum;
    __shared__ int outside;
    const int job = blockIdx.z, ci = cand0 + blockIdx.y;
    if (ci >= (n_live ? n_live[job] : n_cand)) return;
    const SvtHipGmModel b = cands[(size_t)job * cand_stride + ci];
    unsigned long long* out = d_err + (size_t)job * cand_stride + ci;
    // svt_av1_warp_error: if (!svt_get_shear_params(wm)) return 1;  A model flagged valid whose shear parameters is_affine_shear_allowed would refuse is treated the
    // same way: the bound is what keeps every filter index inside Warped_Filters.
    if (!b.valid || 4 * abs((int)b.alpha) + 7 * abs((int)b.beta) >= (1 << 16) || 4 * abs((int)b.gamma) + 4 * abs((int)b.delta) >= (1 << 16)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(out, 1ull);
        return;
    }
    const SvtHipGmRef rp = refs.r[jobs ? jobs[job].ref : 0];
    const uint8_t* __restrict__ ref = rp.d_plane;
    const int width = rp.width, height = rp.height, stride = rp.stride;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nbx = (w + 31) >> 5;
    const int j0 = 32 * (blockIdx.x % nbx), i0 = 32 * (blockIdx.x / nbx);
    const int bw = min(32, w - j0), bh = min(32, h - i0);
    const int ncx = (bw + 7) >> 3, ncy = (bh + 7) >> 3;

    for (int i = tid; i < 193 * 8; i += 256) (&filt[0][0])[i] = (&kWarpedFilterGm[0][0])[i];
    for (int i = tid; i < 512; i += 256) lut[i] = lut_g[i];
    if (tid == 0) { wg_sum = 0; outside = 0; }
    // window origin: where the block's centre lands (the filter position of a cell centred there), minus WIN_ORG
    const svt_warp::Cell cc = svt_warp::cell_origin(b.mat, b.alpha, b.beta, b.gamma, b.delta, j0 + 12, i0 + 12, 0, 0);
    const int wx0 = cc.ix4 - WIN_ORG, wy0 = cc.iy4 - WIN_ORG;
    __syncthreads();
    if (tid < ncx * ncy) {
        const svt_warp::Cell c = svt_warp::cell_origin(b.mat, b.alpha, b.beta, b.gamma, b.delta, j0 + 8 * (tid % ncx), i0 + 8 * (tid / ncx), 0, 0);
        const int x = c.ix4 - wx0, y = c.iy4 - wy0;   // |ix4|, |iy4| <= 2^15: no overflow
        if (x - 7 < 0 || x + 7 >= WIN || y - 7 < 0 || y + 7 >= WIN) outside = 1;
    }
    __syncthreads();
    const bool staged = !outside;
    if (staged) {
        // rows of 48 samples as 12 dwords (+ 1 unused): 576 dwords, clamped like the filter's reads
        for (int i = tid; i < WIN * 12; i += 256) {
            const int r = i / 12, c4 = (i % 12) * 4;
            const uint8_t* row = ref + (ptrdiff_t)clampi(wy0 + r, 0, height - 1) * stride;
            uint32_t v = 0;
#pragma unroll
            for (int t = 0; t < 4; t++) v |= (uint32_t)row[clampi(wx0 + c4 + t, 0, width - 1)] << (8 * t);
            win[r * WIN_DW + (i % 12)] = v;
        }
        if (tid < WIN) win[tid * WIN_DW + 12] = 0;
    }
    __syncthreads();

    unsigned part = 0;
    for (int sb = wave; sb < ncx * ncy; sb += 4) {
        const int j = j0 + 8 * (sb % ncx), i = i0 + 8 * (sb / ncx);
        const svt_warp::Cell cell = svt_warp::cell_origin(b.mat, b.alpha, b.beta, b.gamma, b.delta, j, i, 0, 0);
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int idx = lane + 64 * r;
            if (idx < 120) {
                const int k = (idx >> 3) - 7, l = (idx & 7) - 4;
                if (staged) {
                    const int x0 = cell.ix4 + l - 3 - wx0;                       // 0 .. WIN - 8
                    const uint32_t* p = win + (cell.iy4 + k - wy0) * WIN_DW + (x0 >> 2);
                    const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
                    const int sh = 8 * (x0 & 3);
                    const uint32_t lo = (uint32_t)(((uint64_t)d1 << 32 | d0) >> sh), hi = (uint32_t)(((uint64_t)d2 << 32 | d1) >> sh);
                    tmp[wave][idx] = svt_warp::horiz(cell, b.alpha, b.beta, k, l, filt, obh, rbh,
                                                     [&](int m) { return (int)(((m < 4 ? lo : hi) >> (8 * (m & 3))) & 0xff); });
                } else {
                    const uint8_t* row = ref + (ptrdiff_t)clampi(cell.iy4 + k, 0, height - 1) * stride;
                    const int ix = cell.ix4 + l - 3;
                    tmp[wave][idx] = svt_warp::horiz(cell, b.alpha, b.beta, k, l, filt, obh, rbh, [&](int m) { return (int)row[clampi(ix + m, 0, width - 1)]; });
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's LDS writes have landed
        {
            const int k = (lane >> 3) - 4, l = (lane & 7) - 4;
            if (i + k + 4 < i0 + bh && j + l + 4 < j0 + bw) {
                const int sum = svt_warp::vert(cell, b.gamma, b.delta, k, l, filt, obv, tmp[wave]);
                const int pix = clampi(rp2(sum, rbv) - (1 << 7) - (1 << 8), 0, 255);
                const int s = src[(ptrdiff_t)(i + k + 4) * src_stride + (j + l + 4)];
                part += lut[255 + s - pix];
            }
        }
        __builtin_amdgcn_wave_barrier();      // the tile is rewritten by the next cell
    }
    part = wave_sum(part);
    if (lane == 0) atomicAdd(&wg_sum, part);
    __syncthreads();
    if (tid == 0) atomicAdd(out, (unsigned long long)wg_sum);
}

// svt_av1_calc_frame_error_c of up to 8 planes: blockIdx.x = a band of 8 rows, blockIdx.y = the plane
__global__ void __launch_bounds__(256)
gm_frame_error_kernel(const uint8_t* __restrict__ src, int src_stride, int w, int h, GmRefTab refs, const uint16_t* __restrict__ lut_g,
                      unsigned long long* __restrict__ d_err) {
    __shared__ uint16_t lut[512];
    const int tid = threadIdx.x;
    for (int i = tid; i < 512; i += 256) lut[i] = lut_g[i];
    __syncthreads();
    const SvtHipGmRef rp = refs.r[blockIdx.y];
    const int y0 = 8 * blockIdx.x, y1 = min(h, y0 + 8);
    unsigned long long part = 0;   // a lane sees at most 8 rows x (w / 256) samples of 2^14, the wave 64 times that: 64 bits once, no bound on w
    for (int y = y0; y < y1; y++) {
        const uint8_t* a = src + (ptrdiff_t)y * src_stride;
        const uint8_t* r = rp.d_plane + (ptrdiff_t)y * rp.stride;
        for (int x = tid; x < w; x += 256) part += lut[255 + (int)a[x] - (int)r[x]];
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) part += __shfl_down(part, o, 64);
    if ((tid & 63) == 0) atomicAdd(d_err + blockIdx.y, part);
}

__global__ void __launch_bounds__(256) gm_shear_params_kernel(const int32_t* __restrict__ wmmat, int n, SvtHipGmModel* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t m[6];
    for (int k = 0; k < 6; k++) m[k] = wmmat[(size_t)i * 6 + k];
    SvtHipGmModel o;
    gm_shear_params(m, &o);
    for (int k = 0; k < 6; k++) o.mat[k] = m[k];
    out[i] = o;
}

// The walk's state machine: one wave per job, lane 0 walks the (serial) chain; first = the call's first launch (no errors to read yet).
// Scratch layout (svt_hip_gm_refine_scratch_bytes): states, candidates [job][GM_NC], errors [job][GM_NC], live batch sizes [job], the done counter.
__global__ void __launch_bounds__(64)
gm_refine_step_kernel(const SvtHipGmJob* __restrict__ jobs, int n_refs, GmState* __restrict__ states, SvtHipGmModel* __restrict__ cands, long long* __restrict__ err,
                      int* __restrict__ n_live, int* __restrict__ done_count, SvtHipGmResult* __restrict__ results, int first) {
    __shared__ GmState st;
    __shared__ SvtHipGmModel c[GM_NC];
    __shared__ long long e[GM_NC];
    __shared__ SvtHipGmResult res;
    static_assert(sizeof(GmState) % 4 == 0 && sizeof(SvtHipGmModel) % 4 == 0 && sizeof(SvtHipGmResult) % 4 == 0, "copied as dwords");
    const int job = blockIdx.x, lane = threadIdx.x;
    if (!first) {
        if (states[job].done) return;   // uniform
        for (int k = lane; k < (int)(sizeof(GmState) / 4); k += 64) ((int*)&st)[k] = ((const int*)(states + job))[k];
        if (lane < GM_NC) e[lane] = err[(size_t)job * GM_NC + lane];
    }
    __syncthreads();
    if (lane == 0) {
        if (first) {
            const SvtHipGmJob j = jobs[job];
            gm_job_start(&st, &j, j.ref >= 0 && j.ref < n_refs, c, &res);
        } else {
            gm_job_step(&st, (const int64_t*)e, c, &res);
        }
        if (st.done) atomicAdd(done_count, 1);
        n_live[job] = st.n_live;
    }
    __syncthreads();
    for (int k = lane; k < (int)(sizeof(GmState) / 4); k += 64) ((int*)(states + job))[k] = ((const int*)&st)[k];
    if (st.done) {
        for (int k = lane; k < (int)(sizeof(SvtHipGmResult) / 4); k += 64) ((int*)(results + job))[k] = ((const int*)&res)[k];
    } else {
        for (int k = lane; k < st.n_live * (int)(sizeof(SvtHipGmModel) / 4); k += 64) ((int*)(cands + (size_t)job * GM_NC))[k] = ((const int*)c)[k];
    }
    if (lane < GM_NC) err[(size_t)job * GM_NC + lane] = 0;
}

}  // namespace

extern "C" const uint16_t* svt_hip_gm_error_lut_host() {
    // function-local static: built once, thread-safe.  min(16384, floor(16384 (|i - 255| / 255)^0.7 + 0.5))
    static const struct Lut { uint16_t v[512]; Lut() { for (int i = 0; i < 512; i++) { const double t = floor(16384.0 * pow(abs(i - 255) / 255.0, 0.7) + 0.5); v[i] = (uint16_t)(t > 16384.0 ? 16384.0 : t); } } } lut;
    return lut.v;
}

static GmRefTab ref_tab(const SvtHipGmRef* refs, int n) {
    GmRefTab t = {};
    for (int i = 0; i < n && i < SVT_HIP_GM_MAX_REFS; i++) t.r[i] = refs[i];
    return t;
}

extern "C" int svt_hip_launch_gm_shear_params(hipStream_t st, const int32_t* wmmat, int n, SvtHipGmModel* out) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(gm_shear_params_kernel, dim3((n + 255) / 256), dim3(256), 0, st, wmmat, n, out);
    return (int)hipGetLastError();
}

// d_err is zeroed here (stream-ordered) before the sums are added
extern "C" int svt_hip_launch_gm_warp_error(hipStream_t st, const uint8_t* src, int src_stride, int w, int h, const SvtHipGmRef* ref, const SvtHipGmModel* models, int n,
                                            const uint16_t* d_lut, int64_t* d_err) {
    if (n <= 0) return 0;
    hipError_t e = hipMemsetAsync(d_err, 0, (size_t)n * 8, st);
    if (e != hipSuccess) return (int)e;
    const int nblk = ((w + 31) >> 5) * ((h + 31) >> 5);
    const GmRefTab t = ref_tab(ref, 1);
    for (int c0 = 0; c0 < n; c0 += 32768) {   // grid.y is 16 bits wide
        const int nc = n - c0 < 32768 ? n - c0 : 32768;
        hipLaunchKernelGGL(gm_warp_error_kernel, dim3(nblk, nc, 1), dim3(256), 0, st, src, src_stride, w, h, t, models, n, c0, n, (const SvtHipGmJob*)nullptr,
                           (const int*)nullptr, d_lut, (unsigned long long*)d_err);
    }
    return (int)hipGetLastError();
}

extern "C" int svt_hip_launch_gm_frame_error(hipStream_t st, const uint8_t* src, int src_stride, int w, int h, const SvtHipGmRef* refs, int n_refs, const uint16_t* d_lut,
                                             int64_t* d_err) {
    if (n_refs <= 0) return 0;
    hipError_t e = hipMemsetAsync(d_err, 0, (size_t)n_refs * 8, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(gm_frame_error_kernel, dim3((h + 7) / 8, n_refs), dim3(256), 0, st, src, src_stride, w, h, ref_tab(refs, n_refs), d_lut,
                       (unsigned long long*)d_err);
    return (int)hipGetLastError();
}

namespace {
struct GmScratch { GmState* states; SvtHipGmModel* cands; long long* err; int* n_live; int* done; };
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
GmScratch carve(void* base, int njobs) {
    uint8_t* p = (uint8_t*)base;
    GmScratch s;
    s.states = (GmState*)p; p += up256(sizeof(GmState) * (size_t)njobs);
    s.cands = (SvtHipGmModel*)p; p += up256(sizeof(SvtHipGmModel) * (size_t)njobs * GM_NC);
    s.err = (long long*)p; p += up256(8 * (size_t)njobs * GM_NC);
    s.n_live = (int*)p; p += up256(4 * (size_t)njobs);
    s.done = (int*)p;
    return s;
}
}  // namespace

extern "C" size_t svt_hip_gm_refine_scratch_layout_bytes(int njobs) {
    if (njobs < 0) njobs = 0;
    return up256(sizeof(GmState) * (size_t)njobs) + up256(sizeof(SvtHipGmModel) * (size_t)njobs * GM_NC) + up256(8 * (size_t)njobs * GM_NC) + up256(4 * (size_t)njobs) + 256;
}

// rounds [first_round, first_round + n_rounds) of the walk: round 0 is the launch that starts every job
extern "C" int svt_hip_launch_gm_refine_rounds(hipStream_t st, const uint8_t* src, int src_stride, int w, int h, const SvtHipGmRef* refs, int n_refs, const SvtHipGmJob* jobs,
                                               int njobs, SvtHipGmResult* results, void* scratch, const uint16_t* d_lut, int start, int n_rounds) {
    const GmScratch s = carve(scratch, njobs);
    const GmRefTab t = ref_tab(refs, n_refs);
    const int nblk = ((w + 31) >> 5) * ((h + 31) >> 5);
    if (start) {
        hipError_t e = hipMemsetAsync(s.done, 0, 4, st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(gm_refine_step_kernel, dim3(njobs), dim3(64), 0, st, jobs, n_refs, s.states, s.cands, s.err, s.n_live, s.done, results, 1);
    }
    for (int r = 0; r < n_rounds; r++) {
        hipLaunchKernelGGL(gm_warp_error_kernel, dim3(nblk, GM_NC, njobs), dim3(256), 0, st, src, src_stride, w, h, t, (const SvtHipGmModel*)s.cands, GM_NC, 0, GM_NC, jobs,
                           (const int*)s.n_live, d_lut, (unsigned long long*)s.err);
        hipLaunchKernelGGL(gm_refine_step_kernel, dim3(njobs), dim3(64), 0, st, jobs, n_refs, s.states, s.cands, s.err, s.n_live, s.done, results, 0);
    }
    return (int)hipGetLastError();
}

extern "C" const int* svt_hip_gm_done_counter(void* scratch, int njobs) { return carve(scratch, njobs).done; }

SVT_HIP_TU_PROBE(gm)
