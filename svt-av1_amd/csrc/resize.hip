// resize.hip — super-resolution: the normative upscale and the general scaler; gfx950.
//
// Replaces svt_av1_upscale_normative_rows (Common/Codec/EbSuperRes.c:40-294: the frame upscale between CDEF and the restoration, and the restoration's
// stripe context rows) and av1_resize_plane / av1_highbd_resize_plane (Encoder/Codec/EbResize.c:186-765: the source and the references at the coded size).
// All integer and exact; docs/kernels/superres.md has the per-sample traffic and the two arguments the kernels rest on:
//   * the reference's tile-column loop samples position x0_qn + x * x_step_qn for the whole row, so no kernel takes tile information;
//   * clamping a source index to the row equals the reference's replicated border columns, and equals every "initial / middle / end / short" range of the
//     scaler's filters (those ranges only leave out the clamps that cannot bind), so each filter is written once, with both clamps.
// The filter tables (resize_filters.h) are codec constants; the stage lists and the scratch layout come from resize_plan.h (host).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "resize_plan.h"
#include "resize_filters.h"

namespace {

typedef short taps8 __attribute__((ext_vector_type(8)));   // the eight taps of a phase: one 16-byte read

__device__ __attribute__((aligned(16))) const int16_t k_filters[5][64][8] = {SVT_RESIZE_FILTER_NORMATIVE, SVT_RESIZE_FILTER_875, SVT_RESIZE_FILTER_750, SVT_RESIZE_FILTER_625, SVT_RESIZE_FILTER_500};

constexpr int UP_SEG = 1024;   // output samples of a row per workgroup of superres_upscale_kernel: 4 per thread

struct UpscalePlane { const void* src; void* dst; int src_stride, dst_stride, in_w, out_w, rows, x_step_qn, x0_qn; };
struct UpscaleArgs { UpscalePlane p[3]; };

// One output sample per thread and trip: workgroup (segment, row, plane).  The source samples the segment needs (at most UP_SEG + 8, the step never
// exceeds one sample) and the table go to LDS first; stores are one contiguous run of 256 samples per trip.  Two other shapes were measured and were no
// faster (docs/kernels/superres.md): a workgroup walking eight rows, and eight rows staged behind one barrier with a phase's taps read once for all.
template <typename PIX>
__global__ void __launch_bounds__(256)
superres_upscale_kernel(UpscaleArgs a, int maxv) {
    __shared__ int16_t s_f[64 * 8];
    __shared__ PIX s_src[UP_SEG + 16];
    const UpscalePlane& p = a.p[blockIdx.z];
    const int xs = blockIdx.x * UP_SEG, y = blockIdx.y;
    if (xs >= p.out_w || y >= p.rows) return;   // uniform: planes of one launch differ in size
    const int xe = min(xs + UP_SEG, p.out_w);
    const int first = ((p.x0_qn + xs * p.x_step_qn) >> 14) - 4;
    const int count = ((p.x0_qn + (xe - 1) * p.x_step_qn) >> 14) + 4 - first;
    const PIX* src = (const PIX*)p.src + (size_t)y * p.src_stride;
    for (int i = threadIdx.x; i < count; i += 256) s_src[i] = src[min(max(first + i, 0), p.in_w - 1)];
    for (int i = threadIdx.x; i < 64 * 8; i += 256) s_f[i] = (&k_filters[0][0][0])[i];
    __syncthreads();
    PIX* dst = (PIX*)p.dst + (size_t)y * p.dst_stride;
    for (int x = xs + threadIdx.x; x < xe; x += 256) {
        const int x_qn = p.x0_qn + x * p.x_step_qn;
        const PIX* s = s_src + ((x_qn >> 14) - 4 - first);
        const int16_t* f = s_f + ((x_qn & 0x3fff) >> 8) * 8;
        int sum = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) sum += (int)s[k] * f[k];
        dst[x] = (PIX)min(max((sum + 64) >> 7, 0), maxv);
    }
}

// ---- the scaler's three filters, each over a loader `ld(i)` of the current line; indices are clamped to the line
template <class LD> __device__ __forceinline__ int down2_symeven(LD ld, int len, int o) {
    constexpr int f[4] = SVT_RESIZE_DOWN2_SYMEVEN_HALF;
    const int i = 2 * o;
    int sum = 64;
#pragma unroll
    for (int j = 0; j < 4; j++) sum += (ld(max(i - j, 0)) + ld(min(i + 1 + j, len - 1))) * f[j];
    return sum >> 7;
}
template <class LD> __device__ __forceinline__ int down2_symodd(LD ld, int len, int o) {
    constexpr int f[4] = SVT_RESIZE_DOWN2_SYMODD_HALF;
    const int i = 2 * o;
    int sum = 64 + ld(i) * f[0];
#pragma unroll
    for (int j = 1; j < 4; j++) sum += (ld(max(i - j, 0)) + ld(min(i + j, len - 1))) * f[j];
    return sum >> 7;
}
template <class LD, class FT> __device__ __forceinline__ int interpolate(LD ld, FT taps, const SvtResizeStage& st, int o) {
    const int y = st.offset + 128 + o * st.delta, ip = y >> 14;
    const taps8 f = *(const taps8*)(taps + ((y >> 8) & 63) * 8);
    int sum = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) sum += f[k] * ld(min(max(ip - 3 + k, 0), st.in_len - 1));
    return (sum + 64) >> 7;
}
template <class LD, class FT> __device__ __forceinline__ int stage_sample(LD ld, FT taps, const SvtResizeStage& st, int o, int maxv) {
    const int v = st.kind == SVT_RS_DOWN2_EVEN ? down2_symeven(ld, st.in_len, o) : st.kind == SVT_RS_DOWN2_ODD ? down2_symodd(ld, st.in_len, o)
                : st.kind == SVT_RS_INTERP ? interpolate(ld, taps, st, o) : ld(o);
    return min(max(v, 0), maxv);
}

struct ResizePlane { const void* src; void* dst; void* t0; void* t1; int src_stride, dst_stride, t_stride, lines; SvtResizeAxis ax; };
struct ResizeArgs { ResizePlane p[3]; };

// The row pass: one workgroup per row and plane.  The row goes to LDS once; the halvings ping-pong between two LDS lines (in_w and ceil(in_w / 2) samples,
// kept as 16-bit values) and the last stage writes the destination row.  Dynamic LDS: the interpolation table, then the two lines.
template <typename PIX>
__global__ void __launch_bounds__(256)
resize_rows_kernel(ResizeArgs a, int maxv) {
    extern __shared__ uint16_t s_mem[];
    const ResizePlane& p = a.p[blockIdx.y];
    const int y = blockIdx.x;
    if (y >= p.lines) return;
    const SvtResizeAxis& ax = p.ax;
    const PIX* src = (const PIX*)p.src + (size_t)y * p.src_stride;
    PIX* dst = (PIX*)p.dst + (size_t)y * p.dst_stride;
    const int in_len = ax.s[0].in_len;
    if (ax.s[0].kind == SVT_RS_COPY) {
        for (int i = threadIdx.x; i < in_len; i += 256) dst[i] = src[i];
        return;
    }
    int16_t* s_f = (int16_t*)s_mem;
    uint16_t* const line0 = s_mem + 512;
    uint16_t* const line1 = line0 + in_len;
    for (int i = threadIdx.x; i < in_len; i += 256) line0[i] = src[i];
    const SvtResizeStage& last = ax.s[ax.n - 1];
    if (last.kind == SVT_RS_INTERP)
        for (int i = threadIdx.x; i < 512; i += 256) s_f[i] = (&k_filters[last.filter][0][0])[i];
    __syncthreads();
    for (int s = 0; s < ax.n; s++) {
        const SvtResizeStage& st = ax.s[s];
        const uint16_t* in = (s & 1) ? line1 : line0;
        const auto ld = [in](int i) { return (int)in[i]; };
        if (s == ax.n - 1) {
            for (int o = threadIdx.x; o < st.out_len; o += 256) dst[o] = (PIX)stage_sample(ld, s_f, st, o, maxv);
        } else {
            uint16_t* out = (s & 1) ? line0 : line1;
            for (int o = threadIdx.x; o < st.out_len; o += 256) out[o] = (uint16_t)stage_sample(ld, s_f, st, o, maxv);
            __syncthreads();
        }
    }
}

// One stage of the column pass: threads along x, one output row per workgroup row, so the stage, the output index, the filter phase and the eight source
// rows are uniform over the workgroup (scalar) and every load and store is a contiguous run.  A plane whose list is shorter than `s` stages sits the launch out.
template <typename PIX>
__global__ void __launch_bounds__(256)
resize_cols_kernel(ResizeArgs a, int s, int maxv) {
    const ResizePlane& p = a.p[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y;
    if (s >= p.ax.n) return;
    const SvtResizeStage& st = p.ax.s[s];
    if (o >= st.out_len || x >= p.lines) return;
    const PIX* in = s == 0 ? (const PIX*)p.src : (const PIX*)((s - 1) & 1 ? p.t1 : p.t0);
    const int in_stride = s == 0 ? p.src_stride : p.t_stride;
    const bool is_last = s == p.ax.n - 1;
    PIX* out = is_last ? (PIX*)p.dst : (PIX*)(s & 1 ? p.t1 : p.t0);
    const int out_stride = is_last ? p.dst_stride : p.t_stride;
    const auto ld = [in, in_stride, x](int i) { return (int)in[(size_t)i * in_stride + x]; };
    out[(size_t)o * out_stride + x] = (PIX)stage_sample(ld, &k_filters[st.filter][0][0], st, o, maxv);
}

}  // namespace

extern "C" int svt_hip_launch_superres_upscale(hipStream_t st, int pix_bytes, int bd, const SvtHipUpscalePlane* planes, int n) {
    UpscaleArgs a = {};
    int max_w = 0, max_rows = 0;
    for (int i = 0; i < n; i++) {
        const SvtHipUpscalePlane& q = planes[i];
        const int32_t step = svt_superres_step_qn(q.in_w, q.out_w);
        a.p[i] = UpscalePlane{q.d_src, q.d_dst, q.src_stride, q.dst_stride, q.in_w, q.out_w, q.rows, step, svt_superres_x0_qn(q.in_w, q.out_w, step)};
        max_w = q.out_w > max_w ? q.out_w : max_w;
        max_rows = q.rows > max_rows ? q.rows : max_rows;
    }
    const dim3 grid((max_w + UP_SEG - 1) / UP_SEG, max_rows, n);
    svt_for_pix(pix_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL(superres_upscale_kernel<PIX>, grid, dim3(256), 0, st, a, (1 << bd) - 1);
    });
    return (int)hipGetLastError();
}

extern "C" size_t svt_hip_resize_scratch_layout_bytes(int pix_bytes, const SvtHipResizePlane* planes, int n) {
    size_t off = 0;
    for (int i = 0; i < n; i++) off = svt_resize_scratch_layout(pix_bytes, planes[i], off).end;
    return off;
}

extern "C" int svt_hip_launch_resize_planes(hipStream_t st, int pix_bytes, int bd, const SvtHipResizePlane* planes, int n, void* scratch) {
    ResizeArgs rows = {}, cols = {};
    int row_planes = 0, max_lines = 0, max_in_w = 0, col_stages = 0, max_out_h = 0, max_cols = 0;
    bool halves = false;
    size_t off = 0;
    for (int i = 0; i < n; i++) {
        const SvtHipResizePlane& q = planes[i];
        const SvtResizeScratch l = svt_resize_scratch_layout(pix_bytes, q, off);
        off = l.end;
        char* const x = (char*)scratch;
        const bool do_cols = q.in_h != q.out_h, do_rows = q.in_w != q.out_w || !do_cols;   // equal sizes: the row pass copies
        const void* mid = q.d_src;
        int mid_stride = q.src_stride;
        if (do_rows) {
            ResizePlane& r = rows.p[row_planes++];
            r = ResizePlane{q.d_src, do_cols ? (void*)(x + l.inter) : q.d_dst, nullptr, nullptr, q.src_stride, do_cols ? q.out_w : q.dst_stride, 0, q.in_h,
                            svt_resize_axis_plan(q.in_w, q.out_w)};
            mid = r.dst, mid_stride = r.dst_stride;
            max_lines = q.in_h > max_lines ? q.in_h : max_lines;
            if (r.ax.s[0].kind != SVT_RS_COPY) max_in_w = q.in_w > max_in_w ? q.in_w : max_in_w;
            halves |= r.ax.n > 1;
        }
        // a plane that keeps its height leaves an empty list: it sits the column launches out
        ResizePlane& c = cols.p[i];
        c = ResizePlane{mid, q.d_dst, x + l.t0, x + l.t1, mid_stride, q.dst_stride, q.out_w, q.out_w, do_cols ? svt_resize_axis_plan(q.in_h, q.out_h) : SvtResizeAxis{}};
        if (do_cols) {
            col_stages = c.ax.n > col_stages ? c.ax.n : col_stages;
            max_out_h = (q.in_h + 1) / 2 > max_out_h ? (q.in_h + 1) / 2 : max_out_h;
            max_out_h = q.out_h > max_out_h ? q.out_h : max_out_h;
            max_cols = q.out_w > max_cols ? q.out_w : max_cols;
        }
    }
    const int maxv = (1 << bd) - 1;
    svt_for_pix(pix_bytes, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        if (row_planes) {
            const size_t lds = max_in_w ? 2 * (size_t)(512 + max_in_w + (halves ? (max_in_w + 1) / 2 : 0)) : 0;
            hipLaunchKernelGGL(resize_rows_kernel<PIX>, dim3(max_lines, row_planes), dim3(256), lds, st, rows, maxv);
        }
        for (int s = 0; s < col_stages; s++)
            hipLaunchKernelGGL(resize_cols_kernel<PIX>, dim3((max_cols + 255) / 256, max_out_h, n), dim3(256), 0, st, cols, s, maxv);
    });
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(resize)
