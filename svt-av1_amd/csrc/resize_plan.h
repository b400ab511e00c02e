// resize_plan.h — the host arithmetic of the scaler (csrc/resize.hip): super-resolution sizes and sampling positions, the stage list of one axis of
// av1_resize_plane and the layout of the caller's scratch.  Plain C++17, nothing from HIP: the C-ABI layer answers svt_hip_superres_* and
// svt_hip_resize_scratch_bytes from it without touching the runtime, and the launcher of resize.hip walks the same lists.
// Reference: Common/Codec/EbSuperRes.c:22-51, Encoder/Codec/EbResize.c:186-205, :311-325, :327-335, :407-440.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/svt_hip.h"

enum { SVT_RS_MAX_DIM = 16384 };
enum { SVT_RS_COPY = 0, SVT_RS_DOWN2_EVEN = 1, SVT_RS_DOWN2_ODD = 2, SVT_RS_INTERP = 3 };
enum { SVT_RS_MAX_STAGES = 16 };   // 16384 -> 1 is 14 halvings; an interpolation can only follow fewer

// calculate_scaled_size_helper: dim * 8 / denom rounded, never below min(16, dim)
inline int svt_superres_scaled_dim(int dim, int denom) {
    if (denom == 8) return dim;
    const int min_dim = dim < 16 ? dim : 16;
    const int d = (uint16_t)((dim * 8 + denom / 2) / denom);
    return d > min_dim ? d : min_dim;
}
// av1_get_upscale_convolve_step, get_upscale_convolve_x0 (positions in 1/16384 sample)
inline int32_t svt_superres_step_qn(int in_w, int out_w) { return ((in_w << 14) + out_w / 2) / out_w; }
inline int32_t svt_superres_x0_qn(int in_w, int out_w, int32_t step) {
    const int err = out_w * step - (in_w << 14);
    const int32_t x0 = (-((out_w - in_w) << 13) + out_w / 2) / out_w + 128 - err / 2;
    return (int32_t)((uint32_t)x0 & 0x3fff);
}

// One stage of resize_multistep: out_len samples from in_len.  INTERP: filter = the table (0 normative, 1 .. 4 = the 0.875 / 0.75 / 0.625 / 0.5 bands),
// output o samples position offset + 128 + o * delta (1/16384 sample).
struct SvtResizeStage { int kind, in_len, out_len, filter, delta, offset; };
struct SvtResizeAxis { int n; SvtResizeStage s[SVT_RS_MAX_STAGES]; };

inline int svt_resize_choose_filter(int in_len, int out_len) {
    const int o16 = out_len * 16;
    return o16 >= in_len * 16 ? 0 : o16 >= in_len * 13 ? 1 : o16 >= in_len * 11 ? 2 : o16 >= in_len * 9 ? 3 : 4;
}
inline int svt_resize_down2_steps(int in_len, int out_len) {
    int steps = 0, proj;
    while ((proj = (in_len + 1) >> 1) >= out_len) {
        ++steps;
        in_len = proj;
        if (in_len == 1) break;
    }
    return steps;
}
inline SvtResizeAxis svt_resize_axis_plan(int in_len, int out_len) {
    SvtResizeAxis a = {};
    if (in_len == out_len) {
        a.s[a.n++] = SvtResizeStage{SVT_RS_COPY, in_len, out_len, 0, 0, 0};
        return a;
    }
    int len = in_len;
    for (int steps = svt_resize_down2_steps(in_len, out_len); steps > 0; steps--) {
        a.s[a.n++] = SvtResizeStage{(len & 1) ? SVT_RS_DOWN2_ODD : SVT_RS_DOWN2_EVEN, len, (len + 1) >> 1, 0, 0, 0};
        len = (len + 1) >> 1;
    }
    if (len != out_len) {
        const int32_t delta = (int32_t)((((uint32_t)len << 14) + out_len / 2) / out_len);
        const int32_t offset = len > out_len ? (((int32_t)(len - out_len) << 13) + out_len / 2) / out_len : -((((int32_t)(out_len - len) << 13) + out_len / 2) / out_len);
        a.s[a.n++] = SvtResizeStage{SVT_RS_INTERP, len, out_len, svt_resize_choose_filter(len, out_len), delta, offset};
    }
    return a;
}

inline bool svt_resize_plane_ok(const SvtHipResizePlane& p) {
    return p.d_src && p.d_dst && p.d_src != p.d_dst && p.in_w >= 1 && p.in_w <= SVT_RS_MAX_DIM && p.in_h >= 1 && p.in_h <= SVT_RS_MAX_DIM && p.out_w >= 1 &&
           p.out_w <= SVT_RS_MAX_DIM && p.out_h >= 1 && p.out_h <= SVT_RS_MAX_DIM && p.src_stride >= p.in_w && p.dst_stride >= p.out_w;
}
inline bool svt_upscale_plane_ok(const SvtHipUpscalePlane& p) {
    return p.d_src && p.d_dst && p.d_src != p.d_dst && p.in_w >= 1 && p.out_w >= p.in_w && p.out_w <= SVT_RS_MAX_DIM && p.rows >= 1 && p.rows <= SVT_RS_MAX_DIM &&
           p.src_stride >= p.in_w && p.dst_stride >= p.out_w;
}

// The caller's scratch, per plane and in this order, each part rounded up to 256 bytes: the row pass's result (out_w x in_h; only when both axes change),
// then the column pass's two temporaries (out_w x ceil(in_h / 2) and out_w x ceil(in_h / 4); one per stage of the column's list that is not its last).
struct SvtResizeScratch { size_t inter, t0, t1, end; };
inline SvtResizeScratch svt_resize_scratch_layout(int pix_bytes, const SvtHipResizePlane& p, size_t base) {
    const auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    SvtResizeScratch l = {base, base, base, base};
    if (p.in_h == p.out_h) return l;
    size_t off = base;
    if (p.in_w != p.out_w) off += up((size_t)p.out_w * p.in_h * pix_bytes);
    l.t0 = off;
    const int stages = svt_resize_axis_plan(p.in_h, p.out_h).n;
    if (stages >= 2) off += up((size_t)p.out_w * ((p.in_h + 1) >> 1) * pix_bytes);
    l.t1 = off;
    if (stages >= 3) off += up((size_t)p.out_w * ((p.in_h + 3) >> 2) * pix_bytes);
    l.end = off;
    return l;
}
