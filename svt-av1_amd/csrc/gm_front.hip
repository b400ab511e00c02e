// gm_front.hip — the front half of global motion on the device: FAST-9 corners with non-maximum suppression, the 13x13 normalised cross-correlation and the
// correspondence search with its two refinement passes; gfx950, 8-bit luma.  docs/kernels/gm.md.
//
// Replaces (file:line in the reference's tree): Source/Lib/Encoder/Codec/corner_detect.c:19-32 svt_av1_fast_corner_detect with third_party/fastfeat/fast.c:6-21
// svt_aom_fast9_detect_nonmax, fast_9.c:8-2937 aom_fast9_corner_score, :2961-2973 svt_aom_fast9_score, :2976-5914 svt_aom_fast9_detect and nonmax.c:8-119
// svt_aom_nonmax_suppression; Source/Lib/Encoder/Codec/corner_match.c:24-37 compute_variance, :43-64 svt_av1_compute_cross_correlation_c, :66-76 the two
// eligibility tests, :78-149 improve_correspondence, :151-212 svt_av1_determine_correspondence.
//
// Corners, four launches over every plane of a call: gm_fast_score_kernel writes a u8 score plane (0 = no corner, else the reference's bisected score 18..254);
// gm_nms_count_kernel counts the corners each row keeps; gm_row_scan_kernel turns the counts into row offsets and the plane's totals; gm_nms_emit_kernel writes
// the kept corners at offset + rank-in-row.  A position is a function of the picture alone: no atomic decides an order.
// Correspondences, two launches: gm_match_kernel, one workgroup per source corner (candidate gather, argmax, acceptance, both refinement passes), leaves its pair
// or a "none" mark at slot i of the output; gm_corr_compact_kernel closes the gaps in place, in i order.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "svt_hip_internal.h"

namespace {

constexpr int FAST_BARRIER = 18;
constexpr int MATCH_SZ = 13, MATCH_SZ_BY2 = 6, MATCH_SZ_SQ = 169;
constexpr int SEARCH_SZ = 9, SEARCH_SZ_BY2 = 4;
constexpr int MAXP = SVT_HIP_GM_MAX_CORNERS;
constexpr int MAX_PLANES = 1 + SVT_HIP_GM_MAX_REFS;

// planes of one corner call; score / rows: byte offsets into the scratch (svt_hip_gm_corners_scratch_layout)
struct GmPlaneTab {
    SvtHipGmRef p[MAX_PLANES];
    unsigned long long score[MAX_PLANES], rows[MAX_PLANES];
};
struct GmRefTab8 { SvtHipGmRef r[SVT_HIP_GM_MAX_REFS]; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// ---------------------------------------------------------------------------------------------------------------- FAST-9 score
// The ring in make_offsets' order (fast_9.c:2939-2957): dx, dy of pixel[0..15]
__device__ const int8_t kRing[16][2] = {{0, 3}, {1, 3}, {2, 2}, {3, 1}, {3, 0}, {3, -1}, {2, -2}, {1, -3}, {0, -3}, {-1, -3}, {-2, -2}, {-3, -1}, {-3, 0}, {-3, 1}, {-2, 2}, {-1, 3}};

constexpr int TW = 32, TH = 8, TP = TW + 6 + 2;   // tile of one workgroup; LDS row pitch in bytes

// The score the reference's bisection ends on (bmin = 18, bmax = 255, corner(b) is monotone in b and false at 255): the largest b at which 9 contiguous ring
// pixels are all > p + b or all < p - b, i.e. max(B, D) - 1 with B = max over the 16 arcs of min(ring - p), D the same of p - ring; a corner iff that is >= 18.
__global__ void __launch_bounds__(256) gm_fast_score_kernel(GmPlaneTab tab, uint8_t* __restrict__ scratch) {
    __shared__ uint8_t tile[(TH + 6) * TP];
    const SvtHipGmRef pl = tab.p[blockIdx.z];
    const int w = pl.width, h = pl.height;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    if (x0 >= w || y0 >= h) return;   // uniform: the grid is sized for the largest plane of the call
    const int tid = threadIdx.x;
    for (int i = tid; i < (TH + 6) * (TW + 6); i += 256) {
        const int ty = i / (TW + 6), tx = i % (TW + 6);
        const int gx = x0 - 3 + tx, gy = y0 - 3 + ty;
        tile[ty * TP + tx] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? pl.d_plane[(size_t)gy * pl.stride + gx] : 0;
    }
    __syncthreads();
    const int lx = tid % TW, ly = tid / TW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) return;
    int score = 0;
    if (x >= 3 && x < w - 3 && y >= 3 && y < h - 3) {
        const int p = tile[(ly + 3) * TP + lx + 3];
        int d[16];
#pragma unroll
        for (int k = 0; k < 16; k++) d[k] = (int)tile[(ly + 3 + kRing[k][1]) * TP + lx + 3 + kRing[k][0]] - p;
        // min and max over the 9 pixels of the arc that starts at k: 2, 4, 8, then the ninth
        int lo[16], hi[16], t[16];
#pragma unroll
        for (int k = 0; k < 16; k++) { lo[k] = min(d[k], d[(k + 1) & 15]); hi[k] = max(d[k], d[(k + 1) & 15]); }
#pragma unroll
        for (int k = 0; k < 16; k++) t[k] = min(lo[k], lo[(k + 2) & 15]);
#pragma unroll
        for (int k = 0; k < 16; k++) lo[k] = min(t[k], t[(k + 4) & 15]);
#pragma unroll
        for (int k = 0; k < 16; k++) t[k] = max(hi[k], hi[(k + 2) & 15]);
#pragma unroll
        for (int k = 0; k < 16; k++) hi[k] = max(t[k], t[(k + 4) & 15]);
        int B = -256, D = -256;
#pragma unroll
        for (int k = 0; k < 16; k++) { B = max(B, min(lo[k], d[(k + 8) & 15])); D = max(D, -max(hi[k], d[(k + 8) & 15])); }
        const int s = max(B, D) - 1;   // <= 254
        if (s >= FAST_BARRIER) score = s;
    }
    (scratch + tab.score[blockIdx.z])[(size_t)y * w + x] = (uint8_t)score;
}

// ---------------------------------------------------------------------------------------------- non-maximum suppression, ordered
// nonmax.c keeps a corner unless one of its 8 neighbours is a corner whose score is >= its own.  With 0 for "no corner": kept iff every neighbour's score is
// below its own.  Scores are 0 outside 3 <= x < w - 3, 3 <= y < h - 3, so a kept corner's neighbours are all inside the plane.
__device__ __forceinline__ bool nms_keep(const uint8_t* __restrict__ sc, int w, int h, int x, int y) {
    if (x < 3 || x >= w - 3 || y < 3 || y >= h - 3) return false;
    const uint8_t* c = sc + (size_t)y * w + x;
    const int s = c[0];
    if (!s) return false;
    const int m = max(max(max((int)c[-w - 1], (int)c[-w]), max((int)c[-w + 1], (int)c[-1])), max(max((int)c[1], (int)c[w - 1]), max((int)c[w], (int)c[w + 1])));
    return m < s;
}

// one wave per row: blockIdx.x = 4 rows, blockIdx.y = the plane
__global__ void __launch_bounds__(256) gm_nms_count_kernel(GmPlaneTab tab, uint8_t* __restrict__ scratch) {
    const SvtHipGmRef pl = tab.p[blockIdx.y];
    const int w = pl.width, h = pl.height;
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y >= h) return;
    const uint8_t* sc = scratch + tab.score[blockIdx.y];
    int n = 0;
    if (y >= 3 && y < h - 3)
        for (int xb = 0; xb < w; xb += 64) n += __popcll(__ballot(nms_keep(sc, w, h, xb + lane, y)));
    if (lane == 0) ((int*)(scratch + tab.rows[blockIdx.y]))[y] = n;
}

// exclusive scan of a plane's row counts, in place; one workgroup per plane; h <= 16384 = 256 threads x 64 rows
__global__ void __launch_bounds__(256) gm_row_scan_kernel(GmPlaneTab tab, uint8_t* __restrict__ scratch, int max_points, int* __restrict__ counts, int* __restrict__ kept) {
    __shared__ int part[256];
    const int h = tab.p[blockIdx.x].height, tid = threadIdx.x;
    int* rows = (int*)(scratch + tab.rows[blockIdx.x]);
    const int per = (h + 255) / 256, r0 = min(h, tid * per), r1 = min(h, r0 + per);
    int s = 0;
    for (int r = r0; r < r1; r++) s += rows[r];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {   // inclusive scan of the 256 partial sums
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - s;
    for (int r = r0; r < r1; r++) { const int c = rows[r]; rows[r] = run; run += c; }
    if (tid == 255) {
        counts[blockIdx.x] = min(part[255], max_points);
        if (kept) kept[blockIdx.x] = part[255];
    }
}

// svt_av1_fast_corner_detect copies the first max_points of the raster-ordered list
__global__ void __launch_bounds__(256) gm_nms_emit_kernel(GmPlaneTab tab, const uint8_t* __restrict__ scratch, int max_points, int* __restrict__ points) {
    const SvtHipGmRef pl = tab.p[blockIdx.y];
    const int w = pl.width, h = pl.height;
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y < 3 || y >= h - 3) return;
    const uint8_t* sc = scratch + tab.score[blockIdx.y];
    int base = ((const int*)(scratch + tab.rows[blockIdx.y]))[y];
    int* out = points + (size_t)blockIdx.y * max_points * 2;
    for (int xb = 0; xb < w && base < max_points; xb += 64) {
        const bool k = nms_keep(sc, w, h, xb + lane, y);
        const unsigned long long b = __ballot(k);
        const int pos = base + __popcll(b & ((1ull << lane) - 1));
        if (k && pos < max_points) { out[2 * pos] = xb + lane; out[2 * pos + 1] = y; }
        base += __popcll(b);
    }
}

// -------------------------------------------------------------------------------------------------------------- cross-correlation
__device__ __forceinline__ bool eligible_point(int x, int y, int w, int h) {   // is_eligible_point without the overflow of x + 6: w, h >= 8
    return x >= MATCH_SZ_BY2 && y >= MATCH_SZ_BY2 && x < w - MATCH_SZ_BY2 && y < h - MATCH_SZ_BY2;
}
__device__ __forceinline__ bool eligible_distance(int x1, int y1, int x2, int y2, int thresh_sqr) {   // both points are inside a plane of <= 16384: no overflow
    const int dx = x1 - x2, dy = y1 - y2;
    return dx * dx + dy * dy <= thresh_sqr;
}

// svt_av1_compute_cross_correlation_c with patch 1 given as its 169 samples and their sum: cov / sqrt(var2) in IEEE double (0 / 0 = NaN for a flat patch 2).
// Every sum is the reference's int: 169 * 169 * 255^2 < 2^31.
template <class P1>
__device__ __forceinline__ double ncc_patch(P1 p1, int sum1, const uint8_t* __restrict__ im2, int stride2, int x2, int y2) {
    int sum2 = 0, sumsq2 = 0, cross = 0;
    const uint8_t* q = im2 + (ptrdiff_t)(y2 - MATCH_SZ_BY2) * stride2 + (x2 - MATCH_SZ_BY2);
    for (int i = 0; i < MATCH_SZ; i++, q += stride2) {
#pragma unroll
        for (int j = 0; j < MATCH_SZ; j++) {
            const int v2 = q[j], v1 = p1(i * MATCH_SZ + j);
            sum2 += v2; sumsq2 += v2 * v2; cross += v1 * v2;
        }
    }
    const int var2 = sumsq2 * MATCH_SZ_SQ - sum2 * sum2;
    const int cov = cross * MATCH_SZ_SQ - sum1 * sum2;
    return (double)cov / sqrt((double)var2);
}

// one lane per pair; a pair whose windows do not lie inside w x h is not read: 0.0
__global__ void __launch_bounds__(256) gm_cross_correlation_kernel(const uint8_t* __restrict__ im1, int stride1, const uint8_t* __restrict__ im2, int stride2, int w, int h,
                                                                   const int* __restrict__ pairs, int n, double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x1 = pairs[4 * (size_t)i], y1 = pairs[4 * (size_t)i + 1], x2 = pairs[4 * (size_t)i + 2], y2 = pairs[4 * (size_t)i + 3];
    double r = 0.0;
    if (eligible_point(x1, y1, w, h) && eligible_point(x2, y2, w, h)) {
        const uint8_t* a = im1 + (ptrdiff_t)(y1 - MATCH_SZ_BY2) * stride1 + (x1 - MATCH_SZ_BY2);
        int sum1 = 0;
        for (int k = 0; k < MATCH_SZ_SQ; k++) sum1 += a[(k / MATCH_SZ) * stride1 + k % MATCH_SZ];
        r = ncc_patch([&](int k) { return (int)a[(k / MATCH_SZ) * stride1 + k % MATCH_SZ]; }, sum1, im2, stride2, x2, y2);
    }
    out[i] = r;
}

// ----------------------------------------------------------------------------------------------------------------- correspondences
// The reference's argmax: strict > from 0.0 in index order, so the first (lowest-index) maximum wins, and a NaN, which compares false, never does.
struct Best { double v; int k; };
__device__ __forceinline__ void best_take(Best& a, double v, int k) {
    if (v > a.v || (v == a.v && k < a.k)) { a.v = v; a.k = k; }
}
// over the workgroup; every thread gets the result.  Lanes without a candidate carry {0.0, INT_MAX}: nothing but a value > 0.0 displaces the initial 0.0.
__device__ __forceinline__ Best best_reduce(Best b, Best* red) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double v = __shfl_xor(b.v, o, 64);
        const int k = __shfl_xor(b.k, o, 64);
        best_take(b, v, k);
    }
    __syncthreads();   // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
    __syncthreads();
    Best r = red[0];
#pragma unroll
    for (int i = 1; i < 4; i++) best_take(r, red[i].v, red[i].k);
    return r;
}

__device__ __forceinline__ void stage_patch(uint8_t* dst, int* sums, const uint8_t* __restrict__ im, int stride, int x, int y) {
    // 169 samples of the window centred at (x, y) into LDS, their sum and sum of squares into sums[0..1] (zeroed by the caller before a barrier)
    const int tid = threadIdx.x;
    int s = 0, q = 0;
    if (tid < MATCH_SZ_SQ) {
        const int v = im[(ptrdiff_t)(y - MATCH_SZ_BY2 + tid / MATCH_SZ) * stride + (x - MATCH_SZ_BY2 + tid % MATCH_SZ)];
        dst[tid] = (uint8_t)v; s = v; q = v * v;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) { s += __shfl_down(s, o, 64); q += __shfl_down(q, o, 64); }
    if ((tid & 63) == 0 && tid < 192) { atomicAdd(&sums[0], s); atomicAdd(&sums[1], q); }   // integer adds: exact in any order
}

// One workgroup per (source corner i, reference r).  Slot i of corr[r] receives {x, y, rx, ry} after both refinement passes, or x = -1 when corner i gives no
// correspondence (an accepted x is >= 6).  Counts and coordinates come from device memory: a count is clamped to [0, max_points], and a coordinate is used as
// an address only after eligible_point has passed it.
__global__ void __launch_bounds__(256) gm_match_kernel(const uint8_t* __restrict__ src, int src_stride, int w, int h, const int* __restrict__ src_points,
                                                       const int* __restrict__ src_count, GmRefTab8 refs, const int* __restrict__ ref_points,
                                                       const int* __restrict__ ref_counts, int max_points, int* __restrict__ corr) {
    __shared__ uint8_t tmpl[176];
    __shared__ uint16_t cand[MAXP];
    __shared__ int wcnt[2][4];
    __shared__ int sums[2];
    __shared__ Best red[4];
    const int i = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (i >= clampi(src_count[0], 0, max_points)) return;
    int* out = corr + ((size_t)r * max_points + i) * 4;
    const int x = src_points[2 * i], y = src_points[2 * i + 1];
    if (!eligible_point(x, y, w, h)) {   // uniform
        if (tid == 0) out[0] = -1;
        return;
    }
    const uint8_t* __restrict__ ref = refs.r[r].d_plane;
    const int ref_stride = refs.r[r].stride;
    const int* __restrict__ rp = ref_points + (size_t)r * max_points * 2;
    const int n_ref = clampi(ref_counts[r], 0, max_points);
    const int thresh = max(w, h) >> 4, thresh_sqr = thresh * thresh;

    if (tid < 2) sums[tid] = 0;
    __syncthreads();
    stage_patch(tmpl, sums, src, src_stride, x, y);
    // the eligible reference corners within the distance, compacted in j order
    int n_cand = 0;
    for (int j0 = 0, it = 0; j0 < n_ref; j0 += 256, it++) {
        const int j = j0 + tid;
        bool ok = false;
        if (j < n_ref) {
            const int cx = rp[2 * j], cy = rp[2 * j + 1];
            ok = eligible_point(cx, cy, w, h) && eligible_distance(x, y, cx, cy, thresh_sqr);
        }
        const unsigned long long b = __ballot(ok);
        if (lane == 0) wcnt[it & 1][wave] = __popcll(b);
        __syncthreads();   // also orders tmpl / sums on the first pass
        int pos = n_cand + __popcll(b & ((1ull << lane) - 1));
        for (int k = 0; k < 4; k++) { const int c = wcnt[it & 1][k]; if (k < wave) pos += c; n_cand += c; }
        if (ok) cand[pos] = (uint16_t)j;
    }
    __syncthreads();
    const int sum1 = sums[0], var1 = sums[1] * MATCH_SZ_SQ - sums[0] * sums[0];

    Best b = {0.0, INT_MAX};
    for (int k = tid; k < n_cand; k += 256) {
        const int j = cand[k];
        best_take(b, ncc_patch([&](int t) { return (int)tmpl[t]; }, sum1, ref, ref_stride, rp[2 * j], rp[2 * j + 1]), j);
    }
    b = best_reduce(b, red);
    if (!(b.v > 0.75 * sqrt((double)var1))) {   // THRESHOLD_NCC * sqrt(template_norm); with no candidate 0.0 > x is false for every x >= 0
        if (tid == 0) out[0] = -1;
        return;
    }
    int rx = rp[2 * b.k], ry = rp[2 * b.k + 1];

    // improve_correspondence, first pass: the reference point moves over +-4, raster order, the source patch is the template
    {
        Best m = {0.0, INT_MAX};
        if (tid < SEARCH_SZ * SEARCH_SZ) {
            const int cx = rx + tid % SEARCH_SZ - SEARCH_SZ_BY2, cy = ry + tid / SEARCH_SZ - SEARCH_SZ_BY2;
            if (eligible_point(cx, cy, w, h) && eligible_distance(x, y, cx, cy, thresh_sqr))
                best_take(m, ncc_patch([&](int t) { return (int)tmpl[t]; }, sum1, ref, ref_stride, cx, cy), tid);
        }
        m = best_reduce(m, red);
        if (m.v > 0.0) { rx += m.k % SEARCH_SZ - SEARCH_SZ_BY2; ry += m.k / SEARCH_SZ - SEARCH_SZ_BY2; }
    }
    // second pass: the source point moves, the patch at the updated reference point is the template (the variance is always the moving side's)
    int sx = x, sy = y;
    {
        if (tid < 2) sums[tid] = 0;
        __syncthreads();   // every thread has left the first pass's reads of tmpl (best_reduce ends behind a barrier)
        stage_patch(tmpl, sums, ref, ref_stride, rx, ry);
        __syncthreads();
        const int rsum = sums[0];
        Best m = {0.0, INT_MAX};
        if (tid < SEARCH_SZ * SEARCH_SZ) {
            const int cx = x + tid % SEARCH_SZ - SEARCH_SZ_BY2, cy = y + tid / SEARCH_SZ - SEARCH_SZ_BY2;
            if (eligible_point(cx, cy, w, h) && eligible_distance(cx, cy, rx, ry, thresh_sqr))
                best_take(m, ncc_patch([&](int t) { return (int)tmpl[t]; }, rsum, src, src_stride, cx, cy), tid);
        }
        m = best_reduce(m, red);
        if (m.v > 0.0) { sx += m.k % SEARCH_SZ - SEARCH_SZ_BY2; sy += m.k / SEARCH_SZ - SEARCH_SZ_BY2; }
    }
    if (tid == 0) { out[0] = sx; out[1] = sy; out[2] = rx; out[3] = ry; }
}

// closes the gaps of corr[r][0 .. count) in place, in i order; one workgroup per reference.  A pair moves to a slot at or below its own, and a chunk is written
// only after all of it has been read.
__global__ void __launch_bounds__(256) gm_corr_compact_kernel(const int* __restrict__ src_count, int max_points, int* corr, int* __restrict__ ncorr) {
    __shared__ int wcnt[2][4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = clampi(src_count[0], 0, max_points);
    int* c = corr + (size_t)r * max_points * 4;
    int total = 0;
    for (int i0 = 0, it = 0; i0 < n; i0 += 256, it++) {
        const int i = i0 + tid;
        int v[4] = {-1, 0, 0, 0};
        if (i < n)
            for (int k = 0; k < 4; k++) v[k] = c[4 * i + k];
        const bool ok = v[0] >= 0;
        const unsigned long long b = __ballot(ok);
        if (lane == 0) wcnt[it & 1][wave] = __popcll(b);
        __syncthreads();
        int pos = total + __popcll(b & ((1ull << lane) - 1));
        for (int k = 0; k < 4; k++) { const int cc = wcnt[it & 1][k]; if (k < wave) pos += cc; total += cc; }
        if (ok)
            for (int k = 0; k < 4; k++) c[4 * pos + k] = v[k];
    }
    if (tid == 0) ncorr[r] = total;
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

GmPlaneTab plane_tab(const SvtHipGmRef* planes, int n) {
    GmPlaneTab t = {};
    size_t off = 0;
    for (int i = 0; i < n && i < MAX_PLANES; i++) {
        t.p[i] = planes[i];
        t.score[i] = off; off += up256((size_t)planes[i].width * planes[i].height);
        t.rows[i] = off; off += up256(4 * (size_t)planes[i].height);
    }
    return t;
}

}  // namespace

extern "C" size_t svt_hip_gm_corners_scratch_layout_bytes(const SvtHipGmRef* planes, int n_planes) {
    size_t total = 0;
    for (int i = 0; i < n_planes; i++) total += up256((size_t)planes[i].width * planes[i].height) + up256(4 * (size_t)planes[i].height);
    return total;
}

extern "C" int svt_hip_launch_gm_corners(hipStream_t st, const SvtHipGmRef* planes, int n_planes, int max_points, int* points, int* counts, int* kept, void* scratch) {
    const GmPlaneTab t = plane_tab(planes, n_planes);
    int mw = 0, mh = 0;
    for (int i = 0; i < n_planes; i++) { mw = planes[i].width > mw ? planes[i].width : mw; mh = planes[i].height > mh ? planes[i].height : mh; }
    hipLaunchKernelGGL(gm_fast_score_kernel, dim3((mw + TW - 1) / TW, (mh + TH - 1) / TH, n_planes), dim3(256), 0, st, t, (uint8_t*)scratch);
    hipLaunchKernelGGL(gm_nms_count_kernel, dim3((mh + 3) / 4, n_planes), dim3(256), 0, st, t, (uint8_t*)scratch);
    hipLaunchKernelGGL(gm_row_scan_kernel, dim3(n_planes), dim3(256), 0, st, t, (uint8_t*)scratch, max_points, counts, kept);
    hipLaunchKernelGGL(gm_nms_emit_kernel, dim3((mh + 3) / 4, n_planes), dim3(256), 0, st, t, (const uint8_t*)scratch, max_points, points);
    return (int)hipGetLastError();
}

extern "C" int svt_hip_launch_gm_cross_correlation(hipStream_t st, const uint8_t* im1, int stride1, const uint8_t* im2, int stride2, int w, int h, const int* pairs, int n,
                                                   double* out) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(gm_cross_correlation_kernel, dim3((n + 255) / 256), dim3(256), 0, st, im1, stride1, im2, stride2, w, h, pairs, n, out);
    return (int)hipGetLastError();
}

extern "C" int svt_hip_launch_gm_correspondences(hipStream_t st, const uint8_t* src, int src_stride, int w, int h, const int* src_points, const int* src_count,
                                                 const SvtHipGmRef* refs, int n_refs, const int* ref_points, const int* ref_counts, int max_points, int* corr, int* ncorr) {
    GmRefTab8 t = {};
    for (int i = 0; i < n_refs && i < SVT_HIP_GM_MAX_REFS; i++) t.r[i] = refs[i];
    hipLaunchKernelGGL(gm_match_kernel, dim3(max_points, n_refs), dim3(256), 0, st, src, src_stride, w, h, src_points, src_count, t, ref_points, ref_counts, max_points,
                       corr);
    hipLaunchKernelGGL(gm_corr_compact_kernel, dim3(n_refs), dim3(256), 0, st, src_count, max_points, corr, ncorr);
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(gm_front)
