// palette.hip — the palette luma search of a list of blocks and the screen-content detection of a picture on gfx950 (wave64), behind
// svt_hip_palette_search_batch_dev and svt_hip_screen_content_detect_dev.
//
// Replaces (file:line under Source/Lib of the reference):
//   Encoder/Codec/palette.c:320-496               search_palette_luma (with palette_rd_y :286-312 and svt_av1_palette_color_cost_y :144-153)
//   Encoder/Codec/k_means_template.h:32-133       svt_av1_calc_indices_dim1_c, svt_av1_k_means_dim1_c
//   Encoder/Codec/EbPictureAnalysisProcess.c:3364-3399, :3434-3601   svt_av1_count_colors[_highbd], is_valid_palette_nb_colors[_highbd], the per-pixel variance,
//                                                 is_screen_content
//
// Search: one workgroup of four waves per job.  The block's samples go to LDS once (at most 4096 of 16 bits) and into a histogram of 1 << bd LDS counters by
// ds_add (a block has few distinct values by the nature of the tool, so a sort would order 4096 keys to learn 64 of them; the adds of one value serialise, and that
// is a few hundred LDS cycles for a 64x64 block).  Wave 0 compacts the histogram to the block's distinct values in ascending order, one per lane (colors <= 64 or
// nothing is searched), and takes the eight dominant colours by eight wave maxima of count * 64 + (63 - lane): the largest count, and among equal counts the lowest
// value.  The fourteen candidate slots are then dealt to the four waves, k-means slots first.  A clustering is a wave with one lane per distinct value: the
// nearest centroid of a value is the nearest centroid of every sample that has it, so the per-cluster count and sum and the total distortion are wave sums of
// count-weighted terms, integer and therefore the sample-by-sample sums bit for bit; only the reseed of an empty cluster (data[rand % n]) reads a sample.  The
// centroids live in registers (loops over eight with the size as a guard: no run-time index).  After a barrier the tails of the fourteen candidates (cache snap,
// sort, duplicates, colour cost: palette.h, shared with the host form) run side by side, one lane each, over LDS arrays.  After another barrier every thread takes
// the prefix sum over the fourteen "kept" flags, which is the reference's order, and the workgroup writes the kept records and their maps, four map bytes per
// thread and store.
//
// Detection: a wave per 16x16 block, lane = column + 16 * (row & 3), four rows apart per lane; the distinct values are counted by taking a remaining value from
// the first lane that has one and striking it everywhere, at most five times; sums by row16_sum / rows_total.  A wave walks eight blocks of a block row, a
// workgroup adds its four waves' counts in LDS and makes two global adds; a one-thread kernel takes the two comparisons.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "fmt_dispatch.h"
#include "lane_reduce.h"
#include "palette.h"

namespace {

#define PD __device__ __forceinline__

constexpr int WG = 256, WAVES = WG / 64;

PD void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }

// svt_av1_calc_indices_dim1_c on registers: the first nearest of c[0 .. k); *dist, if asked for, is its squared distance
PD int nearest_reg(int v, const int (&c)[8], int k, int* dist = nullptr) {
    int best = 0, min_dist = (v - c[0]) * (v - c[0]);
#pragma unroll
    for (int j = 1; j < 8; ++j) {
        const int d = (v - c[j]) * (v - c[j]);
        if (j < k && d < min_dist) {
            min_dist = d;
            best = j;
        }
    }
    if (dist) *dist = min_dist;
    return best;
}

// calc_total_dist: every sample's squared distance to its centroid, summed over the distinct values times their counts.  Centroids are means or members of the
// data, so a distance is at most ub - lb <= 1023 and the total at most 4096 * 1023 * 1023 = 4 286 582 784 < 2^32: the 32-bit sum is exact up to bit depth 10.
constexpr int MAX_BD = 10;
static_assert((unsigned long long)pal::MAX_SAMPLES * ((1 << MAX_BD) - 1) * ((1 << MAX_BD) - 1) < (1ull << 32), "calc_total_dist in 32 bits");
PD uint32_t weighted_dist(int dist, int cnt) { return wave_sum_u32((uint32_t)dist * (uint32_t)cnt); }

// svt_av1_k_means_dim1_c of a wave: lane i holds the i-th distinct value of the block and its count (count 0 beyond the last), c[0 .. k) the centroids, wave-uniform
// in and out; samp[0 .. nsamp) the block's samples in raster order
PD void k_means_wave(int (&c)[8], int k, int val, int cnt, const uint16_t* samp, int nsamp) {
    int d;
    int idx = nearest_reg(val, c, k, &d);
    uint32_t this_dist = weighted_dist(d, cnt);
    for (int it = 0; it < pal::MAX_ITR; ++it) {
        const uint32_t pre_dist = this_dist;
        int pre[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) pre[j] = c[j];
        uint32_t rand_state = samp[0];   // calc_centroids seeds from data[0] on every call
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < k) {
                const int count = (int)wave_sum_u32(idx == j ? (uint32_t)cnt : 0u), sum = (int)wave_sum_u32(idx == j ? (uint32_t)(cnt * val) : 0u);
                c[j] = count == 0 ? (int)samp[pal::lcg_rand16(&rand_state) % (uint32_t)nsamp] : pal::div_round(sum, count);
            }
        }
        idx = nearest_reg(val, c, k, &d);
        this_dist = weighted_dist(d, cnt);
        if (this_dist > pre_dist) {   // not reachable in one dimension (docs/kernels/palette.md); kept as the reference has it
#pragma unroll
            for (int j = 0; j < 8; ++j) c[j] = pre[j];
            break;
        }
        bool same = true;
#pragma unroll
        for (int j = 0; j < 8; ++j) same = same && (j >= k || c[j] == pre[j]);
        if (same) break;
    }
}

template <class PIX, int BD> __global__ __launch_bounds__(WG) void palette_search_kernel(const PIX* __restrict__ plane, int stride, const SvtHipPaletteJob* __restrict__ jobs,
                                                                                         SvtHipPaletteResult* __restrict__ results, SvtHipPaletteCand* __restrict__ cands,
                                                                                         uint8_t* __restrict__ maps) {
    constexpr int BINS = 1 << BD;
    static_assert(BD <= MAX_BD, "weighted_dist");
    __shared__ SvtHipPaletteJob  s_job;
    __shared__ uint16_t          s_samp[pal::MAX_SAMPLES];
    __shared__ int               s_hist[BINS];
    __shared__ uint16_t          s_val[pal::MAX_COLORS], s_cnt[pal::MAX_COLORS];
    __shared__ int               s_top[pal::MAX_SIZE], s_colors, s_out_of_range;
    __shared__ SvtHipPaletteCand s_rec[pal::MAX_CANDS];
    __shared__ int               s_cent[pal::MAX_CANDS][pal::MAX_SIZE];   // a slot's centroids: raw, then sorted and distinct
    __shared__ int               s_n[pal::MAX_CANDS], s_size[pal::MAX_CANDS];   // the centroids a slot starts from (0: empty slot), the palette size of a kept slot (0: not kept)
    __shared__ int               s_work[pal::MAX_CANDS][pal::MAX_SIZE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, job = blockIdx.x;

    static_assert(sizeof(SvtHipPaletteJob) % 4 == 0, "copied by words");
    if (tid < (int)(sizeof(SvtHipPaletteJob) / 4)) ((uint32_t*)&s_job)[tid] = ((const uint32_t*)(jobs + job))[tid];
    for (int i = tid; i < BINS; i += WG) s_hist[i] = 0;
    if (tid == 0) s_out_of_range = 0;
    __syncthreads();
    if (!pal::job_ok(s_job)) {   // the same for every thread
        if (tid == 0) results[job] = SvtHipPaletteResult{-1, 0};
        return;
    }
    const int bw = s_job.bw, bh = s_job.bh, cols = s_job.cols, rows = s_job.rows, nsamp = rows * cols;
    const PIX* src = plane + (size_t)s_job.y * stride + s_job.x;
#pragma unroll 4   // up to 16 rounds for a 64x64 block: the loads of four rounds in flight together
    for (int i = tid; i < nsamp; i += WG) {
        const int r = i / cols, cc = i - r * cols;
        const int v = src[(size_t)r * stride + cc];
        s_samp[i] = (uint16_t)v;
        if (v < BINS) atomicAdd(&s_hist[v], 1);
        else s_out_of_range = 1;
    }
    __syncthreads();
    if (wave == 0) {
        int total = 0;
        for (int base = 0; base < BINS; base += 64) {
            const int cn = s_hist[base + lane];
            const unsigned long long m = __ballot(cn > 0);
            const int pos = total + __popcll(m & ((1ull << lane) - 1));
            if (cn > 0 && pos < pal::MAX_COLORS) {
                s_val[pos] = (uint16_t)(base + lane);
                s_cnt[pos] = (uint16_t)cn;
            }
            total += __popcll(m);
        }
        if (s_out_of_range) total = 0;   // svt_av1_count_colors_highbd returns 0 for a sample that is not below 1 << bit_depth
        wave_sync();
        if (total > 1 && total <= pal::MAX_COLORS) {
            int cn = lane < total ? s_cnt[lane] : 0;
            const int v = lane < total ? s_val[lane] : 0;
            const int nmax = total < pal::MAX_SIZE ? total : pal::MAX_SIZE;
            for (int i = 0; i < nmax; ++i) {
                const uint32_t best = ~wave_min_u32(~(cn > 0 ? ((uint32_t)cn << 6) | (uint32_t)(63 - lane) : 0u));   // the maximum, by DPP
                const int winner = 63 - (int)(best & 63);
                if (lane == winner) {
                    s_top[i] = v;
                    cn = 0;
                }
            }
        }
        if (lane == 0) s_colors = total;
    }
    __syncthreads();
    const int colors = s_colors;
    if (!(colors > 1 && colors <= pal::MAX_COLORS)) {
        if (tid == 0) results[job] = SvtHipPaletteResult{colors, 0};
        return;
    }
    const int nmax = colors < pal::MAX_SIZE ? colors : pal::MAX_SIZE, lb = s_val[0], ub = s_val[colors - 1];
    const int val = lane < colors ? s_val[lane] : 0, cnt = lane < colors ? s_cnt[lane] : 0;
    for (int t = wave; t < pal::MAX_CANDS; t += WAVES) {
        const int slot = t < 7 ? 7 + t : t - 7;   // the clusterings first: they are the long tasks
        const int n = pal::slot_n(slot, nmax, s_job.dominant_step), kind = pal::slot_kind(slot);
        if (n < 2) {
            if (lane == 0) s_n[slot] = 0;
            continue;
        }
        int c[8];
        if (!kind) {
#pragma unroll
            for (int j = 0; j < 8; ++j) c[j] = s_top[j < n ? j : 0];
        } else if (colors == 2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) c[j] = j == 0 ? lb : ub;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) c[j] = pal::init_centroid(j < n ? j : 0, n, lb, ub);
            k_means_wave(c, n, val, cnt, s_samp, nsamp);
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) s_cent[slot][j] = c[j];
            s_n[slot] = n;
        }
    }
    __syncthreads();
    // the tails of the fourteen candidates side by side, one lane each: serial code over LDS, whose latency the slots then share
    if (tid < pal::MAX_CANDS) {
        const int n = s_n[tid];
        const int k = n >= 2 ? pal::finish_candidate(s_cent[tid], n, pal::slot_kind(tid), s_job.cache, s_job.n_cache, BD, s_work[tid], &s_rec[tid]) : 0;
        s_size[tid] = k > 2 ? k : 0;
    }
    __syncthreads();
    // palette_cand[] in the reference's order: a kept slot's place is the number of kept slots before it
    int n_cands = 0, my_place = 0;
    for (int s = 0; s < pal::MAX_CANDS; ++s) {
        if (s == tid) my_place = n_cands;
        n_cands += s_size[s] > 0;
    }
    if (tid == 0) results[job] = SvtHipPaletteResult{colors, n_cands};
    if (tid < pal::MAX_CANDS && s_size[tid] > 0) cands[(size_t)job * pal::MAX_CANDS + my_place] = s_rec[tid];
    const int area = bw * bh, bw_log2 = __ffs(bw) - 1;
    uint8_t* job_maps = maps + s_job.map_off;
    int place = 0;
    for (int s = 0; s < pal::MAX_CANDS; ++s) {
        const int k = s_size[s];
        if (!k) continue;
        int c[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = s_cent[s][j < k ? j : 0];
        uint8_t* map = job_maps + (size_t)place * area;
        for (int p = 4 * tid; p < area; p += 4 * WG) {   // bw is a multiple of 4: the four positions are of one row
            const int py = p >> bw_log2, px = p & (bw - 1);
            uint32_t packed = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) packed |= (uint32_t)nearest_reg(s_samp[pal::extended_sample_index(px + e, py, cols, rows)], c, k) << (8 * e);
            if (((uintptr_t)(map + p) & 3) == 0) *(uint32_t*)(map + p) = packed;
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) map[p + e] = (uint8_t)(packed >> (8 * e));
            }
        }
        ++place;
    }
}

// ---------------------------------------------------------------------------------------------------------------- screen-content detection
constexpr int SC_WAVE_BLOCKS = 8, SC_WG_BLOCKS = SC_WAVE_BLOCKS * WAVES;

template <class PIX> __global__ __launch_bounds__(WG) void screen_content_kernel(const PIX* __restrict__ plane, int stride, int blocks_x, int32_t* __restrict__ out) {
    __shared__ int s_counts[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, row = lane >> 4;
    constexpr int OFFS = sizeof(PIX) == 1 ? 128 : 512;   // eb_av1_var_offs / eb_AV1_HIGH_VAR_OFFS_10
    if (tid < 2) s_counts[tid] = 0;
    __syncthreads();
    int counts_1 = 0, counts_2 = 0;
    const int first = blockIdx.x * SC_WG_BLOCKS + wave * SC_WAVE_BLOCKS;
    for (int b = first; b < first + SC_WAVE_BLOCKS && b < blocks_x; ++b) {
        const PIX* p = plane + (size_t)(blockIdx.y * 16 + row) * stride + b * 16 + col;
        int v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = p[(size_t)(4 * i) * stride];
        // is_valid_palette_nb_colors with threshold 4: more than one colour, at most four
        unsigned left = 15;   // which of this lane's four samples have a value not yet counted
        int nb_colors = 0;
        for (;;) {
            const unsigned long long m = __ballot(left != 0);
            if (!m) break;
            const int mine = (left & 1) ? v[0] : ((left & 2) ? v[1] : ((left & 4) ? v[2] : v[3]));
            const int pick = __shfl(mine, __ffsll((long long)m) - 1, 64);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (v[i] == pick) left &= ~(1u << i);
            if (++nb_colors > 4) break;
        }
        if (nb_colors <= 1 || nb_colors > 4) continue;   // wave-uniform
        int d_sum = 0;
        uint32_t d_sse = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = v[i] - OFFS;
            d_sum += d;
            d_sse += (uint32_t)(d * d);
        }
        const int      sum = (int)wave_sum_u32((uint32_t)d_sum);   // |sum| <= 256 * 512, sse <= 256 * 512 * 512
        const uint32_t sse = wave_sum_u32(d_sse);
        uint32_t       var;
        if constexpr (sizeof(PIX) == 1) {
            var = sse - (uint32_t)(((int64_t)sum * sum) / 256);   // svt_aom_variance16x16_c
        } else {                                                  // svt_aom_highbd_10_variance16x16_c
            const uint32_t sse10 = (uint32_t)(((uint64_t)sse + 8) >> 4);
            const int      sum10 = (int)(((int64_t)sum + 2) >> 2);
            const int64_t  v64 = (int64_t)sse10 - ((int64_t)sum10 * sum10) / 256;
            var = v64 >= 0 ? (uint32_t)v64 : 0;
        }
        ++counts_1;
        counts_2 += (int)((var + 128) >> 8) > 0;   // ROUND_POWER_OF_TWO(var, num_pels_log2_lookup[BLOCK_16X16]) > var_thresh
    }
    if (lane == 0 && counts_1) {
        atomicAdd(&s_counts[0], counts_1);
        atomicAdd(&s_counts[1], counts_2);
    }
    __syncthreads();
    if (tid < 2 && s_counts[tid]) atomicAdd(&out[tid], s_counts[tid]);
}

__global__ void screen_content_decide_kernel(int32_t* out, int width, int height) {
    const int64_t counts_1 = out[0], counts_2 = out[1], area = (int64_t)width * height;
    const int     color_detection = counts_1 * 16 * 16 * 10 > area;
    out[2] = color_detection;
    out[3] = color_detection && counts_2 * 16 * 16 * 12 > area;
}

}  // namespace

int svt_hip_launch_palette_search(hipStream_t st, int pix_bytes, int bd, const void* plane, int stride, const SvtHipPaletteJob* jobs, int njobs, SvtHipPaletteResult* results,
                                  SvtHipPaletteCand* cands, uint8_t* maps) {
    svt_for_fmt(pix_bytes, bd, [&](auto f) {
        using PIX = typename decltype(f)::pix;
        hipLaunchKernelGGL((palette_search_kernel<PIX, decltype(f)::bd>), dim3(njobs), dim3(WG), 0, st, (const PIX*)plane, stride, jobs, results, cands, maps);
    });
    return (int)hipGetLastError();
}

int svt_hip_launch_screen_content_detect(hipStream_t st, int pix_bytes, const void* plane, int stride, int width, int height, int32_t* out) {
    const hipError_t e = hipMemsetAsync(out, 0, 4 * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const int blocks_x = width / 16, blocks_y = height / 16;
    if (blocks_x && blocks_y)
        svt_for_pix(pix_bytes, [&](auto f) {
            using PIX = typename decltype(f)::pix;
            hipLaunchKernelGGL((screen_content_kernel<PIX>), dim3((blocks_x + SC_WG_BLOCKS - 1) / SC_WG_BLOCKS, blocks_y), dim3(WG), 0, st, (const PIX*)plane, stride, blocks_x, out);
        });
    hipLaunchKernelGGL(screen_content_decide_kernel, dim3(1), dim3(1), 0, st, out, width, height);
    return (int)hipGetLastError();
}

SVT_HIP_TU_PROBE(palette)
